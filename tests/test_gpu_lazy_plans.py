"""The planner's decisions (csrc/lazy_plan.cpp, lazy_cache.cpp, lazy_exec.cpp) against a table RECORDED FROM THE PARENT of the
commit that made a plan's decisions one record: tests/golden/lazy_plans.txt holds, for every scenario of
tools/lazy_plan_record.py -- sixty random recorded programs in both element types, each run twice so that the second run comes
out of the plan cache; training steps that reach the loss head, its tail, the pair, the chain, the rank-1 unit, a row program, a
weight gradient beyond the small-GEMM range, a captured step; a scope of sibling products and lifts -- the digest of the
TOPS_LAZY_DEBUG text of its flushes, its launch / planner / plan-cache counts and the digest of its results.  A deliberate
change of a fusion rule re-records the lines it moves."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lazy_plans.txt")


def test_every_scenario_plans_launches_and_computes_what_the_parent_did(repo_root, tmp_path):
    sys.path.insert(0, os.path.join(repo_root, "tools"))
    try:
        import lazy_plan_record as R
    finally:
        sys.path.pop(0)
    with open(GOLDEN) as f:
        head = json.loads(f.readline())
        want = {line.split()[0]: line.split() for line in f.read().splitlines() if line}
    assert list(want) == head["scenarios"] and len(want) >= 100
    text_file = str(tmp_path / "plans.txt")
    got = {line.split()[0]: line.split() for line in R.record(text_file, timeout=600)}
    bad = []
    for sid, w in want.items():
        g = got.get(sid)
        if g is not None and w[-1] == "*":      # (its result bits differed between two runs of the parent itself)
            g = g[:-1] + ["*"]
        if g != w:
            bad.append(sid)
            print("---- %s\n  recorded %s\n  now      %s\n%s" % (sid, " ".join(w), g and " ".join(g), R.text_of(text_file, sid)))
    assert not bad, bad
