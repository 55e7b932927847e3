"""The routing decision for contractions (csrc/gemm_route.cpp) against a table RECORDED FROM THE PARENT of the
commit that made the decision one function: tests/golden/gemm_routes.txt holds, for every problem of its grid, the kernel
families the cascade launched in order and what gemm_epilogue_ok / gemm_small_route answered.  Its first line is the grid
(and the commit and the placement probe's verdict of the recording box); to_gemm_route_query must say the same, launching
nothing.  A deliberate routing change re-records the rows it moves."""
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes.txt")


@pytest.fixture(scope="module")
def T():
    from tensor_ops_amd.hipt import HipT
    return HipT(0)


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        head = json.loads(f.readline())
        lines = f.read().split()
    shapes = [list(s) for s in itertools.product(head["V"], repeat=3)] + head["extra"]
    assert len(lines) == len(shapes)
    return head, shapes, lines


def rows_of(head, line):
    """(dtype, ta, tb, epilogue, batch, reduced, recorded outcome) of one shape's line, in the order it was recorded"""
    A, w = head["alphabet"], head["width"]
    combos = itertools.product(head["dtypes"], head["layouts"], head["epilogues"], head["batches"])
    assert len(line) == w * len(head["dtypes"]) * len(head["layouts"]) * len(head["epilogues"]) * len(head["batches"])
    for i, (dt, (ta, tb), epi, (batch, red)) in enumerate(combos):
        code = 0
        for ch in line[i * w:(i + 1) * w]:
            code = code * len(A) + A.index(ch)
        yield dt, ta, tb, epi, batch, red, head["outcomes"][code]


def test_every_recorded_route_and_predicate_answer(T, table):
    from tensor_ops_amd.capi import GEMM_FAMILIES
    head, shapes, lines = table
    if T.gemm_route(64, 64, 64)["split_workspace"] != head["split_workspace"]:
        pytest.skip("the placement probe says %s here, the table was recorded where it said %s"
                    % (not head["split_workspace"], head["split_workspace"]))
    l0 = T.stats()["launches"]
    bad, rows = [], 0
    for (m, k, n), line in zip(shapes, lines):
        for dt, ta, tb, epi, batch, red, want in rows_of(head, line):
            got = T.gemm_route(m, k, n, dtype=dt, batch=batch, reduce_batch=red, a_transposed=ta, b_transposed=tb, epilogue=epi)
            rows += 1
            fam = want["families"] and [GEMM_FAMILIES[f] for f in want["families"]]
            if (got["families"], got["epilogue_ok"], got["small_route"]) != (fam, bool(want["epilogue_ok"]), bool(want["small_route"])):
                bad.append(((m, k, n), dt, ta, tb, epi, batch, red, got, want))
    assert T.stats()["launches"] == l0
    assert rows == 120 * len(shapes) >= 160000
    assert not bad, (len(bad), bad[:5])


# The smallest fp32 rows of the table (operands contiguous, no epilogue, one product) whose recorded plan has two or more
# launches, one per split kind: a K tail (head K = 288, tail K = 12); a block of whole 128 x 128 tiles (896 x 896) with its two
# strips; a block of whole rounds of 256 x 256 tiles (4096 x 4096) with its two strips.
SPLITS = {"k_tail": (256, 300, 256), "block_128": (1001, 512, 1003), "block_256": (4097, 304, 4097)}


@pytest.mark.parametrize("kind", sorted(SPLITS))
def test_split_plans_compute_the_whole_product(T, table, kind):
    """The whole output of a split plan, exact on small integers (every product and partial sum is exact in fp32 whatever the
    summation order), at least one launch per leaf."""
    head, shapes, lines = table
    m, k, n = SPLITS[kind]
    recorded = next(rows_of(head, lines[shapes.index([m, k, n])]))
    assert recorded[:6] == ("f32", 0, 0, [], 1, 0) and len(recorded[6]["families"]) >= 2
    leaves = T.gemm_route(m, k, n)["families"]
    assert len(leaves) >= 2, (m, k, n, leaves)
    rng = np.random.default_rng(m + k + n)
    a = rng.integers(-2, 3, size=(m, k)).astype(np.float32)
    b = rng.integers(-2, 3, size=(k, n)).astype(np.float32)
    da, db = T.put(a), T.put(b)
    l0 = T.stats()["launches"]
    got = T.gmul(1, 1, 1, da, db).numpy()
    assert T.stats()["launches"] - l0 >= len(leaves)
    assert np.array_equal(got, a @ b), (m, k, n)   # (a @ b in fp32 is exact too: integers below 2^24)
