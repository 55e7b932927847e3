"""What the planner (csrc/lazy*.cpp) decides for a fixed list of scenarios, one line each -- the table tests/golden/lazy_plans.txt
was recorded with (from the parent of the commit that made a plan's decisions one record) and tests/test_gpu_lazy_plans.py
compares against:

  <id> <sha256 of the scenario's TOPS_LAZY_DEBUG text> <launches> <recorded> <fused> <elided> <flushes> <hits> <misses> <sha256 of the results>

The scenarios run in ONE fresh child process with TOPS_LAZY_DEBUG=1 (the variable is read once per process); the child writes a
marker line to stderr before each scenario, so the plan text between two markers belongs to one scenario.  The `refs a/b vN`
tokens of dump_plan are host reference counts (a garbage collector's business) and are removed before hashing.  The plan cache
is cleared before every scenario: what a scenario hits it has stored itself.

  python tools/lazy_plan_record.py                 the table on stdout
  python tools/lazy_plan_record.py --text FILE     ... and every scenario's full plan text into FILE (for diffing by hand)
  python tools/lazy_plan_record.py --merge A B     the golden file out of two recordings of one build: a scenario whose plan
                                                   text or counts differ between them is dropped, one whose result digest alone
                                                   differs keeps `*` for a digest (compared on plan text and counts only)
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "@@lazy-plan-scenario "
FUZZ_CASES = range(60)
STEP_SEED = 0x7e500070


# ---- the scenarios (child process) -----------------------------------------------------------------------------------------
def _fuzz_case(F, case):
    """the program, inputs and demands of case `case` of test_recorded_programs_with_values_forced_and_dropped_midway"""
    import numpy as np
    rng = np.random.default_rng(F.SEED + 2000003 + case)
    fam2 = bool(case % 2)
    leaves, steps, kinds, sizes = F.build_program2(rng) if fam2 else F.build_program(rng, extended=(case % 4 == 2))
    if not steps:
        return None
    B = sizes["B"]
    inputs = {}
    for name, kind in leaves.items():
        shape = (((B,) if kind[2] else ()) + (kind[1],)) if kind[0] == "vec" else (kind[1], kind[2])
        inputs[name] = rng.uniform(0, 1, size=shape) if (fam2 and name == "y") else rng.uniform(-1, 1, size=shape)
    produced = [st[1] for st in steps if st[0] not in ("copy", "copy_many")]
    k = int(rng.integers(1, len(produced) + 1))
    demand = [produced[i] for i in rng.permutation(len(produced))[:k]]
    late = set(d for d in demand if rng.random() < 0.25)
    last_use = {}
    for i, st in enumerate(steps):
        for v in F._inputs_of(st):
            last_use[v] = i
    out, nf = [], 0
    for i, st in enumerate(steps):
        out.append(st)
        made = [s2[1] for s2 in steps[:i + 1] if s2[0] not in ("copy", "copy_many")]
        if rng.random() < 0.12:
            out.append(("force", "force%d" % nf, made[int(rng.integers(len(made)))]))
            nf += 1
        for v in made:
            if v not in demand and last_use.get(v, -1) <= i and rng.random() < 0.3 and ("drop", "", v) not in out \
                    and not any(o[0] == "force" and o[2] == v for o in out[-1:]):
                out.append(("drop", "", v))
    dropped, steps2 = set(), []
    for st in out:
        if st[0] == "drop":
            dropped.add(st[2])
        if st[0] == "force" and st[2] in dropped:
            continue
        steps2.append(st)
    forced = [st[1] for st in steps2 if st[0] == "force"]
    return leaves, steps2, inputs, demand, late, demand + forced


def _net_problem(rng, B, i, h, o):
    import numpy as np
    ws = [(0.5 * rng.standard_normal((h, i)), 0.5 * rng.standard_normal(h)),
          (0.5 * rng.standard_normal((o, h)), 0.5 * rng.standard_normal(o))]
    X = rng.uniform(0, 1, size=(B, i))
    Y = np.zeros((B, o))
    Y[np.arange(B), rng.integers(0, o, size=B)] = 1.0
    return ws, X, Y


def scenarios():
    """[(id, thunk)]: a thunk runs the scenario and returns the demanded results (numpy arrays, in order)"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_lazy_fuzz as F
    from tensor_ops_amd import tops
    from tensor_ops_amd.hipt import HipT
    T32 = HipT(0)
    out = []

    for dt, T in (("f32", T32), ("f64", HipT(0, dtype=np.float64))):
        for case in FUZZ_CASES:
            def fuzz(T=T, case=case):
                c = _fuzz_case(F, case)
                if c is None:
                    return []
                leaves, steps, inputs, demand, late, names = c
                res = []
                for _ in range(2):         # (the second run finds the first one's plans in the cache)
                    r = F.run_program(T, leaves, steps, inputs, demand, True, late)
                    res += [r[n] for n in names]
                return res
            out.append(("fuzz-%s-%02d" % (dt, case), fuzz))

    def step(sizes, B, hidden, head, loss, then=None, graph=False, seed=0):
        def run():
            T = T32
            rng = np.random.default_rng(STEP_SEED + seed)
            ws, X, Y = _net_problem(rng, B, *sizes)
            net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], hidden, head)
            if then is not None:
                net = tops.net_then(net, tops.scale(then))
            tr = tops.Trainer(net, loss, 0.01 / B, T.put(X, batched=True), T.put(Y, batched=True), use_graph=graph)
            for _ in range(3):
                tr.step()
            return [p.numpy() for p in tr.net.params]
        return run

    for B in (256, 1):
        out.append(("step-smce-%d" % B, step((96, 48, 10), B, "actMapLogistic", "actSoftmax", "crossEntropy", seed=1)))
        out.append(("step-logse-%d" % B, step((96, 48, 10), B, "actMapLogistic", "actLogistic", "squaredError", seed=2)))
    # (the loss head takes its tail -- dH = (dZ W) * h(1-h) -- from eight 16-wide chunks of hidden units on)
    out.append(("step-tail", step((96, 128, 10), 256, "actMapLogistic", "actSoftmax", "crossEntropy", seed=7)))
    out.append(("step-rowprog", step((30, 17, 20), 50, "actMapTanh", "actSoftmax", "squaredError", then=0.5, seed=3)))
    # the narrowest hidden layer whose weight gradient (dW1 = dZ1^T X with its update and row sums) is beyond the small-GEMM range
    n_in, rows = 784, 32
    wide = next(h for h in range(1, 1 << 14)
                if not T32.gemm_route(h, rows, n_in, a_transposed=True, epilogue=("beta", "rowsum"))["small_route"])
    out.append(("step-wide", step((n_in, wide, 10), rows, "actMapLogistic", "actSoftmax", "crossEntropy", seed=4)))
    out.append(("step-captured", step((96, 48, 10), 256, "actMapLogistic", "actSoftmax", "crossEntropy", graph=True, seed=5)))

    def siblings():
        T = T32
        rng = np.random.default_rng(STEP_SEED + 6)
        As = [T.put(rng.integers(-2, 3, (2048, 16)).astype(np.float32)) for _ in range(64)]
        Bm = T.put(rng.integers(-2, 3, (16, 256)).astype(np.float32))
        f = T.expr(lambda v: v[0] * v[0] - v[0], 1, key="lazy-plan-record-sq")   # (nothing a GEMM epilogue carries)
        with T.memo():
            Cs = [T.gmul(1, 1, 1, a, Bm) for a in As]
            Ls = [T.liftT(f, [c]) for c in Cs]
            T.force_many(Ls)
        return [x.numpy() for x in Ls]
    out.append(("siblings-64", siblings))
    return T32, out


def child():
    from tensor_ops_amd import capi
    T, todo = scenarios()

    def counts():
        a = [C.c_int64() for _ in range(4)]
        capi.check(capi.lib().to_lazy_stats(*[C.byref(v) for v in a]))
        b = [C.c_int64() for _ in range(3)]
        capi.check(capi.lib().to_plan_cache_stats(*[C.byref(v) for v in b]))
        return [T.stats()["launches"]] + [v.value for v in a] + [b[0].value, b[1].value]

    for sid, run in todo:
        capi.check(capi.lib().to_plan_cache_clear())
        sys.stderr.flush()
        os.write(2, (MARK + sid + "\n").encode())
        c0 = counts()
        res = run()
        c1 = counts()
        dg = hashlib.sha256()
        for r in res:
            dg.update(repr((r.shape, str(r.dtype))).encode())
            dg.update(r.tobytes())
        print(json.dumps({"id": sid, "counts": [b - a for a, b in zip(c0, c1)], "results": dg.hexdigest()}), flush=True)
    os.write(2, (MARK + "end\n").encode())


# ---- the table (parent process) -------------------------------------------------------------------------------------------
def plan_texts(stderr):
    """{scenario id: its [lazy] lines, reference counts removed}"""
    texts, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith(MARK):
            cur = line[len(MARK):].strip()
            texts[cur] = []
        elif cur is not None and (line.startswith("[lazy]") or line.startswith("  ")):
            texts[cur].append(re.sub(r"  refs \d+/\d+ v\d+", "", line))
    return {k: "\n".join(v) + "\n" for k, v in texts.items() if k != "end"}


def record(text_file=None, timeout=900):
    env = dict(os.environ, TOPS_LAZY_DEBUG="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError("the scenario process failed (%d):\n%s" % (r.returncode, r.stderr[-4000:]))
    texts = plan_texts(r.stderr)
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["id"] for row in rows] == list(texts), "scenario markers and result lines do not line up"
    if text_file:
        with open(text_file, "w") as f:
            for sid, t in texts.items():
                f.write(MARK + sid + "\n" + t)
    return ["%s %s %s %s" % (row["id"], hashlib.sha256(texts[row["id"]].encode()).hexdigest(),
                             " ".join(str(c) for c in row["counts"]), row["results"]) for row in rows]


def text_of(text_file, sid):
    with open(text_file) as f:
        parts = f.read().split(MARK)
    return next((p.split("\n", 1)[1] for p in parts if p.split("\n", 1)[0] == sid), "")


def merge(a_file, b_file, parent):
    a, b = ([line.split() for line in open(f).read().splitlines() if line and not line.startswith("{")] for f in (a_file, b_file))
    assert [r[0] for r in a] == [r[0] for r in b]
    kept, dropped = [], []
    for ra, rb in zip(a, b):
        if ra[:-1] != rb[:-1]:
            dropped.append(ra[0])
        else:
            kept.append(ra if ra[-1] == rb[-1] else ra[:-1] + ["*"])
    head = {"parent": parent, "scenarios": [r[0] for r in kept], "dropped": dropped,
            "columns": "id plan_text_sha256 launches recorded fused_launches elided flushes cache_hits cache_misses results_sha256"}
    return "\n".join([json.dumps(head)] + [" ".join(r) for r in kept]) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--text")
    ap.add_argument("--merge", nargs=2)
    ap.add_argument("--parent", default="")
    args = ap.parse_args()
    if args.child:
        child()
    elif args.merge:
        sys.stdout.write(merge(args.merge[0], args.merge[1], args.parent))
    else:
        print("\n".join(record(args.text)))
