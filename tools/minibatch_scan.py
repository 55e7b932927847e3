"""One shuffled pass of minibatch SGD over a resident data set, four ways.  Per (dtype, stack, M): samples/s of
  (a) loop     the host loop of entry points that were there before: to_batch_gather (X), to_batch_gather (Y),
               to_fflayer_stack_sgd, per step
  (b) onecall  to_fflayer_stack_minibatch_sgd over the permutation at the default stage bound
  (c) 1-step   the same with one-step chunks (to_set_minibatch_stage_bytes(1)): a staging launch per step -- what the
               amortising of (b) buys
  (d) no idx   the same with idx null (rows in place: no staging at all)
Each is one blocking pass (the call(s), then to_sync); the four alternate, `--reps` (5) rounds after one warm-up round;
the median is reported, for (a) also its spread max - min over the rounds.  `verdict`: (b) is "ok" unless its median pass
is slower than (a)'s by more than (a)'s spread.
usage: minibatch_scan.py [--dtype f32,f64] [--M 16,128,1024] [--rows 60000] [--stacks 784-256-10,784-300-100-10] [--reps 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tensor_ops_amd.hipt import HipT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32,f64")
    ap.add_argument("--M", default="16,128,1024")
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--stacks", default="784-256-10,784-300-100-10")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    N = a.rows
    print("minibatch SGD, one pass over %d synthetic rows in a shuffled order, rate 1e-3; samples/s (median of %d)" % (N, a.reps))
    print("%5s %16s %5s | %12s %12s %12s | %12s %12s %12s | %7s" %
          ("dtype", "stack", "M", "(a) loop", "(a) min", "(a) max", "(b) onecall", "(c) 1-step", "(d) no idx", "verdict"))
    for dname in a.dtype.split(","):
        dt = np.float32 if dname == "f32" else np.float64
        T = HipT(0, dt)
        X = rng.uniform(0, 1, (N, 784)).astype(dt)
        labels = rng.integers(0, 10, N)
        x = T.put(X, batched=True)
        for stack in a.stacks.split(","):
            sizes = [int(v) for v in stack.split("-")]
            Y = np.zeros((N, sizes[-1]), dt)
            Y[np.arange(N), labels % sizes[-1]] = 1
            y = T.put(Y, batched=True)
            ws = [((0.1 * rng.standard_normal((o, i))).astype(dt), (0.1 * rng.standard_normal(o)).astype(dt))
                  for i, o in zip(sizes[:-1], sizes[1:])]
            for M in [int(v) for v in a.M.split(",")]:
                W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
                perm = rng.permutation(N).astype(np.int64)

                def loop():
                    for s in range(0, N, M):
                        idx = perm[s:s + M]
                        T.stack_sgd(W, b, T.batch_gather(x, idx), T.batch_gather(y, idx), 1e-3)

                def onecall(bound, idx):
                    HipT.minibatch_stage_bytes(bound)
                    try:
                        T.stack_minibatch_sgd(W, b, x, y, 1e-3, M, idx=idx, n=N)
                    finally:
                        HipT.minibatch_stage_bytes(0)

                ways = [("a", loop), ("b", lambda: onecall(0, perm)), ("c", lambda: onecall(1, perm)),
                        ("d", lambda: onecall(0, None))]
                secs = {k: [] for k, _ in ways}
                try:
                    for rep in range(a.reps + 1):
                        for k, f in ways:
                            T.sync()
                            t0 = time.perf_counter(); f(); T.sync(); t = time.perf_counter() - t0
                            if rep > 0:          # (round 0 warms every way up)
                                secs[k].append(t)
                except Exception as e:          # a row is information: say why it is missing and go on
                    print("%5s %16s %5d | failed: %s" % (dname, stack, M, str(e)[:100]), flush=True)
                    continue
                med = {k: float(np.median(v)) for k, v in secs.items()}
                spread = max(secs["a"]) - min(secs["a"])
                verdict = "ok" if med["b"] - med["a"] <= spread else "MISS"
                print("%5s %16s %5d | %12.0f %12.0f %12.0f | %12.0f %12.0f %12.0f | %7s" %
                      (dname, stack, M, N / med["a"], N / max(secs["a"]), N / min(secs["a"]), N / med["b"], N / med["c"],
                       N / med["d"], verdict), flush=True)


if __name__ == "__main__":
    main()
