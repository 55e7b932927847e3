"""to_rnn_stack_minibatch_sgd next to the loop a caller had to write before it: fp32, N = 256 sequences, M sequences an update,
softmax head over a stateless output layer, logistic states and hidden layers:
  5 -> 7 (stateful) -> 5 and 64 -> H (stateful) -> 10 for H = 32 / 64 / 128;  T in {8, 64};  M in {4, 16, 64}
Per (stack, T, M), microseconds per UPDATE, median of `--reps` (7) after one warm-up round, the three ways alternating:
  caller      a loop of to_batch_gather (X and Y) + to_rnn_stack_sgd over the minibatches -- the yardstick: what the same
              training cost before the entry existed (unchanged entries, same process)
  route A     to_rnn_stack_minibatch_sgd per minibatch (to_set_rnn_minibatch_persistent 0)
  route B     to_rnn_stack_minibatch_sgd persistent (2); "(route A: no plan)" where the plan does not exist and route A ran
A way is timed with the host clock around the blocking call(s).  Every way trains its own copy of the parameters, all from
the same start, on the same permutation of the sequences; small rates keep the updates finite.  spread: the largest
(max - min) / median of a way's repetitions in the row.  Verdict: AHEAD where route B's median is below both others' by more
than that spread -- the rows the automatic rule of to_set_rnn_minibatch_persistent may name --, else LOSS (or WITHIN the
spread).  The scan runs in a child process under a time limit (`--limit` seconds; at the limit the child's process group is
killed); a child that fails ends the tool with status 1 after it has written what it measured.
usage: rnn_minibatch_scan.py [--N 256] [--T 8,64] [--M 4,16,64] [--reps 7] [--limit 500] [--out DIR]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rnn_online_scan import ChildFailed, make, run_child

ROWS = [("5-7s-5", 5, 7, 5), ("64-32s-10", 64, 32, 10), ("64-64s-10", 64, 64, 10), ("64-128s-10", 64, 128, 10)]
RATES = (0.002, 0.0005)


def child(a):
    from tensor_ops_amd.hipt import HipT
    dt = np.float32
    T = HipT(0, dt)
    N = a.N
    for name, i, H, o in ROWS:
        for n in a.T:
            for M in a.M:
                rng = np.random.default_rng(11)
                layers = make(rng, i, H, o, "logistic", dt)
                x = T.put(rng.uniform(-1, 1, (N, n, i)).astype(dt), batched=True)
                y = T.put(rng.uniform(0.1, 0.9, (N, n, o)).astype(dt), batched=True)
                idx = rng.permutation(N)
                dev = lambda: [tuple(T.put(v) if isinstance(v, np.ndarray) else v for v in lay) for lay in layers]  # noqa: E731
                nets = {"caller": dev(), "route A": dev(), "route B": dev()}
                ran = {}

                def entry(key, mode):
                    HipT.rnn_minibatch_persistent(mode)
                    p0 = HipT.rnn_minibatch_stats()
                    T.rnn_stack_minibatch_sgd(nets[key], x, y, RATES[0], RATES[1], M, idx=idx)
                    ran[mode] = "B" if HipT.rnn_minibatch_stats()[0] > p0[0] else "A"

                def caller():
                    for k in range(0, N, M):
                        q = idx[k:k + M]
                        T.rnn_stack_sgd(nets["caller"], T.batch_gather(x, q), T.batch_gather(y, q), RATES[0], RATES[1])

                ways = [("caller", caller), ("route A", lambda: entry("route A", 0)), ("route B", lambda: entry("route B", 2))]
                secs = {k: [] for k, _ in ways}
                for rep in range(a.reps + 1):
                    for k, f in ways:
                        T.sync()
                        t0 = time.perf_counter(); f(); t = time.perf_counter() - t0
                        if rep > 0:
                            secs[k].append(t)
                updates = (N + M - 1) // M
                us = {k: 1e6 * float(np.median(v)) / updates for k, v in secs.items()}
                spread = max((max(v) - min(v)) / float(np.median(v)) for v in secs.values())
                best = min(us["caller"], us["route A"])
                verdict = "route A: no plan" if ran[2] != "B" else "AHEAD" if us["route B"] * (1 + spread) < best else \
                    "LOSS" if us["route B"] > best * (1 + spread) else "WITHIN"
                finite = all(np.isfinite(t.numpy()).all() for net in nets.values() for lay in net for t in lay[:4] if t is not None)
                print("ROW %11s %3d %3d | %9.2f %9.2f %9.2f | spread %5.1f %% | caller / B %6.2f  A / B %6.2f | %s%s" %
                      (name, n, M, us["caller"], us["route A"], us["route B"], 100 * spread, us["caller"] / us["route B"],
                       us["route A"] / us["route B"], verdict, "" if finite else " | NOT FINITE"), flush=True)
    HipT.rnn_minibatch_persistent(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--T", default="8,64")
    ap.add_argument("--M", default="4,16,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    a = ap.parse_args()
    a.T, a.M = [int(v) for v in str(a.T).split(",")], [int(v) for v in str(a.M).split(",")]
    if a.child:
        return child(a)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    os.makedirs(a.out, exist_ok=True)
    say("rnn minibatch scan: fp32, one to_rnn_stack_sgd update per M of N = %d sequences, softmax head, logistic states; "
        "microseconds per update (host clock around the blocking calls), median of %d" % (a.N, a.reps))
    say("%11s %3s %3s | %9s %9s %9s | %s" % ("stack", "T", "M", "caller", "route A", "route B",
                                             "run-to-run spread | ratios (above 1: route B is ahead) | verdict"))
    status = 0
    try:
        run_child([sys.executable, os.path.abspath(__file__), "--child", "--N", str(a.N), "--T", ",".join(map(str, a.T)), "--M",
                   ",".join(map(str, a.M)), "--reps", str(a.reps)], a.limit, say, {})
    except ChildFailed as e:   # what was measured is written, nothing more is started
        say("ended early, nothing further was started: %s" % e)
        status = 1
    with open(os.path.join(a.out, "rnn_minibatch_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
