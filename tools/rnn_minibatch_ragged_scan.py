"""to_rnn_stack_minibatch_sgd_ragged next to the loop a caller had to write before it: fp32, N = 256 sequences padded to T,
lengths uniform in 1 .. T, M sequences an update, softmax head over a stateless output layer, logistic states and hidden layers:
  5 -> 7 (stateful) -> 5 and 64 -> H (stateful) -> 10 for H = 32 / 64;  T in {8, 64};  M in {4, 16, 64}
Per (stack, T, M), microseconds per UPDATE, median of `--reps` (7) after one warm-up round, the ways alternating:
  caller      a loop of to_batch_gather (X and Y) + to_rnn_stack_sgd_ragged with the lengths gathered on the host -- the
              yardstick: what the same training cost before the entry existed (unchanged entries, same process)
  route A     to_rnn_stack_minibatch_sgd_ragged per minibatch (to_set_rnn_minibatch_persistent 0)
  route B     to_rnn_stack_minibatch_sgd_ragged persistent on packed rows (2); "(route A: no plan)" where route A ran
  dense       to_rnn_stack_minibatch_sgd under its automatic rule on the PADDED set: ANOTHER OBJECTIVE (it trains on the
              padding), a work reference only, in no verdict
A way is timed with the host clock around the blocking call(s).  Every way trains its own copy of the parameters, all from
the same start, on the same permutation of the sequences; small rates keep the updates finite.  spread: the largest
(max - min) / median of a way's repetitions in the row (dense not counted).  Verdict: AHEAD where route B's median is below
both others' by more than that spread -- the rows an automatic rule may name --, else LOSS (or WITHIN the spread).  rows: the
rows route B packs against the T Mp of the dense kernel.  The scan runs in a child process under a time limit (`--limit`
seconds; at the limit the child's process group is killed); a child that fails ends the tool with status 1 after it has
written what it measured.
usage: rnn_minibatch_ragged_scan.py [--N 256] [--T 8,64] [--M 4,16,64] [--reps 7] [--limit 500] [--out DIR]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rnn_online_scan import ChildFailed, make, run_child

ROWS = [("5-7s-5", 5, 7, 5), ("64-32s-10", 64, 32, 10), ("64-64s-10", 64, 64, 10)]
RATES = (0.002, 0.0005)


def packed_rows(lens, idx, M):
    """(rows route B packs, rows of the dense kernel's layout) over the call"""
    up16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    packed = 0
    for k in range(0, len(idx), M):
        ll = lens[idx[k:k + M]]
        packed += sum(up16(int((ll > t).sum())) for t in range(int(ll.max())))
    return packed


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
                lens = rng.integers(1, n + 1, N)
                dev = lambda: [tuple(T.put(v) if isinstance(v, np.ndarray) else v for v in lay) for lay in layers]  # noqa: E731
                nets = {"caller": dev(), "route A": dev(), "route B": dev(), "dense": dev()}
                ran = {}

                def entry(key, mode):
                    HipT.rnn_minibatch_persistent(mode)
                    p0 = HipT.rnn_minibatch_ragged_stats()
                    T.rnn_stack_minibatch_sgd_ragged(nets[key], x, y, lens, RATES[0], RATES[1], M, idx=idx)
                    ran[mode] = "B" if HipT.rnn_minibatch_ragged_stats()[0] > p0[0] else "A"

                def caller():
                    for k in range(0, N, M):
                        q = idx[k:k + M]
                        T.rnn_stack_sgd(nets["caller"], T.batch_gather(x, q), T.batch_gather(y, q), RATES[0], RATES[1],
                                        lens=lens[q])

                def dense():
                    HipT.rnn_minibatch_persistent(1)
                    T.rnn_stack_minibatch_sgd(nets["dense"], x, y, RATES[0], RATES[1], M, idx=idx)

                ways = [("caller", caller), ("route A", lambda: entry("route A", 0)), ("route B", lambda: entry("route B", 2)),
                        ("dense", dense)]
                secs = {k: [] for k, _ in ways}
                for rep in range(a.reps + 1):
                    for k, f in ways:
                        T.sync()
                        t0 = time.perf_counter(); f(); t = time.perf_counter() - t0
                        if rep > 0:
                            secs[k].append(t)
                updates = (N + M - 1) // M
                us = {k: 1e6 * float(np.median(v)) / updates for k, v in secs.items()}
                spread = max((max(v) - min(v)) / float(np.median(v)) for k, v in secs.items() if k != "dense")
                best = min(us["caller"], us["route A"])
                verdict = "route A: no plan" if ran[2] != "B" else "AHEAD" if us["route B"] * (1 + spread) < best else \
                    "LOSS" if us["route B"] > best * (1 + spread) else "WITHIN"
                finite = all(np.isfinite(t.numpy()).all() for net in nets.values() for lay in net for t in lay[:4] if t is not None)
                print("ROW %11s %3d %3d | %9.2f %9.2f %9.2f | spread %5.1f %% | caller / B %6.2f  A / B %6.2f | %-6s | dense "
                      "(another objective) %9.2f | rows %6d of %6d%s" %
                      (name, n, M, us["caller"], us["route A"], us["route B"], 100 * spread, us["caller"] / us["route B"],
                       us["route A"] / us["route B"], verdict, us["dense"], packed_rows(lens, idx, M),
                       updates * n * ((M + 15) // 16 * 16), "" if finite else " | NOT FINITE"), flush=True)
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
    say("rnn minibatch ragged scan: fp32, one to_rnn_stack_sgd_ragged update per M of N = %d sequences padded to T, lengths uniform "
        "in 1 .. T, softmax head, logistic states; microseconds per update (host clock around the blocking calls), median of %d"
        % (a.N, a.reps))
    say("%15s %3s %3s | %9s %9s %9s | %s" % ("stack", "T", "M", "caller", "route A", "route B",
                                             "run-to-run spread | ratios (above 1: route B is ahead) | verdict | dense entry on "
                                             "the padded set | packed rows of the dense layout's"))
    status = 0
    try:
        run_child([sys.executable, os.path.abspath(__file__), "--child", "--N", str(a.N), "--T", ",".join(map(str, a.T)), "--M",
                   ",".join(map(str, a.M)), "--reps", str(a.reps)], a.limit, say, {})
    except ChildFailed as e:   # what was measured is written, nothing more is started
        say("ended early, nothing further was started: %s" % e)
        status = 1
    with open(os.path.join(a.out, "rnn_minibatch_ragged_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
