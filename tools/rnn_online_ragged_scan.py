"""to_rnn_stack_online_sgd_ragged next to what a caller had before it: fp32, N = 256 sequences padded to T = 64, lengths
seeded uniform in 1 .. T, one trainNetwork' step a sequence on its own steps, softmax head over a stateless output layer,
logistic states and hidden layers:
  5 -> 7 (stateful) -> 5   and   64 -> H (stateful) -> 10 for H = 32 / 64 / 96 / 128
Per stack, microseconds per sequence, median of `--reps` (7) after one warm-up round, the ways alternating:
  ragged B    the ragged call on the persistent route (to_set_rnn_online_persistent 2)
  ragged A    the ragged call per sequence (0)
  caller      a host loop of to_rnn_stack_sgd over to_wrap views of each sequence's leading rows (the views made once, outside
              the clock) -- the only thing a caller could write before the entry existed
  padded      the dense to_rnn_stack_online_sgd (persistent) on the padded set: N T rows of work on a DIFFERENT objective -- it
              trains on the padding --, a work reference only.  A sequence's cost follows its own length on route B, so
              padded / ragged B should tend towards N T / sum lens; the tool prints both and asserts nothing
  full B      the ragged call with every length T, next to
  dense B     the dense entry on the same set: the difference is the ragged entry's own overhead, the lengths table and the
              per-sequence length read
A way is timed with the host clock around the blocking call(s).  Every way trains its own copy of the parameters, all from
the same start; small rates keep the updates finite.
The automatic rule of the entry (H* = 128, include/tensorops_hip.h) was read from equal lengths; the tool says for which
scanned rows inside the automatic range route B is at least as fast as route A on these lengths too.
The scan runs in a child process under a time limit (`--limit` seconds; at the limit the child's process group is killed).
A child that fails or does not finish ends the tool with status 1 after it has written what it measured: nothing is started
on a device behind a failure.
usage: rnn_online_ragged_scan.py [--N 256] [--T 64] [--reps 7] [--seed 11] [--limit 300] [--out DIR]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rnn_online_scan import RATES, ChildFailed, make, run_child

# (name, i, H, n_L)
ROWS = [("5-7s-5", 5, 7, 5), ("64-32s-10", 64, 32, 10), ("64-64s-10", 64, 64, 10), ("64-96s-10", 64, 96, 10),
        ("64-128s-10", 64, 128, 10)]
WAYS = ("ragged B", "ragged A", "caller", "padded", "full B", "dense B")


def child(a):
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import DT, HipT
    dt = np.float32
    T = HipT(0, dt)
    N, n = a.N, a.T
    lens = np.random.default_rng(a.seed).integers(1, n + 1, N)
    full = np.full(N, n)
    print("ROW sum lens = %d of N T = %d rows: N T / sum lens = %.2f" % (lens.sum(), N * n, N * n / lens.sum()), flush=True)

    def rows_of(t, q, rows):   # the leading rows of sequence q at t's own address
        (n_t, w) = t.shape
        dims, rank = capi.dims_arr((rows, w))
        h = capi.c_tensor()
        capi.check(capi.lib().to_wrap(C.c_void_p(t.ptr + q * n_t * w * 4), T.to_dtype, rank, dims, 0, C.byref(h)))
        return DT(h)

    for name, i, H, o in ROWS:
        rng = np.random.default_rng(11)
        layers = make(rng, i, H, o, "logistic", dt)
        x = T.put(rng.uniform(-1, 1, (N, n, i)).astype(dt), batched=True)
        y = T.put(rng.uniform(0.1, 0.9, (N, n, o)).astype(dt), batched=True)
        xs, ys = [rows_of(x, q, int(lens[q])) for q in range(N)], [rows_of(y, q, int(lens[q])) for q in range(N)]
        dev = lambda: [tuple(T.put(v) if isinstance(v, np.ndarray) else v for v in lay) for lay in layers]  # noqa: E731
        nets = {k: dev() for k in WAYS}
        ran = {}

        def ragged(key, mode, ll):
            HipT.rnn_online_persistent(mode)
            p0 = HipT.rnn_online_ragged_stats()
            T.rnn_stack_online_sgd_ragged(nets[key], x, y, ll, RATES[0], RATES[1])
            ran[key] = "B" if HipT.rnn_online_ragged_stats()[0] > p0[0] else "A"

        def dense(key):
            HipT.rnn_online_persistent(2)
            p0 = HipT.rnn_online_stats()
            T.rnn_stack_online_sgd(nets[key], x, y, RATES[0], RATES[1])
            ran[key] = "B" if HipT.rnn_online_stats()[0] > p0[0] else "A"

        def caller():
            for q in range(N):
                T.rnn_stack_sgd(nets["caller"], xs[q], ys[q], RATES[0], RATES[1])

        ways = [("ragged B", lambda: ragged("ragged B", 2, lens)), ("ragged A", lambda: ragged("ragged A", 0, lens)),
                ("caller", caller), ("padded", lambda: dense("padded")), ("full B", lambda: ragged("full B", 2, full)),
                ("dense B", lambda: dense("dense B"))]
        secs = {k: [] for k, _ in ways}
        for rep in range(a.reps + 1):
            for k, f in ways:
                T.sync()
                t0 = time.perf_counter(); f(); t = time.perf_counter() - t0
                if rep > 0:
                    secs[k].append(t)
        us = {k: 1e6 * float(np.median(v)) / N for k, v in secs.items()}
        nets["auto"] = dev()
        ragged("auto", 1, lens)   # (not timed: which route the automatic rule takes here)
        routes_ok = ran["ragged B"] == "B" and ran["ragged A"] == "A" and ran["padded"] == "B" and ran["full B"] == "B" and \
            ran["dense B"] == "B"
        finite = all(np.isfinite(t.numpy()).all() for k in WAYS for lay in nets[k] for t in lay[:4] if t is not None)
        print("ROW %11s | %8.2f %8.2f %8.2f %8.2f | A / B %5.2f  caller / B %5.2f  padded / B %5.2f | %8.2f %8.2f  full / dense "
              "%5.3f | automatic: %s%s%s" %
              (name, us["ragged B"], us["ragged A"], us["caller"], us["padded"], us["ragged A"] / us["ragged B"],
               us["caller"] / us["ragged B"], us["padded"] / us["ragged B"], us["full B"], us["dense B"],
               us["full B"] / us["dense B"], ran["auto"], "" if routes_ok else " | A WAY TOOK ANOTHER ROUTE: %s" % ran,
               "" if finite else " | NOT FINITE"), flush=True)
        print("HSTAR %d %d %d" % (H, n, int(us["ragged B"] <= us["ragged A"])), flush=True)
    HipT.rnn_online_persistent(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    os.makedirs(a.out, exist_ok=True)
    say("rnn online ragged scan: fp32, one trainNetwork' step a sequence over N = %d sequences padded to T = %d, lengths uniform in "
        "1 .. T (seed %d), softmax head; microseconds per sequence (host clock around the blocking calls), median of %d" %
        (a.N, a.T, a.seed, a.reps))
    say("%11s | %8s %8s %8s %8s | %s | %8s %8s  %s" %
        ("stack", "ragged B", "ragged A", "caller", "padded", "ratios (above 1: ragged B is ahead)", "full B", "dense B",
         "every length T: the entry's own overhead"))
    status, ahead = 0, {}
    try:
        run_child([sys.executable, os.path.abspath(__file__), "--child", "--N", str(a.N), "--T", str(a.T), "--reps", str(a.reps),
                   "--seed", str(a.seed)], a.limit, say, ahead)
        behind = [H for H in sorted(ahead) if not all(ahead[H].values())]
        say("route B against route A on these lengths, H <= 128 (the automatic range): %s" %
            ("behind at H = %s" % behind if behind else "ahead on every scanned row: the automatic rule H* = 128 is confirmed for "
             "these rows"))
        say("not measured: fp64, tanh states, other length distributions, other T")
    except ChildFailed as e:   # what was measured is written, nothing more is started
        say("ended early, nothing further was started: %s" % e)
        status = 1
    with open(os.path.join(a.out, "rnn_online_ragged_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
