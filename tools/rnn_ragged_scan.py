"""A batch of sequences of different lengths through to_rnn_stack_grad_ragged / _sgd_ragged, next to the two things a caller
could do without them.  Per (stack, B, lengths), wall time of one call in ms (every entry blocks before it returns):
  ragged   one to_rnn_stack_grad_ragged (or _sgd_ragged) call on X [B; T, i] with lens
  padded   (a) the dense entry on the padded batch: the time of doing B T rows of work -- its gradients are NOT the ragged
           objective's, the padded steps count in them
  loop     (b) the caller's loop: one dense call per distinct length on the to_batch_gather'ed group of that length.  The
           group is gathered from a copy of the data cut to that length, [B; len, i], uploaded outside the timed region; the
           gathers are timed.  For grad the per-group gradients still have to be summed (not timed); for sgd the loop is one
           update per group, not one update on the whole batch -- it is timed for its cost only
  ideal    padded x sum lens / (B T): what (a) would cost if its time followed the rows
Stacks: 5 -> 7 (stateful) -> 5 and 64 -> 128 (stateful) -> 64, logistic states, softmax / crossEntropy.  Lengths: uniform in 1..T
(seeded), and all equal to T as a control.  Both entries alternate with their rivals inside one timed loop; the median of
the repeats is printed with the spread (min .. max) of the ragged call.
usage: rnn_ragged_scan.py [--B 64,1024] [--T 64] [--dtype f32] [--out profiles/rnn_ragged_scan.txt]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tensor_ops_amd.hipt import HipT

STACKS = [("5->7s->5", 5, 7, 5), ("64->128s->64", 64, 128, 64)]


def alternate(fs, reps):
    """median (and min, max) wall time in ms of each of fs, called in turn `reps` times after two warm-up rounds"""
    for _ in range(2):
        for f in fs:
            f()
    ts = [[] for _ in fs]
    for _ in range(reps):
        for k, f in enumerate(fs):
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="64,1024")
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dt = np.float32 if a.dtype == "f32" else np.float64
    Tb = HipT(0, dt)
    T = a.T
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("dtype %s; T = %d; automatic routing; ms per call, median of %d alternating repeats (ragged: min .. max)" % (a.dtype, T, a.reps))
    say("%-13s %5s %-8s %6s %5s | %-4s | %8s %17s | %8s %8s %8s | %7s %7s %7s" % (
        "stack", "B", "lens", "fill", "route", "call", "ragged", "(min .. max)", "padded", "loop", "ideal", "pad/rag", "loop/rag",
        "rag/idl"))
    for name, i, H, o in STACKS:
        for B in [int(v) for v in a.B.split(",")]:
            for kind in ("uniform", "equal"):
                rng = np.random.default_rng(B * 1000 + H)
                lens = rng.integers(1, T + 1, B) if kind == "uniform" else np.full(B, T)
                fill = lens.sum() / float(B * T)
                mk = lambda *s: np.asarray(0.1 * rng.standard_normal(s), dt)  # noqa: E731
                layers = [(mk(H), mk(H, H), mk(H, i), mk(H)), (None, None, mk(o, H), mk(o))]
                X = rng.uniform(-1, 1, (B, T, i)).astype(dt)
                Y = rng.dirichlet(np.ones(o), (B, T)).astype(dt)
                x, y = Tb.put(X, batched=True), Tb.put(Y, batched=True)
                groups = [(int(ln), np.nonzero(lens == ln)[0]) for ln in np.unique(lens)]
                cut = {ln: (Tb.put(np.ascontiguousarray(X[:, :ln]), batched=True),
                            Tb.put(np.ascontiguousarray(Y[:, :ln]), batched=True)) for ln, _ in groups}
                for call in ("grad", "sgd"):
                    dl = [tuple(None if v is None else Tb.put(v) for v in lay) for lay in layers]
                    rate = 0.0 if call == "sgd" else None   # rate 0: the same work every repeat, the parameters stay put
                    if call == "grad":
                        one = lambda xx, yy, **kw: Tb.rnn_stack_grad(dl, xx, yy, **kw)  # noqa: E731
                    else:
                        one = lambda xx, yy, **kw: Tb.rnn_stack_sgd(dl, xx, yy, rate, rate, **kw)  # noqa: E731

                    def loop():
                        for ln, idx in groups:
                            cx, cy = cut[ln]
                            one(Tb.batch_gather(cx, idx), Tb.batch_gather(cy, idx))
                    p0 = HipT.rnn_ragged_stats()
                    (rg, lo, hi), (pd, _, _), (lp, _, _) = alternate(
                        [lambda: one(x, y, lens=lens), lambda: one(x, y), loop], a.reps)
                    p1 = HipT.rnn_ragged_stats()
                    route = "pers" if p1[0] > p0[0] else "step"
                    ideal = pd * fill
                    say("%-13s %5d %-8s %6.3f %5s | %-4s | %8.3f (%7.3f..%7.3f) | %8.3f %8.3f %8.3f | %7.2f %7.2f %7.2f" % (
                        name, B, kind, fill, route, call, rg, lo, hi, pd, lp, ideal, pd / rg, lp / rg, rg / ideal))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
