"""to_rnn_stack_grad of one recurrent stack on the three recurrence routes a wide layer can take, ms per call (every entry
blocks before it returns, so a host clock around a call ends in a device synchronise).  The stack: i = 64 -> H
(fullyConnected, logistic state) -> 10 (ffLayer, softmax / crossEntropy), X [B; T, 64].
  wide      to_set_rnn_wide(2): rnn_wide.hip, W' split over the G workgroups of a group, one launch per direction
  per_step  to_set_rnn_wide(0), to_set_rnn_persistent(0): a GEMM + an elementwise launch per step and direction
  seq       to_set_rnn_wide(0), to_set_rnn_persistent(2): rnn_seq_kernel forced, W' streamed from L2 by one workgroup
each next to the kernel launches of one call.  The three routes of a shape are timed in alternation: ROUNDS rounds, in each
round every route runs a window of calls (at least WINDOW_S long, 3 .. 40 calls); a route's figure is the median of its
rounds' per-call means and its spread the lowest and highest round.  The verdict is AHEAD only where the wide route's
highest round is below the lowest round of BOTH other routes, LOSS where its median is above the better of the two, and
"within spread" otherwise.  A shape without a wide plan is listed as such.  The last block runs one shape with
to_set_rnn_wide_groups raised, to show G's effect.  Every wide result is compared with the per-step route's (gW of the wide
layer, relative error) at the size that is timed.
usage: rnn_wide_scan.py [--out profiles/rnn_wide_scan.txt] [--shapes f32:256,512,1024;f64:256,512] [--B 1,16,128] [--T 16,128]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tensor_ops_amd.hipt import HipT

ROUNDS, WINDOW_S = 5, 0.05
ROUTES = (("wide", 2, 1), ("per_step", 0, 0), ("seq", 0, 2))   # (name, to_set_rnn_wide, to_set_rnn_persistent)


def window(f, n):
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rnn_wide_scan.txt")
    ap.add_argument("--shapes", default="f32:256,512,1024;f64:256,512")
    ap.add_argument("--B", default="1,16,128")
    ap.add_argument("--T", default="16,128")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("tools/rnn_wide_scan.py: ms per to_rnn_stack_grad call, stack 64 -> H (fullyConnected, logistic) -> 10 (softmax, crossEntropy)")
    say("median of %d alternating rounds [lowest .. highest round]; launches of one call; G x groups, R of the wide plan" % ROUNDS)
    say("%4s %5s %4s %4s | %-8s | %27s %4s | %27s %5s | %27s %4s | %8s | %s" % (
        "type", "H", "B", "T", "plan", "wide", "lnch", "per_step", "lnch", "seq", "lnch", "err", "verdict"))

    def measure(Tb, dt, H, B, T, routes):
        rng = np.random.default_rng(1)
        layers = [tuple(np.asarray(v, dt) for v in (0.1 * rng.standard_normal(H), 0.1 * rng.standard_normal((H, H)),
                                                     0.1 * rng.standard_normal((H, 64)), 0.1 * rng.standard_normal(H))),
                  (None, None, np.asarray(0.1 * rng.standard_normal((10, H)), dt), np.asarray(0.1 * rng.standard_normal(10), dt))]
        X = rng.uniform(-1, 1, (B, T, 64)).astype(dt)
        Y = rng.dirichlet(np.ones(10), (B, T)).astype(dt)
        dl = [tuple(None if v is None else Tb.put(v) for v in lay) for lay in layers]
        x, y = Tb.put(X, batched=True), Tb.put(Y, batched=True)
        f = lambda: Tb.rnn_stack_grad(dl, x, y)   # noqa: E731
        reps, launches, gw, rounds = {}, {}, {}, {name: [] for name, _, _ in routes}

        def select(wide, pers):
            HipT.rnn_wide(wide)
            HipT.rnn_persistent(pers)
        for name, wide, pers in routes:   # warm-up, the launch count, the result, the window's length
            select(wide, pers)
            f()
            l0 = Tb.stats()["launches"]
            gw[name] = f()[2][0].numpy().astype(np.float64)
            launches[name] = Tb.stats()["launches"] - l0
            reps[name] = max(3, min(40, int(WINDOW_S / max(window(f, 2) * 1e-3, 1e-6))))
        for _ in range(ROUNDS):
            for name, wide, pers in routes:
                select(wide, pers)
                rounds[name].append(window(f, reps[name]))
        HipT.rnn_wide(0)
        HipT.rnn_persistent(1)
        return rounds, launches, gw

    def cell(r):
        return "%8.3f [%7.3f .. %7.3f]" % (float(np.median(r)), min(r), max(r))

    for spec in a.shapes.split(";"):
        tname, hs = spec.split(":")
        dt = np.float32 if tname == "f32" else np.float64
        Tb = HipT(0, dt)
        for H in [int(v) for v in hs.split(",")]:
            for B in [int(v) for v in a.B.split(",")]:
                for T in [int(v) for v in a.T.split(",")]:
                    HipT.rnn_wide_groups(0)
                    p = HipT.rnn_wide_plan(H, B, tname)
                    routes = ROUTES if p["exists"] else ROUTES[1:]
                    rounds, launches, gw = measure(Tb, dt, H, B, T, routes)
                    ps, sq = rounds["per_step"], rounds["seq"]
                    if not p["exists"]:
                        say("%4s %5d %4d %4d | %-8s | %27s %4s | %s %5d | %s %4d | %8s | %s" % (
                            tname, H, B, T, "no plan", "-", "-", cell(ps), launches["per_step"], cell(sq), launches["seq"], "-",
                            "no wide plan: today's routes"))
                        continue
                    w = rounds["wide"]
                    err = np.linalg.norm(gw["wide"] - gw["per_step"]) / np.linalg.norm(gw["per_step"])
                    verdict = "wide AHEAD" if max(w) < min(min(ps), min(sq)) else \
                        "wide: LOSS" if np.median(w) > min(np.median(ps), np.median(sq)) else "within spread"
                    say("%4s %5d %4d %4d | %2dx%d R%-2d | %s %4d | %s %5d | %s %4d | %8.1e | %s" % (
                        tname, H, B, T, p["G"], p["groups"], p["R"], cell(w), launches["wide"], cell(ps), launches["per_step"],
                        cell(sq), launches["seq"], err, verdict))
    say("")
    say("G's effect: f32, H = 256, B = 1, T = 128, to_set_rnn_wide_groups raised (ms per call, wide route alone)")
    Tb = HipT(0, np.float32)
    for mg in (0, 4, 8, 16, 32):
        HipT.rnn_wide_groups(mg)
        p = HipT.rnn_wide_plan(256, 1, "f32")
        rounds, launches, _ = measure(Tb, np.float32, 256, 1, 128, ROUTES[:1])
        say("min_groups %2d: G = %2d, C = %3d | %s" % (mg, p["G"], p["C"], cell(rounds["wide"])))
    HipT.rnn_wide_groups(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
