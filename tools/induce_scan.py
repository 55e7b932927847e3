"""`induceNetwork` iterated through to_fflayer_stack_induce on both routes.  Per (dtype, stack, B, iters): wall time of one
blocking call in ms (median of repeats) and per iteration in us,
  A         to_set_induce_persistent(0): per iteration -- a GEMM a layer each way, the loss head, the step in an epilogue
  B         to_set_induce_persistent(2): the persistent kernel (csrc/induce_seq.hip), `-` where its plan does not fit
            (or the call ran per iteration: read from to_induce_stats)
  launches  kernel launches of one call on each route (to_stats)
  auto      the route to_set_induce_persistent(1) takes
  mirror    B = 1 only: `induceNum` as the host mirror runs it (host/tensorops/trainer.hpp) -- one step of netGrad with the
            input's cotangent through libtensorops_host.so, the update and the copy back, recorded in a fusion scope,
            captured as a graph and replayed iters - 1 times -- restated here on the same entry points, us per iteration.
            This is the path the tree had before to_fflayer_stack_induce; this tool does not change it.
usage: induce_scan.py [--dtype f32,f64] [--B 1,10,256,4096] [--iters 100,5000] [--stacks 784-300-100-10,784-32-10,2-12-8-1]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tensor_ops_amd.hipt import HipT


def wall(f):
    f()
    t0 = time.perf_counter(); f(); est = time.perf_counter() - t0
    n = max(3, min(30, int(0.3 / max(est, 1e-6))))
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def mirror_induce(T, ws, x0, y0, dt, iters):
    from tensor_ops_amd import capi, tops
    from tensor_ops_amd.hipt import Graph
    tops.hlib()
    tops.set_elem_dtype(dt)
    head = "actSoftmax" if ws[-1][0].shape[0] > 1 else "actLogistic"
    loss = "crossEntropy" if ws[-1][0].shape[0] > 1 else "squaredError"
    net = tops.genNet([(T.put(w), T.put(b)) for w, b in ws], "actLogistic", head)
    y = T.put(y0)
    xbuf = T.put(x0)

    def step():
        with T.memo():
            g = tops.netGrad(net, loss, xbuf, y)[0]
            x1 = T.liftT(lambda v: v[0] - 1.0 * v[1], [xbuf, g])
            capi.check(capi.lib().to_copy_into(xbuf.h, x1.h))
    step()
    T.sync()
    with Graph() as g:
        step()

    def run():
        for _ in range(iters - 1):
            g.launch()
        T.sync()
    return wall(run) * 1e3 / (iters - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32,f64")
    ap.add_argument("--B", default="1,10,256,4096")
    ap.add_argument("--iters", default="100,5000")
    ap.add_argument("--stacks", default="784-300-100-10,784-32-10,2-12-8-1")
    ap.add_argument("--no-mirror", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    print("to_fflayer_stack_induce, rate 1, one blocking call; ms per call | us per iteration | launches per call")
    print("%5s %16s %5s %5s | %10s %10s | %8s %8s | %6s %4s | %6s %4s | %8s" %
          ("dtype", "stack", "B", "iters", "A ms", "B ms", "A us/it", "B us/it", "A ln", "B ln", "winner", "auto", "mirror"))
    for dname in a.dtype.split(","):
        dt = np.float32 if dname == "f32" else np.float64
        T = HipT(0, dt)
        for stack in a.stacks.split(","):
            sizes = [int(v) for v in stack.split("-")]
            ws = [((0.1 * rng.standard_normal((o, i))).astype(dt), (0.1 * rng.standard_normal(o)).astype(dt))
                  for i, o in zip(sizes[:-1], sizes[1:])]
            W, b = [T.put(w) for w, _ in ws], [T.put(bb) for _, bb in ws]
            head = ("softmax", "crossEntropy") if sizes[-1] > 1 else ("logistic", "squaredError")
            for B in [int(v) for v in a.B.split(",")]:
                X = rng.uniform(0, 0.05, (B, sizes[0])).astype(dt)
                Y = np.zeros((B, sizes[-1]), dt)
                Y[np.arange(B), rng.integers(0, sizes[-1], B)] = 1
                x, y = T.put(X, batched=True), T.put(Y, batched=True)
                for iters in [int(v) for v in a.iters.split(",")]:
                    if iters > 1000 and B > 10:
                        continue
                    f = lambda: T.induce_stack(W, b, x, y, 1.0, iters, out_act=head[0], loss=head[1])  # noqa: E731
                    ms, ln, took = {}, {}, {}
                    for mode in (0, 2, 1):
                        HipT.induce_persistent(mode)
                        p0, _ = HipT.induce_stats()
                        l0 = T.stats()["launches"]; f(); ln[mode] = T.stats()["launches"] - l0
                        took[mode] = "B" if HipT.induce_stats()[0] > p0 else "A"
                        if mode != 1 and not (mode == 2 and took[2] == "A"):
                            ms[mode] = wall(f)
                    HipT.induce_persistent(1)
                    bms = "%10.3f" % ms[2] if 2 in ms else "%10s" % "-"
                    bus = "%8.2f" % (ms[2] * 1e3 / iters) if 2 in ms else "%8s" % "-"
                    bln = "%4d" % ln[2] if 2 in ms else "%4s" % "-"
                    win = "A" if 2 not in ms or ms[0] <= ms[2] else "B"
                    mir = "-"
                    if B == 1 and iters == 100 and not a.no_mirror:
                        try:
                            mir = "%8.2f" % mirror_induce(T, ws, X[0], Y[0], dt, iters)
                        except Exception as e:   # the column is information: say why it is missing and go on
                            mir = "failed: %s" % str(e)[:60]
                    print("%5s %16s %5d %5d | %10.3f %s | %8.2f %s | %6d %s | %6s %4s | %8s" %
                          (dname, stack, B, iters, ms[0], bms, ms[0] * 1e3 / iters, bus, ln[0], bln, win, took[1], mir), flush=True)


if __name__ == "__main__":
    main()
