"""Batched inference of ffLayer stacks through to_fflayer_stack_infer next to the same arithmetic in torch replayed from a
CUDA graph (addmm + sigmoid per hidden layer, addmm + softmax / sigmoid, argmax).  Per stack, batch and element type:
  stack     device time of the whole call with `out` only (no host result: nothing waits), its kernel launches
  head      the last layer + head alone (a one-layer call on a [B, K_L] activation): time, bytes moved (A once, W_L,
            out), frac_hbm = bytes / time / 6.3 TB/s (streaming-read peak measured on this part)
  classes   wall time of a call that returns classes only (includes the B x 4-byte download)
  torch     the captured torch graph, replayed
usage: infer_scan.py [--batches 1000,10000,60000,1000000] [--dtypes f32,f64]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tensor_ops_amd.hipt import HipT

HBM = 6.3e12
STACKS = [[784, 300, 100, 10], [784, 256, 10], [784, 10], [100, 10], [2, 12, 8, 1], [256, 1000]]


def time_ours(T, f):
    for _ in range(3): f()
    T.sync(); T.timer_start()
    for _ in range(3): f()
    est = max(T.timer_stop() / 3, 1e-3)
    n = max(10, int(20.0 / est))
    T.sync(); T.timer_start()
    for _ in range(n): f()
    return T.timer_stop() / n


def time_wall(f):
    for _ in range(3): f()
    t0 = time.perf_counter(); f(); est = time.perf_counter() - t0
    n = max(5, int(0.02 / max(est, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(n): f()
    return (time.perf_counter() - t0) / n * 1e3


def time_torch(f):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3): f()
    e1.record(); torch.cuda.synchronize()
    est = max(e0.elapsed_time(e1) / 3, 1e-3)
    n = max(10, int(20.0 / est))
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1000,10000,60000,1000000")
    ap.add_argument("--dtypes", default="f32,f64")
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    for dname in a.dtypes.split(","):
        dt = np.float32 if dname == "f32" else np.float64
        tdt = torch.float32 if dname == "f32" else torch.float64
        es = np.dtype(dt).itemsize
        T = HipT(0, dt)
        for sizes in STACKS:
            rng = np.random.default_rng(sum(sizes))
            ws = [((0.1 * rng.standard_normal((o, i))).astype(dt), (0.1 * rng.standard_normal(o)).astype(dt))
                  for i, o in zip(sizes[:-1], sizes[1:])]
            W, b = [T.put(w) for w, _ in ws], [T.put(v) for _, v in ws]
            tw = [(torch.tensor(w, device="cuda"), torch.tensor(v, device="cuda")) for w, v in ws]
            head = "logistic" if sizes[-1] == 1 else "softmax"
            K, n = sizes[-2], sizes[-1]
            for B in batches:
                if B * sum(sizes) * es * 4 > 40e9:
                    print("%-16s %s B=%-8d skipped (memory)" % ("-".join(map(str, sizes)), dname, B), flush=True)
                    continue
                x = T.genRand((sizes[0],), "uniform", 0, 1, 1, batch=B)
                hin = T.genRand((K,), "uniform", 0, 1, 2, batch=B)
                l0 = T.stats()["launches"]
                T.infer_stack(W, b, x, out_act=head, want_out=True, want_classes=False)
                nl = T.stats()["launches"] - l0
                t_stack = time_ours(T, lambda: T.infer_stack(W, b, x, out_act=head, want_out=True, want_classes=False))
                t_head = time_ours(T, lambda: T.infer_stack(W[-1:], b[-1:], hin, out_act=head, want_out=True,
                                                            want_classes=False))
                t_cls = time_wall(lambda: T.infer_stack(W, b, x, out_act=head, want_classes=True))
                hbytes = (B * K + n * K + B * n) * es
                tx = torch.rand(B, sizes[0], device="cuda", dtype=tdt)

                def fwd():
                    h = tx
                    for w, v in tw[:-1]:
                        h = torch.sigmoid(torch.addmm(v, h, w.t()))
                    z = torch.addmm(tw[-1][1], h, tw[-1][0].t())
                    p = torch.softmax(z, dim=1) if head == "softmax" else torch.sigmoid(z)
                    return p, p.argmax(dim=1)
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    fwd()
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fwd()
                t_torch = time_torch(g.replay)
                print("%-16s %s B=%-8d stack %9.1f us (%d launches) %8.2f Gsamples/s | head %8.1f us %9.1f MB "
                      "frac_hbm %.2f | classes %9.1f us wall | torch graph %9.1f us  torch/ours %.2f"
                      % ("-".join(map(str, sizes)), dname, B, t_stack * 1e3, nl, B / (t_stack * 1e-3) / 1e9,
                         t_head * 1e3, hbytes / 1e6, hbytes / (t_head * 1e-3) / HBM, t_cls * 1e3, t_torch * 1e3,
                         t_torch / t_stack), flush=True)
                del g, tx, x, hin
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
