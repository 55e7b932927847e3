"""BPTT of one recurrent stack through to_rnn_stack_grad on both recurrence routes, next to the same arithmetic in torch
replayed from a CUDA graph and (small shapes) the host mirror's generic BPTT.  The stack: i = 64 -> H (fullyConnected,
logistic state) -> 10 (ffLayer, softmax / crossEntropy), X [B; T, 64].  Per (H, B, T), wall time of one call in ms
(every entry blocks before it returns):
  persistent  to_set_rnn_persistent(2): one rnn_seq_kernel launch per direction for all T steps
  per_step    to_set_rnn_persistent(0): a GEMM + an elementwise launch per step and direction
  launches    kernel launches of one call on each route
  torch       forward loop + autograd of the same loss, captured once in a CUDA graph and replayed (+ synchronize)
  generic     the host mirror's rnn_netGrad in a memo scope (B <= 16, T = 16 only)
The recurrence kernel's own time per step comes from a kernel trace of one call (profiles/r07_rnn_grad_kernel_stats.csv).
usage: rnn_scan.py [--H 64,256,512] [--B 1,16,256] [--T 16,128] [--dtype f32]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tensor_ops_amd.hipt import HipT


def wall(f, reps=None):
    f()
    t0 = time.perf_counter(); f(); est = time.perf_counter() - t0
    n = reps or max(3, min(50, int(0.2 / max(est, 1e-6))))
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def torch_graph(layers, X, Y, dt):
    dev = torch.device("cuda")
    tt = lambda a: torch.tensor(np.asarray(a), dtype=dt, device=dev)  # noqa: E731
    s0, ws, w0, b0 = [tt(v).requires_grad_() for v in layers[0]]
    _, _, w1, b1 = layers[1]
    w1, b1 = tt(w1).requires_grad_(), tt(b1).requires_grad_()
    x, y = tt(X), tt(Y)
    params = [s0, ws, w0, b0, w1, b1]

    def step():
        P = x @ w0.T + b0
        s = s0.expand(x.shape[0], -1)
        outs = []
        for t in range(x.shape[1]):
            z = P[:, t] + s @ ws.T
            s = torch.sigmoid(z)
            outs.append(s)
        Hs = torch.stack(outs, 1)
        logp = torch.log_softmax(Hs @ w1.T + b1, -1)
        return torch.autograd.grad(-(y * logp).sum(), params)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(2): step()
    torch.cuda.current_stream().wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()

    def replay():
        g.replay(); torch.cuda.synchronize()
    return replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", default="64,256,512")
    ap.add_argument("--B", default="1,16,256")
    ap.add_argument("--T", default="16,128")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--no-generic", action="store_true")
    a = ap.parse_args()
    dt = np.float32 if a.dtype == "f32" else np.float64
    Tb = HipT(0, dt)
    rng = np.random.default_rng(1)
    print("dtype %s; stack 64 -> H (fullyConnected) -> 10 (softmax, crossEntropy); ms per to_rnn_stack_grad call" % a.dtype)
    print("%5s %4s %4s | %10s %9s | %10s %9s | %9s | %9s | %s" % ("H", "B", "T", "persistent", "launches", "per_step",
                                                                   "launches", "torch", "generic", "winner"))
    for H in [int(v) for v in a.H.split(",")]:
        for B in [int(v) for v in a.B.split(",")]:
            for T in [int(v) for v in a.T.split(",")]:
                layers = [tuple(np.asarray(v, dt) for v in (0.1 * rng.standard_normal(H), 0.1 * rng.standard_normal((H, H)),
                                                             0.1 * rng.standard_normal((H, 64)), 0.1 * rng.standard_normal(H))),
                          (None, None, np.asarray(0.1 * rng.standard_normal((10, H)), dt), np.asarray(0.1 * rng.standard_normal(10), dt))]
                X = rng.uniform(-1, 1, (B, T, 64)).astype(dt)
                Y = rng.dirichlet(np.ones(10), (B, T)).astype(dt)
                dl = [tuple(None if v is None else Tb.put(v) for v in lay) for lay in layers]
                x, y = Tb.put(X, batched=True), Tb.put(Y, batched=True)
                res = {}
                for mode in (2, 0):
                    HipT.rnn_persistent(mode)
                    f = lambda: Tb.rnn_stack_grad(dl, x, y)  # noqa: E731
                    res[mode] = wall(f)
                    l0 = Tb.stats()["launches"]; f(); res[mode + 10] = Tb.stats()["launches"] - l0
                HipT.rnn_persistent(1)
                tg = wall(torch_graph(layers, X, Y, torch.float32 if dt == np.float32 else torch.float64))
                gen = "-"
                if not a.no_generic and B <= 16 and T == 16:
                    from tensor_ops_amd import tops
                    tops.hlib()
                    tops.set_elem_dtype(dt)
                    net = tops.rnn_genNet([(dl[0], "actLogistic", "actLogistic")], ((dl[1][2], dl[1][3]), None), "actSoftmax")
                    xs = [Tb.put(X[:, t], batched=True) for t in range(T)]
                    ys = [Tb.put(Y[:, t], batched=True) for t in range(T)]

                    def g():
                        with Tb.memo():
                            _, gs, gp = tops.rnn_netGrad(net, "crossEntropy", xs, ys, want_inputs=False)
                            Tb.force_many(gs + gp)
                        Tb.sync()
                    gen = "%9.3f" % wall(g, reps=3)
                win = "persistent" if res[2] < res[0] else "per_step"
                print("%5d %4d %4d | %10.3f %9d | %10.3f %9d | %9.3f | %9s | %s" % (H, B, T, res[2], res[12], res[0], res[10],
                                                                                   tg, gen, win), flush=True)


if __name__ == "__main__":
    main()
