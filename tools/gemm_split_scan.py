"""The split-bf16 fp32 GEMM against today's routes and the vendor GEMM (gemm_split_kernel, csrc/gemm_split.hip;
to_set_gemm_f32_split).

For every scan row, us per product: 30 ms warm-up, 100 ms timed, REPS passes, and inside a pass the four arms ALTERNATE on the
same operands in the same process, so drift hits all alike:
  today    the switch off (mode 0): the route the product takes by default (to_gemm_route_query names its family) -- the yardstick
  split6   mode 2, six products (the pre-pass launch included: it is part of every call)
  split9   mode 2, nine products
  torch    torch.mm on the same values
and prints the median of the passes, today / split for both product counts, the run-to-run spread ((max - min) / median over the
passes, the largest of today and the two split arms) and the row-relative error of today, split6, split9 and torch against the
product in fp64 (torch, on the device).  Mode 1's table (split_scanned) is read off this file: the rows where today / split6
exceeds 1 + twice the row's spread.
   usage: gemm_split_scan.py [--out profiles/gemm_split_scan.txt] [--reps 5]
          gemm_split_scan.py --kernels M K N    (mode 2 twenty times and nothing else: the run to put under
                                                 `rocprofv3 --kernel-trace --stats`, whose per-kernel times give the pre-pass's share)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

WARM, TIMED = 30.0, 100.0
ROWS = [(s, s, s) for s in (1024, 2048, 4096, 8192)] + [(1088, 1088, 1088), (1472, 1472, 1472), (1280, 4096, 1280),
                                                        (60000, 784, 300), (60000, 300, 100)]


def timed(sync_ms):
    """us per call; sync_ms(iters, warm) -> ms for iters calls behind warm untimed ones"""
    est = max(sync_ms(5, 2) / 5, 1e-3)
    iters = max(10, int(TIMED / est))
    return 1e3 * sync_ms(iters, max(10, int(WARM / est))) / iters


def row_err(got, want):
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gemm_split_scan.txt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", type=int, nargs=3, metavar=("M", "K", "N"))
    args = ap.parse_args()
    if not args.kernels:   # (torch opens the device first: it finds none once another HIP runtime in the process has)
        import torch
        torch.cuda.init()
    from tensor_ops_amd.hipt import HipT
    T = HipT(0, dtype=np.float32)
    if args.kernels:
        m, k, n = args.kernels
        a, b = T.genRand((m, k), "uniform", -1, 1, 1), T.genRand((k, n), "uniform", -1, 1, 2)
        T.set_gemm_f32_split(2, 6)
        for _ in range(20):
            T.gmul(1, 1, 1, a, b)
        T.sync()
        T.set_gemm_f32_split(0)
        return

    def ours(a, b):
        def ms(iters, warm):
            for _ in range(warm):
                T.gmul(1, 1, 1, a, b)
            T.sync()
            T.timer_start()
            for _ in range(iters):
                T.gmul(1, 1, 1, a, b)
            return T.timer_stop()
        return ms

    def vendor(a, b, c):
        def ms(iters, warm):
            for _ in range(warm):
                torch.mm(a, b, out=c)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                torch.mm(a, b, out=c)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        return ms

    arms = ("today", "split6", "split9", "torch")
    setting = {"today": (0, -1), "split6": (2, 6), "split9": (2, 9)}
    lines = ["# tools/gemm_split_scan.py: us per product, median of %d passes (30 ms warm-up, 100 ms timed each, the four arms alternating in a"
             % args.reps, "# pass; the split arms include their pre-pass launch); TF: 2 m k n over the split6 time; spread: (max - min) / median,",
             "# the largest of today / split6 / split9; err_*: row-relative error against the fp64 product",
             "%-18s %-9s %9s %9s %9s %9s %7s %9s %9s %7s %9s %9s %9s %9s" % (
                 "shape m x k x n", "family", "today", "split6", "split9", "torch", "TF_s6", "today/s6", "today/s9", "spread",
                 "err_today", "err_s6", "err_s9", "err_torch")]
    for m, k, n in ROWS:
        rng = np.random.default_rng(m + k + n)
        ha, hb = rng.uniform(-1, 1, (m, k)).astype(np.float32), rng.uniform(-1, 1, (k, n)).astype(np.float32)
        a, b = T.put(ha), T.put(hb)
        ta, tb = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
        tc = torch.empty(m, n, device="cuda", dtype=torch.float32)
        want = torch.mm(ta.double(), tb.double()).cpu().numpy()
        T.set_gemm_f32_split(0)
        fam = "+".join(T.gemm_route(m, k, n, "f32")["families"])
        err = {}
        for arm in arms[:3]:
            T.set_gemm_f32_split(*setting[arm])
            assert arm == "today" or T.gemm_route(m, k, n, "f32")["families"] == ["split"]
            err[arm] = row_err(T.gmul(1, 1, 1, a, b).numpy(), want)
        err["torch"] = row_err(torch.mm(ta, tb).cpu().numpy(), want)
        del want
        us = {arm: [] for arm in arms}
        for _ in range(args.reps):
            for arm in arms:
                if arm == "torch":
                    us[arm].append(timed(vendor(ta, tb, tc)))
                else:
                    T.set_gemm_f32_split(*setting[arm])
                    us[arm].append(timed(ours(a, b)))
        T.set_gemm_f32_split(0)
        med = {arm: sorted(v)[len(v) // 2] for arm, v in us.items()}
        spread = max((max(us[arm]) - min(us[arm])) / med[arm] for arm in arms[:3])
        lines.append("%-18s %-9s %9.1f %9.1f %9.1f %9.1f %7.1f %9.2f %9.2f %7.3f %9.1e %9.1e %9.1e %9.1e" % (
            "%dx%dx%d" % (m, k, n), fam, med["today"], med["split6"], med["split9"], med["torch"],
            2.0 * m * k * n / med["split6"] / 1e6, med["today"] / med["split6"], med["today"] / med["split9"], spread,
            err["today"], err["split6"], err["split9"], err["torch"]))
        print(lines[-1], flush=True)
        del a, b, ta, tb, tc
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
