"""The few-right-hand-sides streaming kernel against today's routes (gemm_fewrhs_kernel, csrc/gemm_fewrhs.hip;
to_set_gemm_few_rhs).

For every scan row (shape, dtype, storage order of the operands), us per gmul through the C ABI: 30 ms warm-up, 100 ms timed,
REPS passes, and inside a pass the two configurations ALTERNATE on the same operands in the same process, so drift hits both alike:
  today    the switch off (mode 0): the route the product takes by default (to_gemm_route_query names its family) -- the yardstick
  fewrhs   mode 2, the launcher's own split rule
and prints the median of the passes, the HBM floor (bytes of A, B and C once over the 6.29 TB/s copy ceiling), the fraction of
that floor the new kernel reaches, today / fewrhs, the run-to-run spread ((max - min) / median over the passes, the larger of the
two configurations) and the largest difference between the two results relative to the largest magnitude of the result.  Mode
1's table (fewrhs_scanned) is read off this file: the rows where today / fewrhs exceeds 1 + twice the row's spread.
   usage: gemm_fewrhs_scan.py [--out profiles/gemm_fewrhs_scan.txt] [--reps 5]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

HBM = 6.29e12
WARM, TIMED = 30.0, 100.0
BOTH = [(60000, 100, 10), (60000, 784, 10), (60000, 300, 32), (1024, 60000, 32), (10, 60000, 100)]
F32_ONLY = [(60000, 10000, 8), (10000, 60000, 32), (8, 60000, 10000), (32, 10000, 60000)]
# (m, k, n, dtype, A stored transposed, B stored transposed); the last two: the other storage order of the streamed operand
ROWS = [s + (dt, 0, 0) for dt in ("f32", "f64") for s in BOTH] + [s + ("f32", 0, 0) for s in F32_ONLY] + \
       [(60000, 784, 10, "f32", 1, 0), (60000, 784, 10, "f64", 1, 0), (8, 60000, 10000, "f32", 0, 1)]


def timer(T, a, b):
    def run(iters, warm):
        for _ in range(warm):
            T.gmul(1, 1, 1, a, b)
        T.sync()
        T.timer_start()
        for _ in range(iters):
            T.gmul(1, 1, 1, a, b)
        return T.timer_stop() / iters
    est = max(run(5, 2), 1e-3)
    return 1e3 * run(max(10, int(TIMED / est)), max(10, int(WARM / est)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gemm_fewrhs_scan.txt")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from tensor_ops_amd.hipt import HipT
    Ts = {"f32": HipT(0, dtype=np.float32), "f64": HipT(0, dtype=np.float64)}
    lines = ["# tools/gemm_fewrhs_scan.py: us per gmul, median of %d passes (30 ms warm-up, 100 ms timed each, today and fewrhs alternating in"
             % args.reps, "# a pass); floor: bytes of A, B and C over 6.29 TB/s; of_floor = floor / fewrhs; spread: (max - min) / median, the row's larger;",
             "# diff: max |fewrhs - today| / max |today|.  A^T / B^T: that operand is stored transposed",
             "%-18s %-4s %-5s %-9s %9s %9s %8s %9s %9s %7s %9s" % ("shape m x k x n", "type", "store", "family", "today", "fewrhs", "floor",
                                                                   "of_floor", "today/few", "spread", "diff")]
    for m, k, n, dt, ta, tb in ROWS:
        T = Ts[dt]
        a = T.transp(T.genRand((k, m), "uniform", -1, 1, 1)) if ta else T.genRand((m, k), "uniform", -1, 1, 1)
        b = T.transp(T.genRand((n, k), "uniform", -1, 1, 2)) if tb else T.genRand((k, n), "uniform", -1, 1, 2)
        T.set_gemm_few_rhs(0)
        fam = "+".join(T.gemm_route(m, k, n, dt, a_transposed=bool(ta), b_transposed=bool(tb))["families"])
        want = T.gmul(1, 1, 1, a, b).numpy()
        T.set_gemm_few_rhs(2)
        assert T.gemm_route(m, k, n, dt, a_transposed=bool(ta), b_transposed=bool(tb))["families"] == ["fewrhs"]
        diff = float(np.max(np.abs(T.gmul(1, 1, 1, a, b).numpy() - want)) / np.max(np.abs(want)))
        us = {0: [], 2: []}
        for _ in range(args.reps):
            for mode in (0, 2):
                T.set_gemm_few_rhs(mode)
                us[mode].append(timer(T, a, b))
        T.set_gemm_few_rhs(0)
        med = {mode: sorted(v)[len(v) // 2] for mode, v in us.items()}
        spread = max((max(v) - min(v)) / med[mode] for mode, v in us.items())
        floor = 1e6 * (m * k + k * n + m * n) * (8 if dt == "f64" else 4) / HBM
        lines.append("%-18s %-4s %-5s %-9s %9.1f %9.1f %8.1f %9.3f %9.2f %7.3f %9.1e" % (
            "%dx%dx%d" % (m, k, n), dt, "A^T" if ta else "B^T" if tb else "-", fam, med[0], med[2], floor, floor / med[2],
            med[0] / med[2], spread, diff))
        print(lines[-1], flush=True)
        del a, b
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
