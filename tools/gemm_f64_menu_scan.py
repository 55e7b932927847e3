"""The fp64 tile menu against today's routes (gemm_kw64_menu_kernel, csrc/gemm_kwave_f64.hip; to_set_gemm_f64_menu).

For every scan shape, us per gmul through the C ABI (15 ms warm-up, 20 ms timed, REPS passes; the configurations alternate
inside a pass, so drift hits all of them alike):
  parent   the parent commit's library (--parent-lib: its libtensorops_hip.so, built from a checkout of the parent and loaded
           by a child process that runs this file with --child), one child per pass
  mode0    this build with the switch off: the same family as the parent (to_gemm_route_query) and the same time within the spread
  t0..t4   mode 2 with that menu entry forced: 48x48 / 48x64 / 64x48 / 32x64 / 64x32
  vendor   torch.mm in float64, a yardstick only
and prints the median of the passes, TF, the fraction of the 78.6 TF fp64 MFMA peak and the run-to-run spread (max - min over
the median, the largest over the row's configurations).  The rule of mode 1 (kw64m_auto) is fitted from this table.
   usage: gemm_f64_menu_scan.py [--parent-lib PATH] [--out profiles/gemm_f64_menu_scan.txt] [--reps 3]"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PEAK = 78.6
# tools/gemm_scan.py's windows.  20 ms is short: it also measures the clock and the scheduler, and the parent runs in a child of
# its own ahead of each pass, not alternated shape by shape with this build.  Good enough to fit a switch that is off by default
# -- kw64m_auto's 7 % margin is twice the largest spread seen here for that reason -- and not a figure to quote to three digits.
WARM, TIMED = 15.0, 20.0
TILES = ("48x48", "48x64", "64x48", "32x64", "64x32")
# fp64.gmul_mid_sizes and the fp32 mid sizes of bench.py (the three few-tiles-long-K shapes included), 896^3 / 1152^3 between
# them, and the reference's Learn shapes (gmul_learn_shapes)
SHAPES = [(640, 640, 640), (768, 768, 768), (896, 896, 896), (1000, 1000, 1000), (1024, 1024, 1024), (1088, 1088, 1088),
          (1152, 1152, 1152), (1280, 1280, 1280), (1536, 1536, 1536), (2048, 2048, 2048), (3072, 3072, 3072), (768, 1024, 1024),
          (4096, 784, 256), (1024, 1024, 512), (512, 2048, 512), (384, 4096, 384), (1152, 2048, 1152),
          (60000, 784, 300), (60000, 300, 100), (8192, 300, 100), (8192, 100, 300), (100, 8192, 300), (100, 60000, 300)]


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


def one_pass(T, configs):
    """{shape: {config: us}}; configs: [(name, mode, tile)] (the parent's library knows no switch: mode None)"""
    out = {}
    for m, k, n in SHAPES:
        a = T.genRand((m, k), "uniform", -1, 1, 1)
        b = T.genRand((k, n), "uniform", -1, 1, 2)
        if configs[0][1] is not None:
            T.set_gemm_f64_menu(0)
        row = {"family": "+".join(T.gemm_route(m, k, n, "f64")["families"])}   # today's route
        for name, mode, tile in configs:
            if mode is not None:
                T.set_gemm_f64_menu(mode, tile)
            row[name] = timer(T, a, b)
        out["%dx%dx%d" % (m, k, n)] = row
        del a, b
    return out


def child():
    from tensor_ops_amd import capi
    capi.SIGNATURES.pop("to_set_gemm_f64_menu")   # the parent's library has no switch to bind
    from tensor_ops_amd.hipt import HipT
    print(json.dumps(one_pass(HipT(0, dtype=np.float64), [("parent", None, -1)])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default="profiles/gemm_f64_menu_scan.txt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    import torch
    from tensor_ops_amd.hipt import HipT
    T = HipT(0, dtype=np.float64)
    configs = [("mode0", 0, -1)] + [("t%d" % i, 2, i) for i in range(len(TILES))]
    passes, parents, vendor = [], [], {}
    for _ in range(args.reps):
        if args.parent_lib:
            env = dict(os.environ, TOPS_HIP_LIB=os.path.abspath(args.parent_lib), LD_LIBRARY_PATH=os.path.dirname(os.path.abspath(args.parent_lib)))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            parents.append(json.loads(r.stdout.strip().splitlines()[-1]))
        passes.append(one_pass(T, configs))
        T.set_gemm_f64_menu(0)
    for m, k, n in SHAPES:
        a = torch.rand(m, k, device="cuda", dtype=torch.float64) * 2 - 1
        b = torch.rand(k, n, device="cuda", dtype=torch.float64) * 2 - 1
        c = torch.empty(m, n, device="cuda", dtype=torch.float64)

        def run(iters, warm):
            for _ in range(warm):
                torch.mm(a, b, out=c)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                torch.mm(a, b, out=c)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters
        est = max(run(5, 2), 1e-3)
        vendor["%dx%dx%d" % (m, k, n)] = 1e3 * run(max(10, int(TIMED / est)), max(10, int(WARM / est)))
    lines = ["# tools/gemm_f64_menu_scan.py: us per fp64 gmul, median of %d passes (15 ms warm-up, 20 ms timed each); TF and the fraction of the"
             % args.reps, "# %.1f TF fp64 MFMA peak for the best menu tile; spread: (max - min) / median over the passes, the row's largest" % PEAK,
             "%-18s %-9s %9s %9s " % ("shape m x k x n", "family", "parent", "mode0") + " ".join("%9s" % t for t in TILES)
             + " %9s %7s %6s %6s %7s" % ("vendor", "best", "TF", "peak", "spread")]
    for m, k, n in SHAPES:
        key = "%dx%dx%d" % (m, k, n)
        cols, spread = {}, 0.0
        for name in ["parent"] + [c[0] for c in configs]:
            src = parents if name == "parent" else passes
            v = sorted(p[key][name] for p in src)
            if not v:
                cols[name] = float("nan")
                continue
            cols[name] = v[len(v) // 2]
            spread = max(spread, (v[-1] - v[0]) / cols[name])
        fam = passes[0][key]["family"]
        if parents:
            assert parents[0][key]["family"] == fam, (key, parents[0][key]["family"], fam)
        best = min(range(len(TILES)), key=lambda i: cols["t%d" % i])
        tf = 2.0 * m * k * n / cols["t%d" % best] / 1e6
        lines.append("%-18s %-9s %9.1f %9.1f " % (key, fam, cols["parent"], cols["mode0"]) + " ".join("%9.1f" % cols["t%d" % i] for i in range(len(TILES)))
                     + " %9.1f %7s %6.1f %6.3f %7.3f" % (vendor[key], TILES[best], tf, tf / PEAK, spread))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
