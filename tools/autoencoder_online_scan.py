"""to_autoencoder_stack_online_sgd next to the loop a caller had to write before it: `trainEncoder` on one row at a time over
N = 256 rows in fp32, logistic layers under the (logistic, squaredError) head:
  784 -> H -> 784 for H = 16 / 32 / 64 / 128 / 256 (the plans the automatic rule's G* is read from)
  784 -> 256 -> 32 -> 256 -> 784
  32 -> 8 -> 32, a plan of ONE workgroup
Per stack, microseconds per sample, median of `--reps` (7) after one warm-up round, the three ways alternating:
  caller      to_autoencoder_stack_minibatch_sgd(minibatch = 1) over the same idx -- the yardstick: it exists without the entry
  route A     to_autoencoder_stack_online_sgd per sample (to_set_autoencoder_online_persistent 0): that loop, launch for launch
  route B     the persistent kernel (2); "(route A: ...)" where it could not run and route A did
A way is timed with device events around its blocking call (to_timer_start / to_timer_stop).  Every way trains its own copy of
the parameters, all from the same start; idx is a fixed permutation; a small rate keeps 8 x 256 updates finite.  The three
ways' parameters are compared at the end of a row (relative l2, A against the caller: bit for bit).
G* (include/tensorops_hip.h): the largest plan size G such that route B is at least as fast as route A
on every scanned TWO-LAYER row whose plan has at most that many workgroups; the tool prints it.  The automatic rule is "fp32,
two logistic layers, a plan of at most G* workgroups, no layer wider than 784, at least 256 samples": what this tool scans;
everything else takes route A.
A timed window is 256 samples -- a few milliseconds -- so a row's figure carries the scheduler's noise: ratios near 1 decide
nothing.
NOT scanned: fp64, tanh and identity layers, any i0 but 784 and 32, other n_idx.
usage: autoencoder_online_scan.py [--N 256] [--reps 7] [--out DIR]"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# (sizes, n_enc)
ROWS = [([784, H, 784], 1) for H in (16, 32, 64, 128, 256)] + [([784, 256, 32, 256, 784], 2), ([32, 8, 32], 1)]
RATE = 0.01


def box():
    """the device and its clocks as rocm-smi shows them (read only); empty where the tool is missing"""
    try:
        out = subprocess.run(["rocm-smi", "--showproductname", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        keep = [l.strip() for l in out.splitlines() if any(k in l for k in ("Card Series", "GFX Version", "sclk", "mclk", "fclk"))]
        return "; ".join(dict.fromkeys(keep))
    except Exception as e:  # noqa: BLE001
        return "rocm-smi not available (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    a = ap.parse_args()
    from tensor_ops_amd.hipt import HipT
    T, dt, N = HipT(0, np.float32), np.float32, a.N
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    say("autoencoder online scan: one trainEncoder step a row over N = %d rows, fp32, logistic layers, (logistic, squaredError); "
        "microseconds per sample (device events around the blocking call), median of %d after a warm-up round" % (N, a.reps))
    say("box: %s" % box())
    say("%26s %3s %7s | %9s %9s %9s | %s" % ("stack", "G", "LDS KiB", "caller", "route A", "route B", "ratios (above 1: route B is ahead)"))
    ahead = {}
    for sizes, n_enc in ROWS:
        rng = np.random.default_rng(17)
        ws = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(dt), (0.5 * rng.standard_normal(o)).astype(dt))
              for i, o in zip(sizes[:-1], sizes[1:])]
        x = T.put(rng.uniform(0.05, 0.95, (N, sizes[0])).astype(dt), batched=True)
        idx = rng.permutation(N)
        dev = lambda: ([T.put(w) for w, _ in ws], [T.put(b) for _, b in ws])  # noqa: E731
        nets = {"caller": dev(), "route A": dev(), "route B": dev()}
        plan = T.autoencoder_online_plan(sizes)
        ran = {}

        def entry(key, mode):
            HipT.autoencoder_online_persistent(mode)
            p0 = HipT.autoencoder_online_stats()
            T.autoencoder_online_sgd(*nets[key], n_enc, x, RATE, idx=idx)
            ran[mode] = "B" if HipT.autoencoder_online_stats()[0] > p0[0] else "A"

        ways = [("caller", lambda: T.autoencoder_minibatch_sgd(*nets["caller"], n_enc, x, RATE, 1, idx=idx)),
                ("route A", lambda: entry("route A", 0)), ("route B", lambda: entry("route B", 2))]
        ms = {k: [] for k, _ in ways}
        for rep in range(a.reps + 1):
            for k, f in ways:
                T.sync()
                T.timer_start()
                f()
                t = T.timer_stop()
                if rep > 0:
                    ms[k].append(t)
        us = {k: 1e3 * float(np.median(v)) / N for k, v in ms.items()}
        par = {k: np.concatenate([t.numpy().ravel() for t in nets[k][0] + nets[k][1]]).astype(np.float64) for k in nets}
        rel = lambda p, q: np.linalg.norm(p - q) / np.linalg.norm(q)  # noqa: E731
        note = "" if ran[2] == "B" else " (route A: %s)" % ("no plan" if not plan["exists"] else "no placement")
        nets["auto"] = dev()
        entry("auto", 1)   # (not timed: which route the automatic rule takes here)
        verdict = "" if ran[2] != "B" else "  route B %s" % ("ahead" if us["route B"] <= us["route A"] else "LOSES")
        say("%26s %3s %7s | %9.2f %9.2f %9.2f%s | caller / B %6.2f  A / B %6.2f%s | automatic: %s | A == caller: %s, B vs caller %.1e%s" %
            ("-".join(map(str, sizes)), plan["G"] if plan["exists"] else "-",
             "%.0f" % (plan["lds_bytes"] / 1024) if plan["exists"] else "-", us["caller"], us["route A"], us["route B"], note,
             us["caller"] / us["route B"], us["route A"] / us["route B"], verdict, ran[1],
             np.array_equal(par["route A"], par["caller"]), rel(par["route B"], par["caller"]),
             "" if all(np.isfinite(p).all() for p in par.values()) else " | NOT FINITE"))
        if ran[2] == "B" and len(sizes) == 3:
            ahead[plan["G"]] = ahead.get(plan["G"], True) and us["route B"] <= us["route A"]
    HipT.autoencoder_online_persistent(1)
    ok = [g for g in sorted(ahead) if all(ahead[v] for v in ahead if v <= g)]
    say("G* (two-layer rows: the largest scanned plan size up to which route B is at least as fast as route A on every row): %s"
        % (max(ok) if ok else "none"))
    say("box afterwards: %s" % box())
    say("not scanned: fp64, tanh and identity layers, i0 other than 784 and 32, n_idx other than %d" % N)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "autoencoder_online_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
