"""to_autoencoder_stack_* next to the way a caller got by before them, in fp32 on 784-256-784 and 784-256-64-256-784 at
1,024 and 60,000 synthetic rows (logistic everywhere, squaredError: the one autoencoder both ways can express).  Per
(stack, rows), milliseconds per call, median of `--reps` after one warm-up round, the two ways alternating:
  testEncoder  (new) to_autoencoder_stack_run with losses only
               (old) to_fflayer_stack_infer writing the reconstruction, then liftT (r - x)^2 and sumRows for the loss
  trainEncoder (new) to_autoencoder_stack_sgd
               (old) to_fflayer_stack_sgd with y = x  (the same launches by construction: the row says what noise looks like)
  trainEncoder, tanh code and tanh reconstruction (new only: the old entries cannot express it)
A call is timed with the host clock from before the call to after to_sync.
The head kernel: with `--kernels` the tool starts itself once more under `rocprofv3 --kernel-trace --stats` (a child
process of its own, `--child`), which issues in turn to_autoencoder_stack_run with a logistic reconstruction
(recon_head_kernel: z and the target in, the reconstruction and the loss out -- the logistic of loss_grad_rows_kernel),
to_autoencoder_stack_grad with a tanh reconstruction (recon_head_kernel: dz in place and the loss out) and
to_fflayer_stack_grad with y = x (loss_grad_rows_kernel on rows of the same width), and reads the kernels' average time from
the profiler's statistics.  Bytes per second count what the algorithm needs -- z and the target read once, one row written
once, 3 * rows * 784 * 4 bytes -- over that time, for all three.
A way that validation refuses (TO_ERR_UNSUPPORTED / ARG / SHAPE) is a row that says so.  Any other error, a child that exits
non-zero, or one that does not finish (it is killed with its process group) ends the tool with status 1 after it has written
what it measured: nothing is started on a device behind a failure.
usage: autoencoder_scan.py [--rows 1024,60000] [--stacks 784-256-784,784-256-64-256-784] [--reps 7] [--kernels] [--out DIR]"""
import argparse
import csv
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tensor_ops_amd.capi import TensorOpsError
from tensor_ops_amd.hipt import HipT


def stack(rng, sizes):
    return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), (0.1 * rng.standard_normal(o)).astype(np.float32))
            for i, o in zip(sizes[:-1], sizes[1:])]


def put(T, ws):
    return [T.put(w) for w, _ in ws], [T.put(b) for _, b in ws]


REFUSED = (1, 2, 5)      # TO_ERR_ARG, TO_ERR_SHAPE, TO_ERR_UNSUPPORTED: decided by validation, nothing launched


def timed(T, ways, reps):
    """{name: median seconds}, or {name: the error's text} for a way that validation refuses.  Any other error -- a HIP
    error above all -- is not caught: nothing more is started on a device that has just failed."""
    secs = {k: [] for k, _ in ways}
    failed = {}
    for rep in range(reps + 1):
        for k, f in ways:
            if k in failed:
                continue
            try:
                T.sync()
                t0 = time.perf_counter(); f(); T.sync(); t = time.perf_counter() - t0
            except TensorOpsError as e:
                if e.code not in REFUSED:
                    raise
                failed[k] = str(e)[:90]          # a row is information: say why it is missing and go on
                continue
            if rep > 0:
                secs[k].append(t)
    return {k: failed.get(k, float(np.median(v)) if v else "no run") for k, v in secs.items()}


def fmt(v):
    return "%10.3f" % (1e3 * v) if isinstance(v, float) else "  refused: " + v


def child(rows, reps):
    """the two head kernels on rows of width 784, alternately (run under the profiler)"""
    T = HipT(0, np.float32)
    rng = np.random.default_rng(3)
    ws = stack(rng, [784, 256, 784])
    W, b = put(T, ws)
    for n in rows:
        x = T.put(rng.uniform(0.05, 0.95, (n, 784)).astype(np.float32), batched=True)
        for _ in range(reps + 1):
            T.autoencoder_run(W, b, 1, x, "logistic", "squaredError", want_code=False)     # recon_head_kernel<float, 2, ..>
            T.autoencoder_grad(W, b, 1, x, "tanh", "squaredError", "logistic", "logistic", want_losses=True)   # <float, 3, ..>
            T.stack_grad(W, b, x, x, "logistic", "squaredError", want_losses=True)        # loss_grad_rows_kernel<float>
        T.sync()


# a piece of the kernel's name in the profiler's statistics -> what the row is called
KERNELS = {"recon_head_kernel<float, 2": "recon_head_kernel, logistic: z + bias, x -> recon, loss",
           "recon_head_kernel<float, 3": "recon_head_kernel, tanh: z, x -> dz in place, loss",
           "loss_grad_rows_kernel<float": "loss_grad_rows_kernel, logistic: z, y -> dz, loss"}


class ChildFailed(RuntimeError):
    pass


def profiled_child(cmd, limit):
    """the child in a process group of its own; at the limit the whole group is killed (the profiler AND the program under
    it, which has the device open).  A child that fails or hangs raises: no further child is started behind it."""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        raise ChildFailed("the profiled child did not finish within %d s and was killed with its process group" % limit)
    if p.returncode != 0:
        raise ChildFailed("the profiled child ended with status %d: %s" % (p.returncode, out.decode(errors="replace")[-300:]))


def kernel_rates(rows, reps, out_dir, say):
    d = tempfile.mkdtemp(prefix="autoencoder_scan_trace_", dir=out_dir)   # (the traces are not kept)
    try:
        for n in rows:          # one profiled run per row count: the statistics are per kernel name
            sub = os.path.join(d, "rows%d" % n)
            profiled_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", sub, "--", sys.executable,
                            os.path.abspath(__file__), "--child", "--rows", str(n), "--reps", str(reps)], 300)
            avg = {}
            for f in glob.glob(os.path.join(sub, "**", "*kernel_stats.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    for key in KERNELS:
                        if key in r.get("Name", ""):
                            avg[key] = (float(r["AverageNs"]), int(r["Calls"]))
            byts = 3.0 * n * 784 * 4
            for key in KERNELS:
                if key in avg:
                    ns, calls = avg[key]
                    say("%-52s %6d rows x 784: %9.2f us average over %d launches, %8.1f GB/s of the %d bytes the head needs" %
                        (KERNELS[key], n, ns / 1e3, calls, byts / ns, byts))
                else:
                    say("%-52s %6d rows x 784: not measured (no such kernel in the profiler's statistics)" % (KERNELS[key], n))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1024,60000")
    ap.add_argument("--stacks", default="784-256-784,784-256-64-256-784")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    a = ap.parse_args()
    rows = [int(v) for v in a.rows.split(",")]
    if a.child:
        return child(rows, a.reps)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    os.makedirs(a.out, exist_ok=True)
    status = 0
    try:
        scan(a, rows, say)
    except Exception as e:      # a device error, a child that failed or hung: what was measured is written, nothing more is started
        say("ended early, nothing further was started: %s" % str(e)[:400])
        status = 1
    with open(os.path.join(a.out, "autoencoder_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return status


def scan(a, rows, say):
    T = HipT(0, np.float32)
    rng = np.random.default_rng(1)
    say("autoencoder scan, fp32, synthetic rows in (0.05, 0.95); ms per call (host clock to to_sync), median of %d" % a.reps)
    say("%22s %6s | %-34s | %10s %10s" % ("stack", "rows", "what", "new", "old"))
    sq = T.expr(lambda v: (v[0] - v[1]) * (v[0] - v[1]), 2, key="autoencoder_scan_sq")
    for name in a.stacks.split(","):
        sizes = [int(v) for v in name.split("-")]
        n_enc = (len(sizes) - 1) // 2
        ws = stack(rng, sizes)
        for n in rows:
            x = T.put(rng.uniform(0.05, 0.95, (n, sizes[0])).astype(np.float32), batched=True)
            W, b = put(T, ws)

            def old_test():
                r, _, _ = T.infer_stack(W, b, x, out_act="logistic", want_out=True, want_classes=False)
                return T.sumRows(T.liftT(sq, [r, x]))

            res = timed(T, [("new", lambda: T.autoencoder_run(W, b, n_enc, x, want_code=False, want_recon=False)),
                            ("old", old_test)], a.reps)
            say("%22s %6d | %-34s | %s %s" % (name, n, "testEncoder (losses only)", fmt(res["new"]), fmt(res["old"])))
            W1, b1 = put(T, ws)
            W2, b2 = put(T, ws)
            res = timed(T, [("new", lambda: T.autoencoder_sgd(W1, b1, n_enc, x, 1e-4)),
                            ("old", lambda: T.stack_sgd(W2, b2, x, x, 1e-4, "logistic", "squaredError"))], a.reps)
            say("%22s %6d | %-34s | %s %s" % (name, n, "trainEncoder step", fmt(res["new"]), fmt(res["old"])))
            W3, b3 = put(T, ws)
            res = timed(T, [("new", lambda: T.autoencoder_sgd(W3, b3, n_enc, x, 1e-4, "tanh", "squaredError", "logistic", "tanh"))],
                        a.reps)
            say("%22s %6d | %-34s | %s %10s" % (name, n, "trainEncoder, tanh code + tanh out", fmt(res["new"]), "-"))
    if a.kernels:
        say("head kernels (rocprofv3 --kernel-trace --stats, a run of their own):")
        kernel_rates(rows, a.reps, a.out, say)
    else:
        say("head kernels: not measured (run with --kernels)")


if __name__ == "__main__":
    sys.exit(main())
