"""to_rnn_stack_online_sgd next to the loop a caller had to write before it: N = 256 sequences, one trainNetwork' step each,
softmax head over a stateless output layer, hidden logistic:
  fp32 and fp64  5 -> 7 (stateful) -> 5,  64 -> 64 (stateful) -> 10,  64 -> 128 (stateful) -> 64
  fp32 only      64 -> H (stateful) -> 10 for H = 32 / 64 / 96 / 128 (the widths the automatic rule's H* is read from)
  T in {8, 64}; logistic states, plus one row with a tanh state and tanh hidden layers
Per (dtype, stack, T), microseconds per sequence, median of `--reps` (7) after one warm-up round, the three ways alternating:
  caller      a loop of to_rnn_stack_sgd over to_batch_select views of X / Y (the views made once, outside the clock) -- the
              yardstick: what the same training cost before the entry existed
  route A     to_rnn_stack_online_sgd per sequence (to_set_rnn_online_persistent 0)
  route B     to_rnn_stack_online_sgd persistent (2); "route A" in brackets where the plan does not fit and route A ran
A way is timed with the host clock around the blocking call(s).  Every way trains its own copy of the parameters, all from
the same start; small rates keep 8 x 256 updates finite.
H* (include/tensorops_hip.h) is the largest scanned H of the fp32 64 -> H -> 10 rows at which route B is
at least as fast as route A at both T; the tool prints it.
Every dtype runs in a child process of its own under a time limit (`--limit` seconds; at the limit the child's process group
is killed).  A child that fails or does not finish ends the tool with status 1 after it has written what it measured:
nothing is started on a device behind a failure.
usage: rnn_online_scan.py [--N 256] [--T 8,64] [--reps 7] [--limit 300] [--out DIR]"""
import argparse
import os
import signal
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

DTYPES = {"f32": np.float32, "f64": np.float64}
# (name, i, H, n_L, state / hidden activation, dtypes)
ROWS = [("5-7s-5", 5, 7, 5, "logistic", ("f32", "f64")),
        ("64-64s-10", 64, 64, 10, "logistic", ("f32", "f64")),
        ("64-128s-64", 64, 128, 64, "logistic", ("f32", "f64")),
        ("64-32s-10", 64, 32, 10, "logistic", ("f32",)),
        ("64-96s-10", 64, 96, 10, "logistic", ("f32",)),
        ("64-128s-10", 64, 128, 10, "logistic", ("f32",)),
        ("64-64s-10 tanh", 64, 64, 10, "tanh", ("f32",))]
RATES = (0.01, 0.002)


def make(rng, i, H, o, act, dt):
    lay = [(0.5 * rng.standard_normal(H), rng.standard_normal((H, H)) / np.sqrt(H), rng.standard_normal((H, i)) / np.sqrt(i),
            0.5 * rng.standard_normal(H), act),
           (None, None, rng.standard_normal((o, H)) / np.sqrt(H), 0.5 * rng.standard_normal(o), False)]
    return [tuple(v.astype(dt) if isinstance(v, np.ndarray) else v for v in l) for l in lay]


def child(a):
    from tensor_ops_amd.hipt import HipT
    dt = DTYPES[a.dtype]
    T = HipT(0, dt)
    N = a.N
    for name, i, H, o, act, dts in ROWS:
        if a.dtype not in dts:
            continue
        for n in a.T:
            rng = np.random.default_rng(11)
            layers = make(rng, i, H, o, act, dt)
            x = T.put(rng.uniform(-1, 1, (N, n, i)).astype(dt), batched=True)
            y = T.put(rng.uniform(0.1, 0.9, (N, n, o)).astype(dt), batched=True)
            xs, ys = [T.batch_select(x, q) for q in range(N)], [T.batch_select(y, q) for q in range(N)]
            dev = lambda: [tuple(T.put(v) if isinstance(v, np.ndarray) else v for v in lay) for lay in layers]  # noqa: E731
            nets = {"caller": dev(), "route A": dev(), "route B": dev()}
            ran = {}

            def entry(key, mode):
                HipT.rnn_online_persistent(mode)
                p0 = HipT.rnn_online_stats()
                T.rnn_stack_online_sgd(nets[key], x, y, RATES[0], RATES[1], hidden_act=act)
                ran[mode] = "B" if HipT.rnn_online_stats()[0] > p0[0] else "A"

            def caller():
                for q in range(N):
                    T.rnn_stack_sgd(nets["caller"], xs[q], ys[q], RATES[0], RATES[1], hidden_act=act)

            ways = [("caller", caller), ("route A", lambda: entry("route A", 0)), ("route B", lambda: entry("route B", 2))]
            secs = {k: [] for k, _ in ways}
            for rep in range(a.reps + 1):
                for k, f in ways:
                    T.sync()
                    t0 = time.perf_counter(); f(); t = time.perf_counter() - t0
                    if rep > 0:
                        secs[k].append(t)
            us = {k: 1e6 * float(np.median(v)) / N for k, v in secs.items()}
            note = "" if ran[2] == "B" else " (route A: no plan)"
            nets["auto"] = dev()
            entry("auto", 1)   # (not timed: which route the automatic rule takes here)
            finite = all(np.isfinite(t.numpy()).all() for k in ("caller", "route A", "route B") for lay in nets[k]
                         for t in lay[:4] if t is not None)
            print("ROW %4s %15s %3d | %9.2f %9.2f %9.2f%s | caller / B %6.2f  A / B %6.2f | automatic: %s%s" %
                  (a.dtype, name, n, us["caller"], us["route A"], us["route B"], note, us["caller"] / us["route B"],
                   us["route A"] / us["route B"], ran[1], "" if finite else " | NOT FINITE"), flush=True)
            if a.dtype == "f32" and name.endswith("-10") and ran[2] == "B":
                print("HSTAR %d %d %d" % (H, n, int(us["route B"] <= us["route A"])), flush=True)
    HipT.rnn_online_persistent(1)


class ChildFailed(RuntimeError):
    pass


def run_child(cmd, limit, say, hstar):
    """the child in a process group of its own; at the limit the whole group is killed.  Its rows are passed on as they come."""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True, text=True)
    t0, tail = time.monotonic(), []
    try:
        import selectors
        sel = selectors.DefaultSelector()
        sel.register(p.stdout, selectors.EVENT_READ)
        while True:
            left = limit - (time.monotonic() - t0)
            if left <= 0:
                raise subprocess.TimeoutExpired(cmd, limit)
            if not sel.select(timeout=left):
                continue
            line = p.stdout.readline()
            if not line:
                break
            if line.startswith("ROW "):
                say(line[4:].rstrip())
            elif line.startswith("HSTAR "):
                H, n, ahead = (int(v) for v in line.split()[1:])
                hstar.setdefault(H, {})[n] = bool(ahead)
            else:
                tail.append(line.rstrip())
        p.wait(timeout=max(1.0, limit - (time.monotonic() - t0)))
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.wait()
        raise ChildFailed("%s did not finish within %d s and was killed with its process group" % (" ".join(cmd[-6:]), limit))
    if p.returncode != 0:
        raise ChildFailed("%s ended with status %d: %s" % (" ".join(cmd[-6:]), p.returncode, " | ".join(tail[-6:])[-400:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--T", default="8,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    a = ap.parse_args()
    a.T = [int(v) for v in str(a.T).split(",")]
    if a.child:
        return child(a)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    os.makedirs(a.out, exist_ok=True)
    say("rnn online scan: one trainNetwork' step a sequence over N = %d sequences, softmax head; microseconds per sequence (host "
        "clock around the blocking calls), median of %d; T in %s" % (a.N, a.reps, a.T))
    say("%4s %15s %3s | %9s %9s %9s | %s" % ("", "stack", "T", "caller", "route A", "route B",
                                             "ratios (above 1: route B is ahead)"))
    status, hstar = 0, {}
    try:
        for dtype in DTYPES:
            run_child([sys.executable, os.path.abspath(__file__), "--child", "--dtype", dtype, "--N", str(a.N), "--T",
                       ",".join(map(str, a.T)), "--reps", str(a.reps)], a.limit, say, hstar)
        ok = [H for H in sorted(hstar) if len(hstar[H]) == len(a.T) and all(hstar[H].values())]
        say("H* (fp32 64 -> H (stateful) -> 10, logistic: the largest scanned H with route B at least as fast as route A at every "
            "T): %s" % (max(ok) if ok else "none"))
    except ChildFailed as e:   # what was measured is written, nothing more is started
        say("ended early, nothing further was started: %s" % e)
        status = 1
    with open(os.path.join(a.out, "rnn_online_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
