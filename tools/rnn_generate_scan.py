"""to_rnn_stack_generate next to the loop a caller had to write before it, greedy (argmax) feed, softmax head, in fp32 and fp64:
  stacks  5 -> 7 (stateful) -> 5   and   64 -> 128 (stateful) -> 64
  B in {1, 32, 256, 4096} sequences (`--B`: other batch sizes, e.g. around the automatic rule's bound), G in {16, 256}
  generated steps after a prime of one step
Per (dtype, stack, B, G), milliseconds per whole generation, median of `--reps` after one warm-up round, the three ways
alternating:
  per step    to_rnn_stack_generate on route A (to_set_rnn_generate_persistent 0)
  persistent  to_rnn_stack_generate on route B (2); "per step" in brackets where the plan does not fit and route A ran
  caller      per generated step: to_arg_max of the last output row, to_one_hot, to_rnn_stack_run with T = 1 carrying the states
              -- the yardstick: what the same generation cost before the entry existed
A way is timed with the host clock from before its first call to after to_sync.  All three feed the same prime and must
arrive at the same symbols or the row says so (a greedy closed loop amplifies a last-bit difference into another symbol only
at a near-tie, so "differ" is information, not an error).
Every (dtype, stack) runs in a child process of its own under a time limit (`--limit` seconds; at the limit the child's
process group is killed).  A child that fails or does not finish ends the tool with status 1 after it has written what it
measured: nothing is started on a device behind a failure.
usage: rnn_generate_scan.py [--B 1,32,256,4096] [--G 16,256] [--reps 5] [--limit 240] [--out DIR]"""
import argparse
import os
import signal
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

STACKS = {"5-7s-5": (5, 7), "64-128s-64": (64, 128)}
DTYPES = {"f32": np.float32, "f64": np.float64}


def make(rng, i, H, dt):
    """i -> H (stateful, logistic) -> i with a cyclic shift in the last layer, so that the greedy loop walks"""
    W1 = rng.standard_normal((H, i)) / np.sqrt(i)
    W1[:i, :i] += 6 * np.eye(i)
    W2 = rng.standard_normal((i, H)) / np.sqrt(H)
    for c in range(i):
        W2[(c + 1) % i, c] += 6
    lay = [(0.5 * rng.standard_normal(H), rng.standard_normal((H, H)) / np.sqrt(H), W1, 0.5 * rng.standard_normal(H)),
           (None, None, W2, 0.5 * rng.standard_normal(i))]
    return [tuple(None if v is None else v.astype(dt) for v in l) for l in lay]


def child(a):
    from tensor_ops_amd.hipt import HipT
    dt = DTYPES[a.dtype]
    i, H = STACKS[a.stack]
    T = HipT(0, dt)
    rng = np.random.default_rng(7)
    layers = make(rng, i, H, dt)
    dl = [tuple(None if v is None else T.put(v) for v in lay) for lay in layers]
    for B in a.B:
        X = np.zeros((B, 1, i), dt)
        X[np.arange(B), 0, rng.integers(0, i, B)] = 1
        x = T.put(X, batched=True)
        for G in a.G:
            ran = {}

            def entry(mode):
                HipT.rnn_generate_persistent(mode)
                p0 = HipT.rnn_generate_stats()
                _, sym, _, _ = T.rnn_stack_generate(dl, x, G, "argmax")
                p1 = HipT.rnn_generate_stats()
                ran[mode] = "persistent" if p1[0] > p0[0] else "per step"
                return sym

            def caller():
                out, fin = T.rnn_stack_run(dl, x, "softmax", want_states=True)
                syms = []
                for _ in range(G):
                    c = T.arg_max(T.slice(out, (0,)))
                    syms.append(c)
                    xk = T.stack((1,), [T.one_hot(i, 1.0, 0.0, c)])
                    cur = [(fin[0],) + dl[0][1:], dl[1]]
                    out, fin = T.rnn_stack_run(cur, xk, "softmax", want_states=True)
                return np.stack(syms, axis=1)

            ways = [("per step", lambda: entry(0)), ("persistent", lambda: entry(2)), ("caller", caller)]
            secs, syms = {k: [] for k, _ in ways}, {}
            for rep in range(a.reps + 1):
                for k, f in ways:
                    T.sync()
                    t0 = time.perf_counter(); syms[k] = f(); T.sync(); t = time.perf_counter() - t0
                    if rep > 0:
                        secs[k].append(t)
            ms = {k: 1e3 * float(np.median(v)) for k, v in secs.items()}
            agree = all(np.array_equal(syms["caller"], syms[k]) for k in ("per step", "persistent"))
            note = "" if ran[2] == "persistent" else " (per step: no plan)"
            entry(1)   # (not timed: which route the automatic rule takes here)
            print("ROW %4s %11s %5d %4d | %10.3f %10.3f%s %10.3f | caller / persistent %6.2f  caller / per step %6.2f | automatic: %s | symbols %s" %
                  (a.dtype, a.stack, B, G, ms["per step"], ms["persistent"], note, ms["caller"], ms["caller"] / ms["persistent"],
                   ms["caller"] / ms["per step"], ran[1], "agree" if agree else "differ"), flush=True)
    HipT.rnn_generate_persistent(1)


class ChildFailed(RuntimeError):
    pass


def run_child(cmd, limit, say):
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
    ap.add_argument("--B", default="1,32,256,4096")
    ap.add_argument("--G", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--stack", default="5-7s-5")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    a = ap.parse_args()
    a.B = [int(v) for v in str(a.B).split(",")]
    a.G = [int(v) for v in str(a.G).split(",")]
    if a.child:
        return child(a)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    os.makedirs(a.out, exist_ok=True)
    say("rnn generate scan: greedy (argmax) closed loop, softmax head, prime of one step; ms per generation of G steps (host clock "
        "to to_sync), median of %d; B in %s, G in %s" % (a.reps, a.B, a.G))
    say("%4s %11s %5s %4s | %10s %10s %10s | %s" % ("", "stack", "B", "G", "per step", "persistent", "caller", "ratios (above 1: the entry is ahead of the caller's loop)"))
    status = 0
    try:
        for dtype in DTYPES:
            for stack in STACKS:
                run_child([sys.executable, os.path.abspath(__file__), "--child", "--dtype", dtype, "--stack", stack, "--B",
                           ",".join(map(str, a.B)), "--G", ",".join(map(str, a.G)), "--reps", str(a.reps)], a.limit, say)
    except ChildFailed as e:   # what was measured is written, nothing more is started
        say("ended early, nothing further was started: %s" % e)
        status = 1
    with open(os.path.join(a.out, "rnn_generate_scan.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
