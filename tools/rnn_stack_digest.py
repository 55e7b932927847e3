"""Every recurrent one-call entry on the smallest cases at which its shared host code can go wrong, one line per call: what
was launched and a digest of what came out.  Two builds whose lines are equal launch the same work and compute the same
bits, so the file is what a host-side change of csrc/stack_rnn.cpp is compared by (profiles/README.md).  Per line:
  entry dtype rnn=<0|1|2> [gen=|online=<0|2>] stack batch [case]    (rnn: the to_set_rnn_persistent setting)
  L=  T.stats()["launches"] of the SECOND of two identical calls (the first warms the pool and the plan caches)
  C=  what that call added to the four (persistent, per-step) counter pairs: rnn / ragged / generate / online
  then the sha256 of the raw bytes of every output of that call, each behind its name and shape: out, final states, every
  gradient, gx, losses -- for the SGD entries the updated initial states and parameters.  A line shows the first 16 hex
  digits, enough to say which call moved; the last line of the file is the sha256, in full, of all the calls' full digests
Stacks (input width, then layer widths; s = stateful, f = stateless; T = 5 but for the one-step stack):
  6-8s-4f            stateful, then stateless                                softmax / crossEntropy
  3-4s-5f-2s         a stateful output layer over a stateless middle one     softmax / crossEntropy
  9-37s-300s-11f     300 is past the LDS rule: automatic routing mixes routes  softmax / crossEntropy
  4-4s               T = 1                                                   logistic / squaredError
  6-8t-4f            tanh states under a logistic hidden activation (the Ah pass)  softmax / crossEntropy
Generation feeds the output back as the input, so there each stack's input width is its output width.  Batches: unbatched
(the B == 1 shortcuts) and B = 7; run also with initial states [B; n].  Lengths: [3, 1, 5, 5, 2, 5, 1] (ties for the stable
sort, length 1, full length) and all equal to T; an unbatched ragged call (no shortcut there, but no batch stride either) on the
first stack only.  The settings are crossed where the host code branches on them, not everywhere: fp32 runs rnn = 0 and 2 on
every stack and 1 (automatic) on the mixed stack, the only one where 1 differs from 2; fp64 runs 0 and 1 on every stack and
2 on the mixed stack, the only one where 2 differs from 1; generation and online SGD run on their own routes 0 and 2 under
rnn = 1, their shared forward's other settings being the run lines'.  Everything is seeded by the case's own name.
usage: rnn_stack_digest.py [--out FILE] [--each]      (--each: a digest per output, to find which one moved)"""
import argparse
import hashlib
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tensor_ops_amd.hipt import HipT

STACKS = [  # name, input width, [(width, state activation or None)], hidden, out, loss, T
    ("6-8s-4f", 6, [(8, "logistic"), (4, None)], "logistic", "softmax", "crossEntropy", 5),
    ("3-4s-5f-2s", 3, [(4, "logistic"), (5, None), (2, "logistic")], "logistic", "softmax", "crossEntropy", 5),
    ("9-37s-300s-11f", 9, [(37, "logistic"), (300, "logistic"), (11, None)], "logistic", "softmax", "crossEntropy", 5),
    ("4-4s", 4, [(4, "logistic")], "logistic", "logistic", "squaredError", 1),
    ("6-8t-4f", 6, [(8, "tanh"), (4, None)], "logistic", "softmax", "crossEntropy", 5),
]
B = 7
LENS = [3, 1, 5, 5, 2, 5, 1]
G = 3
IDX = [2, 0, 2, 1, 3]   # online: sequence 2 twice
RATES = (0.05, 0.1)


class Case:
    """the host arrays of one (stack, batch): parameters, data, targets; everything uploaded afresh for every call"""

    def __init__(self, Tb, name, i, spec, T, batch, closed_loop=False, n_seq=None):
        self.Tb, self.T = Tb, T
        dt = Tb.dtype
        rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (name, batch, closed_loop)).encode()))
        nL = spec[-1][0]
        i = nL if closed_loop else i
        self.host = []
        fan = i
        for n, sa in spec:
            mk = lambda *s: np.asarray(rng.standard_normal(s) / np.sqrt(s[-1]), dt)  # noqa: E731
            self.host.append((mk(n) if sa else None, mk(n, n) if sa else None, mk(n, fan), mk(n), sa))
            fan = n
        nb = n_seq or max(batch, 1)
        self.batched = batch > 0 or n_seq is not None
        lead = (nb,) if self.batched else ()
        self.X = rng.uniform(-1, 1, lead + (T, i)).astype(dt)
        self.Y = rng.dirichlet(np.ones(nL), lead + (T,)).astype(dt)
        self.S0 = [None if h[0] is None else np.asarray(rng.standard_normal((nb, len(h[0]))), dt) for h in self.host]
        self.U = rng.uniform(0, 1, lead + (G,)).astype(dt)

    def layers(self, batched_states=False):
        put = self.Tb.put
        out = []
        for (s, ws, w, b, sa), s0 in zip(self.host, self.S0):
            if s is None:
                out.append((None, None, put(w), put(b)))
            else:
                out.append((put(s0, batched=True) if batched_states else put(s), put(ws), put(w), put(b), sa))
        return out

    def data(self):
        return self.Tb.put(self.X, batched=self.batched), self.Tb.put(self.Y, batched=self.batched)


def named(prefix, ts):
    return [("%s%d" % (prefix, l), t) for l, t in enumerate(ts or []) if t is not None]


def params(layers):
    return [("%s%d" % (nm, l), t) for l, lay in enumerate(layers) for nm, t in zip(("s", "ws", "w", "b"), lay[:4]) if t is not None]


def counters():
    return HipT.rnn_stats() + HipT.rnn_ragged_stats() + HipT.rnn_generate_stats() + HipT.rnn_online_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--each", action="store_true")
    a = ap.parse_args()
    lines = []
    total = hashlib.sha256()

    def line(Tb, label, call):
        """call() twice on fresh uploads; the second call's launches, counters and outputs"""
        call()
        l0, c0 = Tb.stats()["launches"], counters()
        outs = call()
        l1, c1 = Tb.stats()["launches"], counters()
        d = [y - x for x, y in zip(c0, c1)]
        hs = []
        for nm, t in outs:
            v = np.ascontiguousarray(t if isinstance(t, np.ndarray) else t.numpy())
            hs.append((nm, ("%s%s" % (nm, v.shape)).encode() + v.tobytes()))
        if a.each:
            dig = " ".join("%s=%s" % (nm, hashlib.sha256(raw).hexdigest()[:16]) for nm, raw in hs)
        else:
            full = hashlib.sha256(b"".join(raw for _, raw in hs)).hexdigest()
            total.update(full.encode())
            dig = full[:16]
        s = "%s L=%d C=%d,%d/%d,%d/%d,%d/%d,%d %s" % ((label, l1 - l0) + tuple(d) + (dig,))
        print(s, flush=True)
        lines.append(s)

    mixed, first = STACKS[2][0], STACKS[0][0]
    every = [st[0] for st in STACKS]
    for dname, dt, plan in (("f32", np.float32, ((0, every), (1, [mixed]), (2, every))),
                            ("f64", np.float64, ((0, every), (1, every), (2, [mixed])))):
        Tb = HipT(0, dt)
        for route, names in plan:
            HipT.rnn_persistent(route)
            HipT.rnn_generate_persistent(0)
            HipT.rnn_online_persistent(0)
            for name, i, spec, hid, oact, loss, T in STACKS:
                for batch in (0, B) if name in names else ():
                    c = Case(Tb, name, i, spec, T, batch)
                    kw = dict(out_act=oact, hidden_act=hid)
                    kl = dict(kw, loss=loss)
                    lens_sets = [("lens=mixed", [min(v, T) for v in LENS]), ("lens=T", [T] * B)] if batch else [
                        ("lens=3", [min(3, T)])] if name == first else []

                    def run(lens=None, bs=False):
                        x, _ = c.data()
                        out, fin = Tb.rnn_stack_run(c.layers(bs), x, want_states=True, lens=lens, **kw)
                        return [("out", out)] + named("s_out", fin)

                    def grad(lens=None):
                        x, y = c.data()
                        gs, gws, gw, gb, gx, ls = Tb.rnn_stack_grad(c.layers(), x, y, want_gx=True, want_losses=True, lens=lens, **kl)
                        return named("gs", gs) + named("gws", gws) + named("gw", gw) + named("gb", gb) + [("gx", gx), ("losses", ls)]

                    def sgd(lens=None):
                        x, y = c.data()
                        lay = c.layers()
                        ls = Tb.rnn_stack_sgd(lay, x, y, RATES[0], RATES[1], want_losses=True, lens=lens, **kl)
                        return params(lay) + [("losses", ls)]

                    head = "%s rnn=%d %s B=%d" % (dname, route, name, batch)
                    line(Tb, "run " + head, run)
                    if batch:
                        line(Tb, "run " + head + " states=[B;n]", lambda: run(bs=True))
                    line(Tb, "grad " + head, grad)
                    line(Tb, "sgd " + head, sgd)
                    for lname, lens in lens_sets:
                        line(Tb, "run_ragged " + head + " " + lname, lambda: run(lens))
                        if batch:
                            line(Tb, "run_ragged " + head + " " + lname + " states=[B;n]", lambda: run(lens, True))
                        line(Tb, "grad_ragged " + head + " " + lname, lambda: grad(lens))
                        line(Tb, "sgd_ragged " + head + " " + lname, lambda: sgd(lens))
            for sub in (0, 2) if route == 1 else ():   # the two chained entries: per step / per sequence, and their kernels
                HipT.rnn_generate_persistent(sub)
                HipT.rnn_online_persistent(sub)
                for name, i, spec, hid, oact, loss, T in STACKS:
                    kw = dict(out_act=oact, hidden_act=hid)
                    for batch in (0, B):
                        c = Case(Tb, name, i, spec, T, batch, closed_loop=True)
                        for feed in ("output", "argmax", "sample"):
                            def gen():
                                x, _ = c.data()
                                u = Tb.put(c.U, batched=batch > 0) if feed == "sample" else None
                                out, sym, prime, fin = Tb.rnn_stack_generate(c.layers(), x, G, feed=feed, U=u, want_prime_out=True,
                                                                             want_states=True, **kw)
                                return [("out", out), ("prime_out", prime)] + ([("symbols", sym)] if sym is not None else []) + named("s_out", fin)
                            line(Tb, "generate %s rnn=%d gen=%d %s B=%d feed=%s" % (dname, route, sub, name, batch, feed), gen)
                    c = Case(Tb, name, i, spec, T, 0, n_seq=4)

                    def online():
                        x, y = c.data()
                        lay = c.layers()
                        ls = Tb.rnn_stack_online_sgd(lay, x, y, RATES[0], RATES[1], idx=IDX, want_losses=True, loss=loss, **kw)
                        return params(lay) + [("losses", ls)]
                    line(Tb, "online_sgd %s rnn=%d online=%d %s N=4 idx=%s" % (
                        dname, route, sub, name, ",".join(map(str, IDX))), online)
    HipT.rnn_persistent(1)
    HipT.rnn_generate_persistent(1)
    HipT.rnn_online_persistent(1)
    if not a.each:
        lines.append("all %d calls sha256=%s" % (len(lines), total.hexdigest()))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
