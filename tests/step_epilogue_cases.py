"""The cases of tests/test_gpu_step_epilogue.py and how one of them is run: shared with tools/record_step_epilogue.py, which
records the parameters a library produces (tests/golden/step_epilogue/).  One step of a case is `trainNetwork` on a batch
through to_fflayer_stack_sgd: forward; output layer + loss head (+ the hidden layer's cotangent as its fused tail); the two
weight gradients with their updates, one pair launch where the pair forms.

A case is (name, rows, inputs, hidden, classes, out_act, loss, hidden_act, launches of a step).

Heads -- 17 and 33 rows (one / two full 16-row tiles and one masked row: rows beyond M are the lanes whose target the head
must read as 0), 3 / 10 / 16 classes (masked columns; none), hidden layers of
  40, 64   the lean head kernel, K of 2.5 and 4 chunks of 16: no fused tail (gemm_small_fuses_tail wants eight), dZ1 is a
           launch of its own;
  136      the lean head kernel WITH the fused tail, whose width -- 8.5 tiles of 16 columns -- is ragged;
  138      K no multiple of 4: no 16-byte operand loads, the generic 16x16 kernel, with the fused tail;
  272      K > 256: the generic kernel; a tail of 272 columns is not fused (at most 256);
40, 64 and 272 with every class count, 136 and 138 with two, and (rows, head, hidden activation) rotated over them so that
each of the eight combinations occurs (the full product would be 360 steps and a megabyte of recorded parameters for no
further path).  Launches: forward, head, [dZ1 where the tail is not fused], and the two weight gradients as the short-K
pair (eight inputs put dW1 on 16x16 tiles, and a K of 17 or 33 is one wave's): four, or three with the fused tail.

Pairs -- 50 -> 40 -> 10: dW1 is 40 x 50 on 2 x 2 tiles of 32 x 32, ragged in both directions, two of them with tile_n == 0
(the tiles that write the bias's row sums); at 720 rows K = 720 is the 16-wave one-shot pair (705..1024), at 16 the short-K
pair.  Hidden 40: no fused tail, four launches."""
import numpy as np

SEED = 0x7e5000a5
STEPS = (1, 5)     # the parameters are looked at after this many steps

SM, LG = ("softmax", "crossEntropy"), ("logistic", "squaredError")
HIDDEN_CLASSES = [(40, 3), (40, 10), (40, 16), (64, 3), (64, 10), (64, 16), (136, 10), (136, 16), (138, 3), (138, 16),
                  (272, 3), (272, 10), (272, 16)]


def _heads():
    combos = [(rows, head, act) for rows in (17, 33) for head in (SM, LG) for act in ("logistic", "tanh")]
    out = []
    for n, (hidden, classes) in enumerate(HIDDEN_CLASSES):
        rows, (out_act, loss), act = combos[n % len(combos)]
        fused_tail = hidden in (136, 138)
        launches = 3 if fused_tail else 4
        out.append(("head-r%d-h%d-c%d-%s-%s" % (rows, hidden, classes, out_act, act), rows, 8, hidden, classes, out_act, loss,
                    act, launches))
    return out


HEADS = _heads()
PAIRS = [("pair-r720", 720, 50, 40, 10, "softmax", "crossEntropy", "logistic", 4),
         ("pair-r16", 16, 50, 40, 10, "softmax", "crossEntropy", "logistic", 4)]
# the lean head kernel with the fused tail under softmax + crossEntropy too (the rotation gives hidden 136 the logistic head
# twice); appended, since a case's seed is its place in CASES
EXTRA = [("head-r33-h136-c10-softmax-tanh", 33, 8, 136, 10, "softmax", "crossEntropy", "tanh", 3),
         ("head-r17-h136-c3-softmax-logistic", 17, 8, 136, 3, "softmax", "crossEntropy", "logistic", 3)]
CASES = HEADS + PAIRS + EXTRA


def rate_of(rows):
    """the gradients are sums over the rows: a step of 0.5 on their mean"""
    return 0.5 / rows


def problem(case):
    """float32-representable parameters [(W, b)], X [rows, inputs], Y [rows, classes] of a case, from its seed"""
    name, rows, i, h, o = case[:5]
    rng = np.random.default_rng(SEED + CASES.index(case))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    ws = [(f32(0.5 * rng.standard_normal((h, i))), f32(0.5 * rng.standard_normal(h))),
          (f32(0.5 * rng.standard_normal((o, h))), f32(0.5 * rng.standard_normal(o)))]
    X = f32(rng.uniform(0, 1, size=(rows, i)))
    Y = np.zeros((rows, o))
    Y[np.arange(rows), rng.integers(0, o, size=rows)] = 1.0
    return ws, X, Y


def run(T, case):
    """({steps: [W1, b1, W2, b2] float32} for steps in STEPS, launches of one step) on the device"""
    name, rows, i, h, o, out_act, loss, act, _ = case
    ws, X, Y = problem(case)
    W, b = [T.put(w) for w, _ in ws], [T.put(v) for _, v in ws]
    x, y = T.put(X, batched=True), T.put(Y, batched=True)
    got, launches = {}, None
    for k in range(1, max(STEPS) + 1):
        T.sync()
        n0 = T.stats()["launches"]
        T.stack_sgd(W, b, x, y, rate_of(rows), out_act, loss, hidden_act=act)
        T.sync()
        n = T.stats()["launches"] - n0
        assert launches in (None, n), (launches, n)
        launches = n
        if k in STEPS:
            got[k] = [W[0].numpy(), b[0].numpy(), W[1].numpy(), b[1].numpy()]
    return got, launches


def keys(case, steps):
    return ["%s/%d/%s" % (case[0], steps, p) for p in ("W1", "b1", "W2", "b2")]
