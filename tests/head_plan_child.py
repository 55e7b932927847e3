"""Child process of tests/test_gpu_heads.py::test_planner_heads_with_a_loss_node (run as a script; the parent sets
TOPS_STEP_SEAM, which the library reads once at start).  A training step of config 3's shape class -- K -> 256 -> n <= 16 on a
few hundred rows -- is recorded call by call through the class-method stream, WITH the loss -sum y log p asked for beside the
gradients, so that the planner's fused head carries a loss node.  The logits are the table's rows: W_1 = 0 and b_1 = 0 make
every hidden unit logistic(0) = 1/2, the rows of W_2 sum to zero, b_2 is the row.  Prints one JSON line: the launches of each
step, the worst errors, what missed."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import head_cases as HC  # noqa: E402
import nonfinite_ref as NR  # noqa: E402
import test_gpu_heads as G  # noqa: E402

K, HID, B = 256, 256, 416          # 13 row blocks of 32 x 8 tiles of the first layer: inside the joined kernel's 96 .. 512 tiles


def step(T, hipt, W1, b1, W2, b2, x, y):
    """forward, softmax >>> crossEntropy with its loss, backward, the four gradients: all deferred, demanded together"""
    with T.memo():
        a1 = T.sumT([T.gmul(1, 1, 0, W1, x), b1], (HID,))
        h = T.liftT(hipt.logistic_closure, [a1], key="heads-logistic")
        a2 = T.sumT([T.gmul(1, 1, 0, W2, h), b2], (W2.shape[0],))
        e = T.liftT(lambda v: hipt.exp(v[0]), [a2], key="heads-exp")
        r = T.liftT(lambda v: 1.0 / v[0], [T.sumRows(e)], key="heads-recip")
        p = T.gmul(0, 0, 1, r, e)
        loss = T.scaleT(-1.0, T.sumRows(T.liftT(lambda v: v[0] * hipt.log(v[1]), [y, p], key="heads-ylogp")))
        dz2 = T.liftT(lambda v: v[0] - v[1], [T.gmul(0, 0, 1, T.sumRows(y), p), y], key="heads-sub")
        dh = T.gmul(1, 1, 0, T.transp(W2), dz2)
        dz1 = T.liftT(lambda v: v[0] * ((1.0 / (1.0 + hipt.exp(-v[1]))) * (1.0 - 1.0 / (1.0 + hipt.exp(-v[1])))), [dh, a1],
                      key="heads-dlogistic")
        outs = [loss, T.gmul_batch_sum(1, 0, 1, dz2, T.transp(h)), T.batch_sum(dz2),
                T.gmul_batch_sum(1, 0, 1, dz1, T.transp(x)), T.batch_sum(dz1)]
        T.force_many(outs)
    return [o.numpy() for o in outs]


def main():
    from tensor_ops_amd import hipt
    T = hipt.HipT(0)
    dt = np.float32
    rep = G.Report(dt)
    rng = np.random.default_rng(0x7e5)
    X = rng.integers(-4, 5, (B, K)).astype(np.float64)
    H = np.full((B, HID), 0.5)
    launches = {}
    for n in (10, 16):
        W2 = rng.integers(-3, 4, (n, HID)).astype(np.float64)
        W2[:, -1] -= W2.sum(axis=1)
        counts = set()
        for cid, zrow, Yfew in G.shared_batches(n, dt):
            Y = Yfew[np.arange(B) % len(Yfew)]
            G.nan_pool(T, B, n * HID, n, HID * K, HID, B * n, B * HID)
            args = [T.put(np.zeros((HID, K))), T.put(np.zeros(HID)), T.put(W2), T.put(zrow), T.put(X, batched=True),
                    T.put(Y, batched=True)]
            got, k = G.counted(T, lambda: step(T, hipt, *args))
            counts.add(k)
            _, dz, loss = HC.softmax_ce(np.broadcast_to(zrow, Y.shape), Y)
            dz1 = 0.25 * NR.contract(dz, W2)
            want = [loss, NR.contract(dz.T, H), NR.sum_rows(dz), NR.contract(dz1.T, X), NR.sum_rows(dz1)]
            for name, g, w, how in zip(("loss", "gW2", "gb2", "gW1", "gb1"), got, want, ("loss", "rel", "rel", "rel", "rel")):
                rep.hold(cid, name, g, w, how)
        launches[str(n)] = sorted(counts)
    print(json.dumps({"launches": launches, "worst": rep.worst, "fails": rep.fails}))


if __name__ == "__main__":
    main()
