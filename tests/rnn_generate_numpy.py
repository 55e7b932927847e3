"""A plain numpy restatement of closed-loop generation (to_rnn_stack_generate): one `step` of a recurrent stack, the three
`feed` rules and `generate` -- prime, then every output fed back -- in a chosen dtype (float64 unless said otherwise).
tests/test_rnn_generate_numpy_ref.py holds `step` to oracle/recurrent.py; tests/test_gpu_rnn_generate.py uses `feed` as the
exact statement of the symbol rule and `generate` to pick stacks whose closed loop visits several symbols.

A layer is (s, Ws, W, b, state_act): s [n] or [B, n], Ws = W' [n, n] and state_act "logistic" or "tanh" for a fullyConnected
layer; None, None and None for an ffLayer.  One step: z = W a + W' s + b, new state state_act(z), layer output hidden(z),
out_act(z) for the last layer."""
import numpy as np


def sig(z):
    return 1 / (1 + np.exp(-z))


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


ACT = {"logistic": sig, "tanh": np.tanh}


def initial_states(layers, B, dt=np.float64):
    return [None if lay[0] is None else np.broadcast_to(np.asarray(lay[0], dt), (B, lay[2].shape[0])).copy() for lay in layers]


def step(layers, x, states, hidden="logistic", out_act="softmax", dt=np.float64):
    """x [B, i], states per layer ([B, n] or None) -> (out [B, n_L], the new states)"""
    a, new = np.asarray(x, dt), []
    for l, (s, Ws, W, b, sa) in enumerate(layers):
        z = a @ np.asarray(W, dt).T + np.asarray(b, dt)
        if Ws is not None:
            z = z + states[l] @ np.asarray(Ws, dt).T
            new.append(ACT[sa](z))
        else:
            new.append(None)
        a = ACT[hidden](z) if l + 1 < len(layers) else (softmax(z) if out_act == "softmax" else sig(z))
    return a, new


def one_hot(c, n, dt):
    x = np.zeros((len(c), n), dt)
    x[np.arange(len(c)), c] = 1
    return x


def feed(prev, mode, u=None):
    """the next input rows from the STORED previous output rows prev [B, n], in prev's dtype: (x [B, n], symbols [B] or None).
    "argmax": the first index of the row maximum.  "sample": c_0 = p_0, c_j = c_{j-1} + p_j (np.cumsum accumulates
    sequentially, in the row's dtype), thr = u * c_{n-1}, the symbol = #{j : c_j <= thr}, at most n - 1."""
    prev = np.asarray(prev)
    dt, n = prev.dtype.type, prev.shape[-1]
    if mode == "output":
        return prev.copy(), None
    if mode == "argmax":
        c = prev.argmax(axis=-1)
    else:
        cum = np.cumsum(prev, axis=-1, dtype=dt)
        thr = np.asarray(u, dt) * cum[:, -1]
        assert cum.dtype == dt and thr.dtype == dt
        c = np.minimum((cum <= thr[:, None]).sum(axis=-1), n - 1)
    return one_hot(c, n, dt), c.astype(np.int64)


def generate(layers, X, G, mode="output", U=None, hidden="logistic", out_act="softmax", dt=np.float64):
    """X [B, Tp, i], U [B, G] for "sample": (out [B, G, n_L], symbols [B, G] or None, prime_out [B, Tp, n_L], final states,
    fed [B, G, i] -- the inputs of the generated steps)"""
    X = np.asarray(X, dt)
    B, Tp, _ = X.shape
    states = initial_states(layers, B, dt)
    prime = []
    for t in range(Tp):
        o, states = step(layers, X[:, t], states, hidden, out_act, dt)
        prime.append(o)
    prev, outs, syms, fed = prime[-1], [], [], []
    for k in range(G):
        x, c = feed(prev, mode, None if U is None else np.asarray(U, dt)[:, k])
        prev, states = step(layers, x, states, hidden, out_act, dt)
        outs.append(prev)
        fed.append(x)
        syms.append(c)
    return (np.stack(outs, 1), None if mode == "output" else np.stack(syms, 1), np.stack(prime, 1), states, np.stack(fed, 1))


def shift_stack(seed, i, spec, dt=np.float64, gain=6.0, noise=0.5):
    """A stack whose greedy closed loop walks through the symbols instead of collapsing onto one: N(0, noise^2) weights (a
    layer wider than 16: divided by sqrt(fan-in)) plus `gain` on an identity block in every layer but the last and on a
    one-step cyclic shift of the first n_L inputs in the last.  spec: [(n, state_act or None)], input to output."""
    rng = np.random.default_rng(seed)
    layers, prev, nL = [], i, spec[-1][0]
    for l, (n, sa) in enumerate(spec):
        k = noise / np.sqrt(prev) if max(n, prev) > 16 else noise
        W, b = k * rng.standard_normal((n, prev)), noise * rng.standard_normal(n)
        if l + 1 < len(spec):
            m = min(n, prev, nL)
            W[:m, :m] += gain * np.eye(m)
        else:
            for c in range(nL):
                W[(c + 1) % nL, c] += gain
        kn = noise / np.sqrt(n) if n > 16 else noise
        s, Ws = (noise * rng.standard_normal(n), kn * rng.standard_normal((n, n))) if sa else (None, None)
        layers.append(tuple(None if v is None else np.asarray(v, dt) for v in (s, Ws, W, b)) + (sa,))
        prev = n
    return layers
