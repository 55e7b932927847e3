"""A null pointer argument of the dense and ragged recurrent entries is refused by name: TO_ERR_ARG and the message
"null argument: <the parameter's name in include/tensorops_hip.h>", whichever entry and whichever argument.  The message is
the argument's spelling at the check (NONNULL), so it changes silently when the check is moved behind another name."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STACK = ["state_act", "s", "ws", "w", "b"]
GRADS = ["gs", "gws", "gw", "gb"]
CASES = [(e + sfx, null) for sfx in ("", "_ragged") for e, names in (
    ("run", STACK + ["X", "out"]), ("grad", STACK + ["X", "Y"] + GRADS), ("sgd", STACK + ["X", "Y"]))
    for null in names + (["lens"] if sfx else [])]


@pytest.fixture(scope="module")
def args():
    from tensor_ops_amd import capi
    from tensor_ops_amd.hipt import HipT
    T = HipT(0)
    keep = []   # the handles live as long as the fixture: the arrays below hold raw pointers only

    def one(*shape):
        keep.append(T.put(np.full(shape, 0.25)))
        return (capi.c_tensor * 1)(keep[-1].h)
    seq = lambda n: T.put(np.full((2, 3, n), 0.25), batched=True)  # noqa: E731
    keep += [seq(3), seq(4), seq(4)]
    a = {"state_act": (C.c_int * 1)(0), "s": one(4), "ws": one(4, 4), "w": one(4, 3), "b": one(4), "gs": one(4), "gws": one(4, 4),
         "gw": one(4, 3), "gb": one(4), "lens": (C.c_int64 * 2)(2, 3), "X": keep[0].h, "Y": keep[1].h, "out": keep[2].h}
    return a, keep


@pytest.mark.parametrize("entry,null", CASES, ids=["%s-%s" % c for c in CASES])
def test_null_argument_is_named(args, entry, null):
    from tensor_ops_amd import capi
    a = dict(args[0], **{null: None})
    lens = (a["lens"],) if entry.endswith("_ragged") else ()
    head = (1, a["state_act"], a["s"], a["ws"], a["w"], a["b"], 0, 2)   # logistic hidden, softmax
    if entry.startswith("run"):
        tail = (a["X"],) + lens + (a["out"], None)
    elif entry.startswith("grad"):
        tail = (1, a["X"], a["Y"]) + lens + (a["gs"], a["gws"], a["gw"], a["gb"], None, None)
    else:
        tail = (1, a["X"], a["Y"]) + lens + (0.0, 0.0, None)
    status = getattr(capi.lib(), "to_rnn_stack_" + entry)(*(head + tail))
    assert status == 1   # TO_ERR_ARG
    assert capi.lib().to_last_error().decode() == "null argument: " + null
