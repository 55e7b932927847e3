"""CPU: the ragged recurrent entries are part of the C ABI -- include/tensorops_hip.h declares them with the argument lists
the ctypes table binds, the built library exports them and the Python binding names them and takes `lens=`."""
import inspect
import os
import re
import subprocess

import pytest

import tensor_ops_amd  # noqa: F401
from tensor_ops_amd import capi

ENTRIES = {"to_rnn_stack_run_ragged": 12, "to_rnn_stack_grad_ragged": 18, "to_rnn_stack_sgd_ragged": 15,
           "to_rnn_ragged_stats": 2}


@pytest.fixture(scope="module")
def built(repo_root):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tops_build", os.path.join(repo_root, "tensor-ops_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build()


def test_header_declares_the_entries(repo_root):
    text = open(os.path.join(repo_root, "include", "tensorops_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in ENTRIES.items():
        m = re.search(r"to_status\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        args = m.group(1).split(",")
        assert len(args) == n_args, name
        assert len(capi.SIGNATURES[name]) == n_args, name
        if name != "to_rnn_ragged_stats":   # lens sits directly after the data tensors
            after = {"to_rnn_stack_run_ragged": "X"}.get(name, "Y")
            k = [i for i, a in enumerate(args) if re.search(r"\bto_tensor\s+%s$" % after, a.strip())]
            assert len(k) == 1 and re.search(r"const\s+int64_t\s*\*\s*lens$", args[k[0] + 1].strip()), name
            assert capi.SIGNATURES[name][k[0] + 1] is capi.i64p, name


def test_library_exports_the_entries(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(re.findall(r" T (to_[a-z0-9_]+)", out))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported


def test_python_binding_names_the_methods():
    from tensor_ops_amd.hipt import HipT
    assert callable(HipT.rnn_ragged_stats)
    for name in ("rnn_stack_run", "rnn_stack_grad", "rnn_stack_sgd"):
        p = inspect.signature(getattr(HipT, name)).parameters
        assert "lens" in p and p["lens"].default is None, name
