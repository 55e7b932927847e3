"""tensor-ops-mnist with `--minibatch M --onecall`: every "Batch" of the app trained by ONE to_fflayer_stack_minibatch_sgd over
the epoch's permutation (host/apps/mnist.cpp).  The command line and the assertions are those of
tests/test_mnist_app.py::test_app_learns_the_synthetic_set for `--minibatch 50`, plus the app's `update:` line."""
import subprocess

import pytest

from test_mnist_app import app

pytestmark = pytest.mark.gpu


def test_app_learns_the_synthetic_set_in_one_call_a_batch(repo_root):
    out = subprocess.run([app(repo_root), "--synthetic", "2000,400", "--layers", "[32,16]", "--batch", "500",
                          "--rate", "0.05", "--epochs", "2", "--minibatch", "50", "--onecall"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("Synthetic data") and "Loaded data." in lines and "Data processed." in lines
    assert any(l.startswith("rate: 0.05") and "layers: [32,16]" in l for l in lines)
    assert "update: one-call minibatch SGD over 50 samples" in lines
    assert not any(l.startswith("update: batched gradTOp") for l in lines)
    assert lines.count("[Epoch 1]") == 1 and lines.count("[Epoch 2]") == 1
    val = [float(l.split()[1].rstrip("%")) for l in lines if l.startswith("Validation:")]
    assert len(val) >= 8 and val[-1] < 15.0 and val[-1] < val[0], val
    # confusion matrix: 10 rows "[r] c0 c1 ..." after every batch, entries sum to the set size
    k = max(i for i, l in enumerate(lines) if l.startswith("Validation:"))
    rows = lines[k + 1:k + 11]
    assert [r.split()[0] for r in rows] == ["[%d]" % i for i in range(10)]
    assert sum(int(v) for r in rows for v in r.split()[1:]) == 400


def test_onecall_needs_a_minibatch(repo_root):
    out = subprocess.run([app(repo_root), "--synthetic", "20,10", "--onecall"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--onecall needs --minibatch" in out.stderr
