"""A plain `bench.py --gpus 1 --steps K --warmup W` run: exactly K timed steps in one region, the headline line, and
with --dump-outputs the parameters the last timed step produced -- held here to W + K steps of the same update replayed by
the fp64 oracle from the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_plain_line_and_dumped_outputs(repo_root, tmp_path):
    steps, warmup = 3, 2
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(repo_root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=repo_root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["timing"]["regions"] == 1 and d["timing"]["steps_per_region"] == steps
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 2e-3
    assert d["step"]["params_finite_after_timed_region"] is True
    assert d["cpu_baseline"] is None and d["roofline"] is None and d["steady_state"] is None   # (--full legs)

    import bench
    from oracle import hmat
    ws, X, Y = bench.synth(0, 1024)
    p = [ws[0][0], ws[0][1], ws[1][0], ws[1][1]]
    for _ in range(warmup + steps):
        g, _ = hmat.batched_grads(X, Y, *p, recompute=False)
        p = [w - bench.RATE / 1024 * gw for w, gw in zip(p, g)]
    names = ["layer1_weights", "layer1_bias", "layer2_weights", "layer2_bias"]
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    for name, want in zip(names, p):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == want.shape, name
        err = np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want)
        assert err < 1e-5, (name, err)
