"""The loss-head launch of the batched step (gemm_small_head_kernel: the one-shot 16x16 body of two chunks a wave) on the
GENERATED gfx950 code, product and development build alike:

* its K loop -- everything in front of the first workgroup barrier, where the eight partial tiles meet -- holds the 8 MFMAs of
  two chunks, not the 16 of the two-stage pipeline's four (two of which were masked to zeros for K <= 256);
* no `ds_bpermute_b32` anywhere in it: the sixteen-lane reductions of softmax / crossEntropy (max, sum e, sum y, sum loss) are
  row-local DPP moves, twenty of them (four reductions of four steps, xor 4 taking two);
* no scratch.
Built the way tests/test_step_schedule.py builds its kernels.  No GPU needed."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SRC = "gemm_small.hip"
HEAD = "gemm_small_head_kernel"


def _build_mod():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tops_build", os.path.join(ROOT, "tensor-ops_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _compile(extra, out):
    b = _build_mod()
    spath = os.path.join(ROOT, "tensor-ops_amd", "csrc", SRC)
    flags = [f for f in b.FLAGS if not f.startswith("-DTOPS_")]
    r = subprocess.run([HIPCC] + flags + extra + ["--cuda-device-only", "-S", "-o", str(out), "-x", "hip", spath],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    """the device assembly of the product build: the file the build kept, or (stale / absent) a fresh -S"""
    b = _build_mod()
    kept = b.device_asm(SRC)
    csrc = os.path.join(ROOT, "tensor-ops_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hpp", ".h")) or f == SRC)
    if os.path.exists(kept) and os.path.getmtime(kept) >= newest and not any(f.startswith("-DTOPS_") for f in b.FLAGS):
        return kept
    return _compile([], tmp_path_factory.mktemp("asm") / "product.s")


@pytest.fixture(scope="module")
def development_asm(tmp_path_factory):
    return _compile(["-DTOPS_AB_KNOBS"], tmp_path_factory.mktemp("asm") / "development.s")


def head_report(path):
    """of the head kernel: MFMAs in front of the first s_barrier, MFMAs in all, ds_bpermute count, DPP moves, scratch bytes"""
    import asm_schedule
    with open(path) as f:
        lines = f.read().split("\n")
    name, body, tail = asm_schedule.kernel_text(lines, HEAD)
    ins = [l.split(";")[0].strip() for l in body]
    ins = [t for t in ins if t and not t.endswith(":") and not t.startswith(".")]
    barrier = next(i for i, t in enumerate(ins) if t.startswith("s_barrier"))
    _, _, scratch = asm_schedule.resources(name, tail)
    return {"k_loop_mfmas": sum(t.startswith("v_mfma_f32_16x16x4") for t in ins[:barrier]),
            "mfmas": sum(t.startswith("v_mfma") for t in ins),
            "bpermute": sum(t.startswith("ds_bpermute") for t in ins),
            "dpp": sum(bool(re.search(r"\b(quad_perm|row_ror|row_shl|row_shr):", t)) for t in ins),
            "scratch": scratch}


def check(r):
    assert r["k_loop_mfmas"] == 8, r          # two chunks of four MFMAs; the fused tail's eight sit behind the barriers
    assert r["mfmas"] == 16, r
    assert r["bpermute"] == 0, r
    assert r["dpp"] == 20, r
    assert r["scratch"] == 0, r


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_product_head_kernel_is_the_lean_instance(product_asm):
    check(head_report(product_asm))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_development_build_agrees(product_asm, development_asm):
    """the stamp code of a development build adds no MFMA in front of the barrier and brings no shuffle back"""
    dev = head_report(development_asm)
    check(dev)
    assert dev == head_report(product_asm)


SNIPPET = """
\t.text
_ZN2to22gemm_small_head_kernelEv:
\tbuffer_load_dwordx4 v[1:4], v0, s[0:3], 0 offen
\ts_waitcnt vmcnt(0)
\tv_mfma_f32_16x16x4_f32 v[32:35], v1, v2, v[32:35]
\tds_write_b32 v5, v32
\ts_barrier
\tv_add_f32_dpp v6, v6, v6 row_ror:8 row_mask:0xf bank_mask:0xf
\tv_mov_b32_dpp v7, v6 row_shl:4 row_mask:0xf bank_mask:0x5
\tds_bpermute_b32 v8, v9, v6
\tv_mfma_f32_16x16x4_f32 v[32:35], v3, v4, v[32:35]
\ts_endpgm
.Lfunc_end0:
\t.size\t_ZN2to22gemm_small_head_kernelEv, .Lfunc_end0-_ZN2to22gemm_small_head_kernelEv
; Kernel info:
; NumVgprs: 36
; NumAgprs: 0
; ScratchSize: 0
"""


def test_report_on_a_known_snippet(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(SNIPPET)
    assert head_report(str(p)) == {"k_loop_mfmas": 1, "mfmas": 2, "bpermute": 1, "dpp": 2, "scratch": 0}
