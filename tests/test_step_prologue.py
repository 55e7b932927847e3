"""The prologues of the batched step's three kernels -- forward (gemm_t32_kernel<true,true,8,1,true,true>), loss head
(gemm_small_head_kernel), weight-gradient pair (gemm_small_pair_kernel) -- on the GENERATED gfx950 code, product and
development build alike: in front of the first vector-memory or LDS-DMA load there is

* exactly one `s_waitcnt` that waits on `lgkmcnt` -- the argument block's hot part arrives in ONE scalar round trip, not
  three (tile grid, then the pointers behind the tile map's arithmetic, then whatever the next branch needed);
* no `v_rcp_iflag_f32` -- the workgroup -> tile maps divide by multiply-high with reciprocals planned on the host;

and in the head kernel no vector load lies between the K loop's last MFMA and the reduction barrier (the fused tail's
operands leave with the operand batch).  Built the way tests/test_step_schedule.py builds its kernels.  No GPU needed."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

FORWARD = ("gemm_t32.hip", "gemm_t32_kernelILb1ELb1ELi8ELi1ELb1ELb1E")    # <AKC, BKC, 8 waves, 1 stage, EARLY, REGU>
HEAD = ("gemm_small.hip", "gemm_small_head_kernel")
PAIR = ("gemm_small.hip", "gemm_small_pair_kernelIfLi1ELi0ELi16ELi32ELi8ELi1ELi0ELi8ELi16ELi8E")   # as tests/test_step_schedule.py
KERNELS = {"forward": FORWARD, "head": HEAD, "pair": PAIR}

VECTOR_LOAD = re.compile(r"^(buffer_load_|global_load_|flat_load_|scratch_load_)")   # (global_load_lds_*: the LDS DMA)


def _build_mod():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tops_build", os.path.join(ROOT, "tensor-ops_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _compile(src, extra, out):
    b = _build_mod()
    spath = os.path.join(ROOT, "tensor-ops_amd", "csrc", src)
    flags = [f for f in b.FLAGS if not f.startswith("-DTOPS_")]
    r = subprocess.run([HIPCC] + flags + extra + ["--cuda-device-only", "-S", "-o", str(out), "-x", "hip", spath],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def _product(src, tmp):
    """the device assembly of the product build: the file the build kept, or (stale / absent) a fresh -S"""
    b = _build_mod()
    kept = b.device_asm(src)
    csrc = os.path.join(ROOT, "tensor-ops_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hpp", ".h")) or f == src)
    if os.path.exists(kept) and os.path.getmtime(kept) >= newest and not any(f.startswith("-DTOPS_") for f in b.FLAGS):
        return kept
    return _compile(src, [], tmp / ("product_" + src + ".s"))


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    return {src: _product(src, tmp) for src in ("gemm_small.hip", "gemm_t32.hip")}


@pytest.fixture(scope="module")
def development_asm(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm_dev")
    return {src: _compile(src, ["-DTOPS_AB_KNOBS"], tmp / ("development_" + src + ".s")) for src in ("gemm_small.hip", "gemm_t32.hip")}


def instructions(path, pattern):
    """(symbol, [instructions in text order]) of the one kernel whose symbol contains `pattern`"""
    import asm_schedule
    with open(path) as f:
        lines = f.read().split("\n")
    name, body, _ = asm_schedule.kernel_text(lines, pattern)
    ins = [l.split(";")[0].strip() for l in body]
    return name, [t for t in ins if t and not t.endswith(":") and not t.startswith(".")]


def prologue_report(path, pattern):
    """of the code in front of the kernel's first vector-memory / LDS-DMA load: waits on lgkmcnt, v_rcp_iflag_f32"""
    name, ins = instructions(path, pattern)
    first = next(i for i, t in enumerate(ins) if VECTOR_LOAD.match(t))
    pro = ins[:first]
    return {"kernel": name,
            "lgkm_waits": sum(t.startswith("s_waitcnt") and "lgkmcnt" in t for t in pro),
            "rcp": sum(t.startswith("v_rcp_iflag_f32") for t in pro)}


def head_loads_behind_k_loop(path, pattern):
    """vector loads between the last MFMA in front of the first s_barrier (the K loop's last) and that barrier"""
    _, ins = instructions(path, pattern)
    barrier = next(i for i, t in enumerate(ins) if t.startswith("s_barrier"))
    last = max(i for i, t in enumerate(ins[:barrier]) if t.startswith("v_mfma"))
    return sum(bool(VECTOR_LOAD.match(t)) for t in ins[last + 1:barrier])


def check(r):
    assert r["lgkm_waits"] == 1, r
    assert r["rcp"] == 0, r


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("which", sorted(KERNELS))
def test_product_prologue(product_asm, which):
    src, pattern = KERNELS[which]
    check(prologue_report(product_asm[src], pattern))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_product_head_has_no_load_behind_its_k_loop(product_asm):
    assert head_loads_behind_k_loop(product_asm[HEAD[0]], HEAD[1]) == 0


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("which", sorted(KERNELS))
def test_development_build_agrees(product_asm, development_asm, which):
    """the stamps of a development build (entry clock, first operand load) add no wait and no division in front of the first load"""
    src, pattern = KERNELS[which]
    prod = prologue_report(product_asm[src], pattern)
    dev = prologue_report(development_asm[src], prod["kernel"])   # the same instance among the development build's
    check(dev)
    assert dev == prod
    if which == "head":
        assert head_loads_behind_k_loop(development_asm[src], pattern) == 0


SNIPPET = """
\t.text
_ZN2to22gemm_small_head_kernelEv:
\ts_load_dwordx16 s[4:19], s[0:1], 0x0
\ts_load_dwordx4 s[20:23], s[0:1], 0x40
\ts_waitcnt lgkmcnt(0)
\tv_rcp_iflag_f32_e32 v1, v1
\ts_load_dword s24, s[0:1], 0x50
\ts_waitcnt vmcnt(0)
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tglobal_load_lds_dwordx4 v2, s[4:5] offset:0
\ts_waitcnt lgkmcnt(0)
\tv_rcp_iflag_f32_e32 v1, v1
\tbuffer_load_dwordx4 v[1:4], v0, s[0:3], 0 offen
\tv_mfma_f32_16x16x4_f32 v[32:35], v1, v2, v[32:35]
\tbuffer_load_dword v5, v0, s[0:3], 0 offen
\tv_mfma_f32_16x16x4_f32 v[32:35], v3, v4, v[32:35]
\tglobal_load_dword v6, v[8:9], off
\tds_write_b32 v5, v32
\ts_barrier
\tglobal_load_dword v7, v[8:9], off
\tv_mfma_f32_16x16x4_f32 v[32:35], v3, v4, v[32:35]
\ts_barrier
\ts_endpgm
.Lfunc_end0:
\t.size\t_ZN2to22gemm_small_head_kernelEv, .Lfunc_end0-_ZN2to22gemm_small_head_kernelEv
"""


def test_reports_on_a_known_snippet(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(SNIPPET)
    r = prologue_report(str(p), "gemm_small_head_kernel")
    assert (r["lgkm_waits"], r["rcp"]) == (2, 1)          # the waits and the division behind the DMA load do not count
    assert head_loads_behind_k_loop(str(p), "gemm_small_head_kernel") == 1   # the load between the MFMAs is in the K loop
    with pytest.raises(AssertionError):
        check(r)
