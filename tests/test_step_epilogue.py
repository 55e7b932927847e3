"""What runs BEHIND the cross-wave reduction barrier of the step's loss head, on the GENERATED gfx950 code, product and
development build alike ("epilogues").  Every workgroup is on that stretch just before its kernel can end,
so a memory round trip there is paid in full.  In gemm_small_head_kernel and gemm_small_head_tanh_kernel, from the first
`s_barrier` to `s_endpgm`:

* no vector load (the target element leaves with the operand batch; the row sums' path is not compiled into these kernels),
* no scalar load (the cold members are in registers when the barrier opens),
* from the first store of the fused tail on no `s_waitcnt` that names `vmcnt` (the eight values are computed first, the
  eight stores go back to back through a descriptor: none waits for another's acknowledgement).

The weight-gradient pair is NOT checked here: fetching its row sums' old value ahead of the barrier and pinning its cold
members showed no gain and read slower, and its kernel is the parent's, instruction for instruction (DESIGN.md 3.4 and
profiles/README.md have the figures).

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
HEADS = ["gemm_small_head_kernel", "gemm_small_head_tanh_kernel"]
TAIL_STORES = 8    # two 16-column tiles a wave, four rows a lane

VECTOR_LOAD = re.compile(r"^(buffer_load_|global_load_|flat_load_|scratch_load_)")
STORE = re.compile(r"^(buffer_store_|global_store_|flat_store_)")


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


def instructions(path, pattern):
    """(symbol, [instructions in text order]) of the one kernel whose symbol contains `pattern`"""
    import asm_schedule
    with open(path) as f:
        lines = f.read().split("\n")
    name, body, _ = asm_schedule.kernel_text(lines, pattern)
    ins = [l.split(";")[0].strip() for l in body]
    return name, [t for t in ins if t and not t.endswith(":") and not t.startswith(".")]


def behind_barrier(ins):
    """the instructions behind the first s_barrier, up to and including the first s_endpgm behind it"""
    barrier = next(i for i, t in enumerate(ins) if t.startswith("s_barrier"))
    end = next(i for i, t in enumerate(ins) if i > barrier and t.startswith("s_endpgm"))
    return ins[barrier + 1:end + 1]


def epilogue_report(path, pattern):
    """of the stretch behind the kernel's first reduction barrier: vector loads, scalar loads, flat_ instructions, stores,
    and the waits naming vmcnt between and behind the fused tail's stores"""
    name, ins = instructions(path, pattern)
    ep = behind_barrier(ins)
    stores = [i for i, t in enumerate(ep) if STORE.match(t)]
    # the tail's stores: the last eight through a descriptor (a development build's stamps are plain stores behind branches)
    desc = [i for i in stores if ep[i].startswith("buffer_store_")]
    first, last = (desc[-TAIL_STORES], desc[-1]) if len(desc) >= TAIL_STORES else (len(ep), len(ep))
    waits = [i for i, t in enumerate(ep) if t.startswith("s_waitcnt") and "vmcnt" in t]
    return {"kernel": name,
            "vector_loads": sum(bool(VECTOR_LOAD.match(t)) for t in ep),
            "scalar_loads": sum(t.startswith(("s_load_", "s_buffer_load_")) for t in ep),
            "flat": sum(t.startswith("flat_") for t in ep),
            "stores": len(stores),
            "descriptor_stores": len(desc),
            "tail_vmcnt_waits": sum(first < i < last for i in waits),      # between the tail's stores
            "end_vmcnt_waits": sum(i > last for i in waits)}               # behind them, up to s_endpgm


def check_head(r, development=False):
    assert r["vector_loads"] == 0, r
    assert r["scalar_loads"] == 0, r
    assert r["descriptor_stores"] >= TAIL_STORES + 2, r     # dz and the row's loss, then the tail's eight
    assert r["tail_vmcnt_waits"] == 0, r
    # (a development build's stamped thread drains its stores for the `stores acknowledged` stamp: one wait, behind a branch
    #  that only it takes, behind the tail's last store)
    assert r["end_vmcnt_waits"] == (1 if development else 0), r


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("head", HEADS)
def test_product_head_waits_for_no_memory_behind_its_barrier(product_asm, head):
    check_head(epilogue_report(product_asm, head))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("head", HEADS)
def test_development_head_agrees(product_asm, development_asm, head):
    """the stamp code of a development build brings no load and no wait between the tail's stores back"""
    prod = epilogue_report(product_asm, head)
    check_head(epilogue_report(development_asm, prod["kernel"]), development=True)   # the same instance among the development build's


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_the_switched_back_forms_of_a_development_build_are_the_old_ones(development_asm):
    """TOPS_SMALL_EPI=0 (gemm_small_oldepi_*): the reader finds there what this change removed"""
    for head in ("gemm_small_oldepi_head_kernel", "gemm_small_oldepi_head_tanh_kernel"):
        r = epilogue_report(development_asm, head)
        assert r["vector_loads"] >= 1 and r["scalar_loads"] >= 1, r


SNIPPET = """
\t.text
_ZN2to22gemm_small_head_kernelEv:
\ts_load_dwordx4 s[20:23], s[0:1], 0x40
\tbuffer_load_dword v5, v0, s[0:3], 0 offen
\tv_mfma_f32_16x16x4_f32 v[32:35], v1, v2, v[32:35]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\ts_barrier
\ts_load_dword s24, s[0:1], 0xc4
\tglobal_load_dword v6, v[8:9], off
\ts_waitcnt vmcnt(0)
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tglobal_store_dword v[8:9], v6, off
\ts_barrier
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\ts_waitcnt vmcnt(0)
\tflat_store_dword v[8:9], v6
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\ts_waitcnt lgkmcnt(0)
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tbuffer_store_dword v6, v0, s[4:7], 0 offen
\tglobal_store_dwordx2 v[8:9], v[6:7], off
\ts_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)
\ts_endpgm
\tglobal_load_dword v7, v[8:9], off
\ts_barrier
\ts_endpgm
.Lfunc_end0:
\t.size\t_ZN2to22gemm_small_head_kernelEv, .Lfunc_end0-_ZN2to22gemm_small_head_kernelEv
"""


def test_reports_on_a_known_snippet(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(SNIPPET)
    r = epilogue_report(str(p), "gemm_small_head_kernel")
    # what stands in front of the barrier and behind the first s_endpgm does not count; the wait between the tail's third and
    # fourth store does, the one in front of the first descriptor store and the lgkmcnt wait do not; the drain in front of
    # s_endpgm is counted apart
    assert r == {"kernel": "_ZN2to22gemm_small_head_kernelEv", "vector_loads": 1, "scalar_loads": 1, "flat": 1, "stores": 12,
                 "descriptor_stores": 9, "tail_vmcnt_waits": 1, "end_vmcnt_waits": 1}
    with pytest.raises(AssertionError):
        check_head(r)
    with pytest.raises(AssertionError):
        check_head(dict(r, vector_loads=0, scalar_loads=0, descriptor_stores=10))   # (the wait between the tail's stores alone)
    check_head(dict(r, vector_loads=0, scalar_loads=0, descriptor_stores=10, tail_vmcnt_waits=0), development=True)
