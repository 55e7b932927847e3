"""The weight-gradient pair launch of the batched step (gemm_small_pair_kernel: dW1 on 16-wave one-shot 32x32 tiles) owes its
time to the ORDER of one wave's 64 operand loads and 32 MFMAs.  Left to the compiler that order differed between the
product build (16 loads, then the rest dripped between MFMAs that each waited for a load issued a few instructions
earlier) and the development build the stamps are taken with (a branch between loads and MFMAs: all 64 loads first).
gemm_small_body now pins it (PARTS / STAG, scheduling barriers); this file asserts, on the GENERATED gfx950 code, what
DESIGN.md 3.4 relies on: the loads ahead of the first MFMA, waits that leave exactly the younger loads in flight, no
scratch, at most 128 VGPRs (1,024 threads a workgroup), and the same order with and without -DTOPS_AB_KNOBS.
tools/asm_schedule.py prints the same table for any kernel.  No GPU needed."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SRC = "gemm_small.hip"
PAIR = "gemm_small_pair_kernelIfLi1ELi0ELi16ELi32ELi8ELi1ELi0ELi8ELi16ELi8E"   # <float, 1,0,16,32,8, 1,0,8,16,8, ...>
# what ships (gemm_small.hip SMALL_PAIR_PARTS / SMALL_PAIR_STAG): chunks a part, and the loads in front of MFMA 1 --
# the operand loads of parts 0 and 1 plus the three epilogue prefetches (W1's old value, issued first)
CHUNKS = 8
EPILOGUE_LOADS = 3


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


def _parts_of(symbol):
    """PARTS and STAG from the last two template arguments of the pair kernel's symbol"""
    import re
    m = re.search(re.escape(PAIR) + r"Li(\d+)ELb([01])E", symbol)
    assert m, symbol
    return int(m.group(1)), bool(int(m.group(2)))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_product_pair_kernel_runs_the_pinned_schedule(product_asm):
    import asm_schedule
    r = asm_schedule.report(product_asm, PAIR, "32x32x2")   # (exactly one instance in a product build)
    parts, _ = _parts_of(r["kernel"])
    assert parts >= 1, "the pair's 32x32 body is compiler-scheduled again"
    assert r["scratch"] == 0 and r["vgprs"] <= 128 and (r["agprs"] or 0) == 0, r
    assert r["mfmas"] == 4 * CHUNKS and r["loads"] == 8 * CHUNKS + EPILOGUE_LOADS, r
    cp = CHUNKS // parts                       # chunks a part
    ahead = min(2, parts) * cp * 8             # parts 0 and 1 are out before the first MFMA
    assert r["loads_ahead"] == ahead + EPILOGUE_LOADS, r
    # MFMA j of chunk c issues when the chunk's loads up to b[c][j] are back: A's four, then B's j + 1 -- and everything
    # younger (the rest of the chunk, the later chunks of its part, the whole next part) is still in flight
    want = []
    for c in range(CHUNKS):
        p = c // cp
        issued = min(p + 2, parts) * cp * 8    # operand loads issued when part p's MFMAs run
        for j in range(4):
            want.append(issued - (c * 8 + 4 + j + 1))
    assert r["vmcnt"] == want, (r["vmcnt"], want)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_development_build_generates_the_same_order(product_asm, development_asm):
    """the stamp code of a development build (a branch and a store at each stamp point) does not move a load or an MFMA"""
    import asm_schedule
    prod = asm_schedule.report(product_asm, PAIR, "32x32x2")
    dev = asm_schedule.report(development_asm, prod["kernel"], "32x32x2")   # the same instance among the development build's
    assert dev["scratch"] == 0 and dev["vgprs"] <= 128, dev
    assert dev["order"] == prod["order"], (asm_schedule.runs(dev["order"]), asm_schedule.runs(prod["order"]))
    assert dev["loads_ahead"] == prod["loads_ahead"]
    assert dev["vmcnt"] == prod["vmcnt"], (dev["vmcnt"], prod["vmcnt"])


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_every_development_form_fits_the_register_file(development_asm):
    """the A/B forms a development build can be steered onto (TOPS_SMALL_PARTS x TOPS_SMALL_STAGGER): none spills"""
    import asm_schedule
    for parts in (0, 1, 2, 4, 8):
        for stag in ((0,) if parts == 0 else (0, 1)):
            r = asm_schedule.report(development_asm, PAIR + "Li%dELb%dE" % (parts, stag), "32x32x2")
            assert r["scratch"] == 0 and r["vgprs"] <= 128 and r["mfmas"] == 32, r


SNIPPET = """
\t.text
_Z1kv:
\tbuffer_load_dword v1, v0, s[0:3], 0 offen
\tbuffer_load_dword v2, v0, s[0:3], 0 offen offset:4
\tglobal_load_dword v3, v[8:9], off
\ts_waitcnt vmcnt(1)
\tv_mfma_f32_32x32x2_f32 v[16:31], v1, v2, v[16:31]
\tbuffer_load_dword v4, v0, s[0:3], 0 offen offset:8
\tv_mfma_f32_16x16x4_f32 v[32:35], v1, v2, v[32:35]
\tv_add_f32_e32 v5, v1, v2
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_mfma_f32_32x32x2_f32 v[16:31], v3, v4, v[16:31]
\tglobal_store_dword v[8:9], v16, off
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z1kv, .Lfunc_end0-_Z1kv
; Kernel info:
; NumVgprs: 36
; NumAgprs: 0
; ScratchSize: 0
"""


def test_schedule_tool_on_a_known_snippet(tmp_path):
    import asm_schedule
    p = tmp_path / "k.s"
    p.write_text(SNIPPET)
    r = asm_schedule.report(str(p), "_Z1kv", "32x32x2")
    assert (r["vgprs"], r["agprs"], r["scratch"]) == (36, 0, 0)
    assert r["loads"] == 4 and r["loads_ahead"] == 3 and r["mfmas"] == 2
    assert r["vmcnt"] == [1, 0] and r["order"] == "LLLMLM"
    assert asm_schedule.runs(r["order"]) == "L3 M1 L1 M1"
    with pytest.raises(SystemExit):
        asm_schedule.report(str(p), "no_such_kernel")
