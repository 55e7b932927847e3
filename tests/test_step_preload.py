"""Kernarg preload in the batched step's kernels on the GENERATED gfx950 code, product and development build
alike: forward (gemm_t32_kernel<true,true,8,1,true,true>), loss head (gemm_small_head_kernel and its tanh twin) and the
weight-gradient pair (gemm_small_pair_kernel) take what stands in front of their first loads as LEADING SCALAR parameters,
which the dispatcher puts into user SGPRs (build.py, FLAGS), so

* `.amdhsa_user_sgpr_kernarg_preload_length` is the dword count of the kernel's leading scalars (read from the argument
  metadata of the same file: the offset of the first parameter that is no scalar or pointer) and at most 14, the user SGPRs
  are at most 16, and there is no scratch;
* behind the 256-byte compatibility header (firmware without preload enters there: loads, one wait, a branch) no `s_waitcnt`
  waits on `lgkmcnt` in front of the first vector-memory or LDS-DMA load;
* the pair asks for its first problem's operand members -- by hand, gemm_small.hip small_ask_operands -- in front of its first
  vector load, and nothing reads or copies a register of that request before the wait that small_take_operands issues.

And, on the host: the launchers' predicates for the arguments that became 32-bit (csrc/arg_fit.hpp), compiled into a
program of their own.  Built the way tests/test_step_prologue.py builds its kernels.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

import test_step_prologue as SP

HIPCC = SP.HIPCC
ROOT = SP.ROOT

# name -> (source, substring of the symbol, dwords of leading scalars)
#   forward: A, B (2 + 2), a_sx, b_sx, M, N, K, the packed map word, wmag0, wmag1
#   heads:   A, B (2 + 2), a_bytes, b_bytes, M, N, K, kper, a_sm, b_sn
#   pair:    Cin, bias, dact (2 + 2 + 2), n1 | order, M, N, map_d, map_mag, map_q, map_r, c_sm
KERNELS = {"forward": SP.FORWARD + (12,),
           "head": SP.HEAD + (12,),
           "head_tanh": ("gemm_small.hip", "gemm_small_head_tanh_kernel", 12),
           "pair": SP.PAIR + (14,),
           # the pair's short-K form (one wave per 16 x 16 tile, both problems): the same kernel template, the same request
           "pair_short": ("gemm_small.hip", "gemm_small_pair_kernelIfLi1ELi0ELi1ELi16ELi0ELi1ELi0ELi1ELi16ELi0E", 14)}
PAIR_FIRST = 56                       # byte offset of the pair's first argument block: behind fourteen dwords
PAIR_ASKED = (0, 16, 32, 64, 168)     # A B | a_bytes b_bytes | K kper | a_sm a_sk b_sk b_sn | rowsum rowsum_in


@pytest.fixture(scope="module")
def product_asm(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    return {src: SP._product(src, tmp) for src in ("gemm_small.hip", "gemm_t32.hip")}


@pytest.fixture(scope="module")
def development_asm(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm_dev")
    return {src: SP._compile(src, ["-DTOPS_AB_KNOBS"], tmp / ("development_" + src + ".s")) for src in ("gemm_small.hip", "gemm_t32.hip")}


def _lines(path):
    with open(path) as f:
        return f.read().split("\n")


def descriptor(lines, symbol):
    """the `.amdhsa_*` directives of one kernel as a dict of ints"""
    out, inside = {}, False
    for l in lines:
        t = l.strip()
        if t.startswith(".amdhsa_kernel"):
            inside = t.split()[1] == symbol
        elif t.startswith(".end_amdhsa_kernel"):
            inside = False
        elif inside and t.startswith(".amdhsa_"):
            k, v = t.split()[:2]
            out[k] = int(v, 0)
    assert out, symbol
    return out


def leading_dwords(lines, symbol):
    """(dwords in front of the first parameter that is neither a scalar nor a pointer, byte offset of that parameter), from the
    kernel's argument metadata"""
    at = next(n for n, l in enumerate(lines) if l.startswith("    .name:") and l.split()[-1] == symbol)
    # the `.args:` list of this kernel precedes its `.name:` in the metadata document; its entries are indented deeper
    lo = max(n for n in range(at) if lines[n].strip() in ("- .args:", ".args:"))
    args, cur = [], None
    for l in lines[lo + 1:at]:
        if not l.startswith("      "):
            break
        t = l.strip()
        if t.startswith("- ."):
            cur = {}
            args.append(cur)
            t = t[2:]
        if cur is not None and t.startswith(".") and ":" in t:
            k, v = t.split(":", 1)
            cur[k] = v.strip()
    for a in args:
        if a.get(".value_kind") in ("by_value", "global_buffer") and int(a[".size"]) <= 8:
            continue
        off = int(a[".offset"])
        return (off + 3) // 4, off
    raise AssertionError("no argument block behind the scalars of " + symbol)


def body_behind_header(lines, pattern):
    """(symbol, instructions of the kernel behind its 256-byte compatibility header, instructions of the header)"""
    import asm_schedule
    name, body, _ = asm_schedule.kernel_text(lines, pattern)
    text = [l.split(";")[0].strip() for l in body]
    cut = next((n for n, t in enumerate(text) if re.match(r"\.p2align\s+8$", t)), None)
    assert cut is not None, "no compatibility header in " + name
    keep = lambda ts: [t for t in ts if t and not t.endswith(":") and not t.startswith(".")]
    return name, keep(text[cut:]), keep(text[:cut])


def prologue(ins):
    first = next(i for i, t in enumerate(ins) if SP.VECTOR_LOAD.match(t))
    return ins[:first]


def lgkm_waits(ins):
    return [t for t in ins if t.startswith("s_waitcnt") and "lgkmcnt" in t]


def sgprs(token_text):
    """scalar registers named in an operand list"""
    out = set()
    for lo, hi in re.findall(r"\bs\[(\d+):(\d+)\]", token_text):
        out.update(range(int(lo), int(hi) + 1))
    out.update(int(r) for r in re.findall(r"\bs(\d+)\b", token_text))
    return out


def scalar_requests(ins):
    """[(index, destination registers, byte offset)] of the s_load_dword* instructions"""
    out = []
    for i, t in enumerate(ins):
        m = re.match(r"s_load_dword\w*\s+(\S+),\s*(\S+),\s*(\S+)", t)
        if m:
            out.append((i, sgprs(m.group(1).rstrip(",")), int(m.group(3), 0)))
    return out


def pair_report(ins):
    """of the pair kernel behind its header: which of the first block's operand members are asked for in front of the first
    vector load, and the instructions between that request and the first wait on lgkmcnt that name one of its registers"""
    first = next(i for i, t in enumerate(ins) if SP.VECTOR_LOAD.match(t))
    asked = [(i, regs, off) for i, regs, off in scalar_requests(ins[:first]) if off - PAIR_FIRST in PAIR_ASKED]
    pending = set().union(*[regs for _, regs, _ in asked]) if asked else set()
    last = max((i for i, _, _ in asked), default=-1)
    wait = next(i for i, t in enumerate(ins) if i > last and t.startswith("s_waitcnt") and "lgkmcnt(0)" in t)
    touched = [t for t in ins[last + 1:wait] if sgprs(t.split(None, 1)[1] if " " in t else "") & pending]
    return {"asked": sorted(off - PAIR_FIRST for _, _, off in asked), "wait_behind_first_load": wait > first, "touched": touched}


def symbols(lines, pattern):
    """the kernels of the file whose symbol contains `pattern` (a development build holds every form of the pair)"""
    return [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel") and pattern in l]


def check_kernel(lines, which, symbol):
    src, pattern, dwords = KERNELS[which]
    name, ins, header = body_behind_header(lines, symbol)
    d = descriptor(lines, name)
    lead, off = leading_dwords(lines, name)
    assert name == symbol
    print(which, name, {k: d[k] for k in (".amdhsa_user_sgpr_kernarg_preload_length", ".amdhsa_user_sgpr_count",
                                           ".amdhsa_private_segment_fixed_size")}, "leading dwords", lead)
    assert lead == dwords
    assert d[".amdhsa_user_sgpr_kernarg_preload_length"] == lead <= 14
    assert d[".amdhsa_user_sgpr_count"] <= 16
    assert d[".amdhsa_private_segment_fixed_size"] == 0 and d.get(".amdhsa_uses_dynamic_stack", 0) == 0
    assert len(lgkm_waits(header)) == 1                      # the header: loads, ONE wait, the branch
    assert lgkm_waits(prologue(ins)) == []
    if which.startswith("pair"):
        assert off == PAIR_FIRST
        r = pair_report(ins)
        print(r)
        assert r["asked"] == sorted(PAIR_ASKED) and r["wait_behind_first_load"] and r["touched"] == []


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("which", sorted(KERNELS))
def test_product_kernels_start_from_preloaded_arguments(product_asm, which):
    lines = _lines(product_asm[KERNELS[which][0]])
    names = symbols(lines, KERNELS[which][1])
    assert len(names) == 1, names
    check_kernel(lines, which, names[0])


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("which", sorted(KERNELS))
def test_development_build_agrees(product_asm, development_asm, which):
    """the product's instance among the development build's -- and every other form of it that build can launch"""
    src, pattern, _ = KERNELS[which]
    product = symbols(_lines(product_asm[src]), pattern)
    lines = _lines(development_asm[src])
    names = symbols(lines, pattern)
    assert set(product) <= set(names), (product, names)
    for name in names:
        check_kernel(lines, which, name)


SNIPPET = """
\t.text
_ZN2to9k_preloadEPKfiNS_4ArgsE:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\ts_load_dword s4, s[0:1], 0x8
\ts_waitcnt lgkmcnt(0)
\ts_branch .LBB0_0
\t.p2align\t8
.LBB0_0:
\ts_load_dwordx4 s[8:11], s[0:1], 56
\ts_load_dwordx2 s[12:13], s[0:1], 0x48
\ts_add_i32 s5, s4, 31
\ts_mov_b32 s20, s13
\tglobal_load_dword v1, v0, s[2:3]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tbuffer_load_dword v2, v1, s[8:11], 0 offen
\ts_endpgm
.Lfunc_end0:
\t.size\t_ZN2to9k_preloadEPKfiNS_4ArgsE, .Lfunc_end0-_ZN2to9k_preloadEPKfiNS_4ArgsE
\t.amdhsa_kernel _ZN2to9k_preloadEPKfiNS_4ArgsE
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_user_sgpr_count 5
\t\t.amdhsa_user_sgpr_kernarg_preload_length 3
\t.end_amdhsa_kernel
amdhsa.kernels:
  - .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         8
        .size:           4
        .value_kind:     by_value
      - .offset:         16
        .size:           64
        .value_kind:     by_value
    .group_segment_fixed_size: 0
    .name:           _ZN2to9k_preloadEPKfiNS_4ArgsE
"""


def test_reports_on_a_known_snippet():
    lines = SNIPPET.split("\n")
    name, ins, header = body_behind_header(lines, "k_preload")
    assert len(header) == 4 and len(lgkm_waits(header)) == 1
    assert ins[0].startswith("s_load_dwordx4") and lgkm_waits(prologue(ins)) == []          # the wait behind the first load does not count
    d = descriptor(lines, name)
    assert (d[".amdhsa_user_sgpr_kernarg_preload_length"], d[".amdhsa_user_sgpr_count"]) == (3, 5)
    assert leading_dwords(lines, name) == (4, 16)      # 12 bytes of scalars, padded to the block's alignment: NOT the preload length
    assert sgprs("s[8:11], s20, v1, vcc") == {8, 9, 10, 11, 20}
    r = pair_report(ins)
    assert r["asked"] == [0, 16] and r["wait_behind_first_load"]
    assert r["touched"] == ["s_mov_b32 s20, s13"]      # a copy of a register that has not arrived: what must not happen


HOST_PROGRAM = r"""
#include <cstdio>
#include "arg_fit.hpp"
using namespace to;
int main() {
  const long long G = 1LL << 30;
  int bad = 0;
  auto expect = [&](bool got, bool want, const char* what) { if (got != want) { std::printf("WRONG: %s\n", what); ++bad; } };
  // the step's forward: X [1024][784] . W1^T [256][784], both k-contiguous
  expect(t32_spans_fit(1024, 256, 784, 784, 1, 784, 1), true, "the step's forward fits");
  // a span of 2 GiB and more: (M + 32) rows of a_sm floats
  expect(t32_spans_fit(1024, 256, 784, (2 * G / 4) / (1024 + 32) + 1, 1, 784, 1), false, "A spans 2 GiB");
  expect(t32_spans_fit(1024, 256, 784, 784, 1, (2 * G / 4) / (256 + 32) + 1, 1), false, "B spans 2 GiB");
  expect(t32_spans_fit(1024, 256, 784, (2 * G / 4 - 784) / (1024 + 32) - 1, 1, 784, 1), true, "A just below 2 GiB");
  // a stride that does not fit 32 bits, whatever the extents
  expect(t32_spans_fit(4, 4, 4, 1LL << 31, 1, 4, 1), false, "a_sm = 2^31");
  expect(t32_spans_fit(4, 4, 4, 4, 1, 1, 1LL << 32), false, "b_sk = 2^32");
  expect(t32_spans_fit(4, 4, 4, (1LL << 32) + 4, 1, 4, 1), false, "a_sm = 2^32 + 4 (its low word alone would pass)");
  expect(t32_spans_fit(1LL << 40, 4, 4, 1, 1, 4, 1), false, "M = 2^40");
  expect(t32_spans_fit(4, 4, 1LL << 29, 1, 4, 1, 4), false, "K = 2^29");
  // the pair's output row stride
  expect(fits_i32(784), true, "c_sm = 784");
  expect(fits_i32((1LL << 31) - 1), true, "c_sm = 2^31 - 1");
  expect(fits_i32(1LL << 31), false, "c_sm = 2^31");
  expect(fits_i32((1LL << 32) + 784), false, "c_sm = 2^32 + 784");
  std::printf("%d wrong\n", bad);
  return bad ? 1 : 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_launchers_refuse_strides_and_spans_that_do_not_fit(tmp_path):
    src = tmp_path / "fit.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "fit"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tensor-ops_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
