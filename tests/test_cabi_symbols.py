"""CPU-side checks of the drop-in boundary: the library builds, loads, exports every
symbol include/tensorops_hip.h declares, and refuses to compute without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import tensor_ops_amd  # noqa: F401
from tensor_ops_amd import capi


@pytest.fixture(scope="module")
def built(repo_root):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_tops_build", os.path.join(repo_root, "tensor-ops_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.build()


def declared_symbols(repo_root):
    text = open(os.path.join(repo_root, "include", "tensorops_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(to_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(built, repo_root):
    names = declared_symbols(repo_root)
    assert len(names) >= 55
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(re.findall(r" T (to_[a-z0-9_]+)", out))
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    # nothing but the C ABI leaks out of the library
    leaked = [l for l in out.splitlines() if " T " in l and " T to_" not in l]
    assert not leaked, leaked


def test_ctypes_table_matches_header(built, repo_root):
    names = set(declared_symbols(repo_root))
    assert set(capi.SIGNATURES) | {"to_last_error"} == names


def test_no_cpu_fallback(built):
    L = capi.lib()
    n = C.c_int(-1)
    assert L.to_device_count(C.byref(n)) == 0
    if n.value == 0:
        assert L.to_init(0) != 0
        assert b"no CPU fallback" in L.to_last_error()
        t = capi.c_tensor()
        d = (C.c_int64 * 1)(4)
        assert L.to_alloc(0, 1, d, 0, C.byref(t)) != 0  # not initialised -> loud error


def test_route_query_refuses_before_init(built):
    """The debug query of the routing decision reads state to_init sets (the placement probe): TO_ERR_STATE without it, and
    its outputs untouched.  In a process of its own, which has not initialised the library whatever this one has done."""
    import sys
    code = ("import ctypes as C; from tensor_ops_amd import capi; L = capi.lib(); fam = (C.c_int * 4)(); "
            "out = [C.c_int(-7) for _ in range(4)]; "
            "st = L.to_gemm_route_query(0, 64, 64, 64, 1, 0, 0, 0, 0, 4, fam, *[C.byref(o) for o in out]); "
            "print(st, [o.value for o in out], L.to_last_error().decode())")
    got = subprocess.check_output([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert got.decode().startswith("4 [-7, -7, -7, -7] ") and "to_init" in got.decode(), got   # 4: TO_ERR_STATE


def test_ewise_route_query_refuses_before_init(built):
    """The elementwise routing query launches nothing and reads no device state, but it is part of the library's debug
    surface like the contraction query: TO_ERR_STATE before to_init, outputs untouched."""
    import sys
    code = ("import ctypes as C; from tensor_ops_amd import capi; L = capi.lib(); "
            "form, blocks, second = C.c_int(-7), C.c_int64(-7), C.c_int(-7); "
            "st = L.to_ewise_route_query(0, 1, 1024, 1, None, 0, C.byref(form), C.byref(blocks), C.byref(second)); "
            "print(st, [form.value, blocks.value, second.value], L.to_last_error().decode())")
    got = subprocess.check_output([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert got.decode().startswith("4 [-7, -7, -7] ") and "to_init" in got.decode(), got   # 4: TO_ERR_STATE


def test_persist_plan_query_refuses_before_init(built):
    """The plan query of the two persistent kernels reports the placement probe's verdict, which needs a device:
    TO_ERR_STATE before to_init, outputs untouched."""
    import sys
    code = ("import ctypes as C; from tensor_ops_amd import capi; L = capi.lib(); dims = (C.c_int64 * 8)(784, 300, 100, 10); "
            "i = [C.c_int(-7) for _ in range(4)]; lds, grid, ok = C.c_int64(-7), C.c_int64(-7), C.c_int(-7); "
            "st = L.to_persist_plan_query(0, 0, 3, dims, 1, 1, *[C.byref(o) for o in i], C.byref(lds), C.byref(grid), C.byref(ok)); "
            "print(st, [o.value for o in i] + [lds.value, grid.value, ok.value], L.to_last_error().decode())")
    got = subprocess.check_output([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert got.decode().startswith("4 [-7, -7, -7, -7, -7, -7, -7] ") and "to_init" in got.decode(), got   # 4: TO_ERR_STATE


def test_kernels_are_gfx950(built):
    """The shared object carries gfx950 code objects only (no other arch, no generic fallback)."""
    blob = open(built, "rb").read()
    targets = set(re.findall(rb"hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob))
    assert targets == {b"gfx950"}, targets
