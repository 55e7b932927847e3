"""to_autoencoder_online_plan_query before to_init (no device needed)."""
import os
import subprocess
import sys

from test_cabi_symbols import built  # noqa: F401  (the library, built once)


def test_autoencoder_online_plan_query_refuses_before_init(built):  # noqa: F811
    """The plan query of the persistent autoencoder kernel reports the placement probe's verdict, which needs a device:
    TO_ERR_STATE before to_init, outputs untouched."""
    code = ("import ctypes as C; from tensor_ops_amd import capi; L = capi.lib(); dims = (C.c_int64 * 8)(784, 64, 784); "
            "i = [C.c_int(-7) for _ in range(4)]; lds, grid, ok = C.c_int64(-7), C.c_int64(-7), C.c_int(-7); "
            "st = L.to_autoencoder_online_plan_query(0, 2, dims, *[C.byref(o) for o in i], C.byref(lds), C.byref(grid), C.byref(ok)); "
            "print(st, [o.value for o in i] + [lds.value, grid.value, ok.value], L.to_last_error().decode())")
    got = subprocess.check_output([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert got.decode().startswith("4 [-7, -7, -7, -7, -7, -7, -7] ") and "to_init" in got.decode(), got   # 4: TO_ERR_STATE
