"""The ctypes mirrors of the two backtest kernels' launch structs match the C++ structs' sizes (CPU: the HIP
library is only loaded, no HIP call is made)."""
import ctypes as C

import pytest

from sharetrade.ops import native


@pytest.fixture(scope="module")
def lib():
    import build

    build.build_all()
    return native.lib()


def _sizes(lib, fn_name):
    fn = getattr(lib, fn_name)
    fn.argtypes, fn.restype = [C.POINTER(C.c_int), C.c_int], C.c_int
    n = fn(None, 0)
    out = (C.c_int * n)()
    assert fn(out, n) == n
    return list(out)


def test_gru_rollout_struct_matches(lib):
    from sharetrade.ops.gru import RolloutArgs

    assert _sizes(lib, "st_abi_gru_rollout") == [C.sizeof(RolloutArgs)]
    # 20 pointers, 6 ints, 3 floats, 3 words
    assert C.sizeof(RolloutArgs) == 20 * 8 + 12 * 4


def test_qrollout_struct_matches(lib):
    from sharetrade.serve.rollout import RolloutParams

    assert _sizes(lib, "st_abi_qrollout") == [C.sizeof(RolloutParams)]


def test_gru_rollout_exports(lib):
    from sharetrade.ops import gru as G

    L = G.lib()
    assert 0 < L.st_gru_rollout_lds_bytes() <= 160 * 1024
    assert L.st_gru_rollout_block() >= 0
