"""The ctypes mirrors of the launch structs of ``csrc/bar_features.hip`` match the C++ structs' sizes (CPU: the HIP
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


def test_bar_features_structs_match(lib):
    from sharetrade.ops.bar_features import BarFeaturesArgs, BarSessionsArgs, MinuteBarsOhlcvArgs

    assert _sizes(lib, "st_abi_bar_features") == [C.sizeof(BarFeaturesArgs), C.sizeof(BarSessionsArgs),
                                                  C.sizeof(MinuteBarsOhlcvArgs)]
    # 11 pointers, 3 ints, 2 floats (padded to 8); 6 pointers, 3 ints, 2 floats (padded); 6 pointers, 3 ints,
    # 5 floats, 2 words
    assert C.sizeof(BarFeaturesArgs) == 11 * 8 + 6 * 4
    assert C.sizeof(BarSessionsArgs) == 6 * 8 + 6 * 4
    assert C.sizeof(MinuteBarsOhlcvArgs) == 6 * 8 + 10 * 4


def test_bar_features_exports(lib):
    from sharetrade.ops import bar_features as BF

    L = BF.lib()
    # one tile of the whole-history kernel: 7 planes of [64 series][65] dwords, within the 160 KiB of a CU
    assert L.st_bar_features_lds_bytes() == 7 * 64 * 65 * 4 <= 160 * 1024
    assert len(BF.STATE_FIELDS) == BF.NSTATE == 8 and BF.TILE_SERIES == 64
