"""The ctypes mirror of the ledger rollout's launch struct (``GruRolloutLedger`` of ``csrc/gru_rollout.hip``: a
``GruRollout`` followed by the ledger pointers) matches the C++ struct's size, and the plain struct is what it was
(CPU: the HIP library is only loaded, no HIP call is made)."""
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


def test_ledger_struct_matches(lib):
    from sharetrade.ops.gru import LedgerOut, RolloutArgs, RolloutLedgerArgs

    assert _sizes(lib, "st_abi_gru_rollout_ledger") == [C.sizeof(RolloutLedgerArgs), C.sizeof(LedgerOut)]
    # 7 pointers and 2 ints behind the plain struct, which starts the ledger struct
    assert C.sizeof(LedgerOut) == 7 * 8 + 2 * 4
    assert C.sizeof(RolloutLedgerArgs) == C.sizeof(RolloutArgs) + C.sizeof(LedgerOut)
    assert RolloutLedgerArgs.r.offset == 0 and RolloutLedgerArgs.l.offset == C.sizeof(RolloutArgs)


def test_plain_rollout_struct_is_unchanged(lib):
    from sharetrade.ops.gru import RolloutArgs

    assert _sizes(lib, "st_abi_gru_rollout") == [C.sizeof(RolloutArgs)] == [20 * 8 + 12 * 4]
    assert [n for n, _ in RolloutArgs._fields_][-3:] == ["key0", "key1", "env_offset"]


def test_ledger_exports_are_bound(lib):
    from sharetrade.ops import gru as G

    L = G.lib()
    assert L.st_gru_rollout_ledger_launch.argtypes[0] == C.POINTER(G.RolloutLedgerArgs)
    assert G.LEDGER_STATE_COLS[:4] == ("cum", "peak", "trip", "ep") and len(G.LEDGER_STATS_COLS) == 7
