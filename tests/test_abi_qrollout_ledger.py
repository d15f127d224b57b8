"""The ctypes mirrors of the ledger rollout's launch structs (``RolloutLedger`` of ``csrc/qrollout.hip``: a
``RolloutParams`` followed by ``LedgerOut``) match the C++ structs' sizes, and the plain struct is what it was
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


def test_ledger_structs_match(lib):
    from sharetrade.serve.rollout import LedgerOut, RolloutLedger, RolloutParams

    assert _sizes(lib, "st_abi_qrollout_ledger") == [C.sizeof(RolloutLedger), C.sizeof(LedgerOut)]
    # 4 pointers, the stride and a pad behind the plain struct, which starts the ledger struct
    assert C.sizeof(LedgerOut) == 4 * 8 + 2 * 4
    assert C.sizeof(RolloutLedger) == C.sizeof(RolloutParams) + C.sizeof(LedgerOut)
    assert RolloutLedger.r.offset == 0 and RolloutLedger.l.offset == C.sizeof(RolloutParams)


def test_plain_rollout_struct_is_unchanged(lib):
    from sharetrade.serve.rollout import RolloutParams

    assert _sizes(lib, "st_abi_qrollout") == [C.sizeof(RolloutParams)] == [13 * 8 + 22 * 4]
    assert [n for n, _ in RolloutParams._fields_][-3:] == ["key0", "key1", "env_offset"]


def test_ledger_exports_are_bound_and_the_record_has_24_words(lib):
    from sharetrade.serve import rollout as R

    L = R._lib()
    assert L.st_qrollout_ledger_launch.argtypes[0] == C.POINTER(R.RolloutLedger)
    assert len(R.LEDGER_F32) + len(R.LEDGER_I32) + 1 + 2 * len(R.LEDGER_I64) == R.LEDGER_WORDS == 24
    assert R.LEDGER_F32[:3] == ("eq_prev", "eq0", "v0") and R.LEDGER_I64 == ("sum_s", "sum_s2")
