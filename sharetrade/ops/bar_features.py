"""Host bindings of ``csrc/bar_features.hip``: raw OHLCV minute bars -> the GRU(256) policy's feature rows
(whole histories, one bar per session) and the synthetic generator that also writes the OHLCV planes."""
from __future__ import annotations

import ctypes as C

from . import native

NF, NSTATE = 8, 8
STATE_FIELDS = ("prev_close", "r1", "r2", "r3", "r4", "var", "sigma", "vol_scale")
STATE_COL = {n: i for i, n in enumerate(STATE_FIELDS)}
# st_bar_features_launch variants: the tiled kernel from 64 series on, one thread per series, the tiled kernel
AUTO, NAIVE, TILED = 0, 1, 2
TILE_SERIES = 64


class BarFeaturesArgs(C.Structure):
    """``BarFeatures``: N series of T bars, five fp32 planes and an int16 minute plane [N, T]."""
    _fields_ = [("open", C.c_void_p), ("high", C.c_void_p), ("low", C.c_void_p), ("close_in", C.c_void_p),
                ("volume", C.c_void_p), ("minute", C.c_void_p), ("state_in", C.c_void_p), ("feat", C.c_void_p),
                ("close", C.c_void_p), ("state_out", C.c_void_p), ("feat32", C.c_void_p),
                ("N", C.c_int), ("T", C.c_int), ("day", C.c_int), ("alpha", C.c_float), ("beta", C.c_float)]


class BarSessionsArgs(C.Structure):
    """``BarSessions``: B request rows, one raw bar each, on a table of S feature-state rows."""
    _fields_ = [("slot", C.c_void_p), ("ohlcv", C.c_void_p), ("minute", C.c_void_p), ("state", C.c_void_p),
                ("feat", C.c_void_p), ("close", C.c_void_p), ("B", C.c_int), ("S", C.c_int), ("day", C.c_int),
                ("alpha", C.c_float), ("beta", C.c_float)]


class MinuteBarsOhlcvArgs(C.Structure):
    """``MinuteBarsOhlcv``: ``ops.gru.MinuteBarsArgs`` plus the open / high / low / volume planes."""
    _fields_ = [("close", C.c_void_p), ("feat", C.c_void_p), ("open", C.c_void_p), ("high", C.c_void_p),
                ("low", C.c_void_p), ("volume", C.c_void_p), ("E", C.c_int), ("T", C.c_int), ("day", C.c_int),
                ("sigma", C.c_float), ("phi", C.c_float), ("alpha", C.c_float), ("beta", C.c_float),
                ("p0", C.c_float), ("key0", C.c_uint32), ("key1", C.c_uint32)]


def lib():
    L = native.lib()
    if not getattr(L, "_barf_bound", False):
        vp, i = C.c_void_p, C.c_int
        for fn, args in (("st_bar_features_launch", [C.POINTER(BarFeaturesArgs), i, vp]),
                         ("st_bar_features_sessions", [C.POINTER(BarSessionsArgs), vp]),
                         ("st_minute_bars_ohlcv", [C.POINTER(MinuteBarsOhlcvArgs), vp]),
                         ("st_abi_bar_features", [C.POINTER(C.c_int), i])):
            f = getattr(L, fn)
            f.argtypes = args
            f.restype = C.c_int
        L.st_bar_features_lds_bytes.restype = C.c_int
        L._barf_bound = True
    return L
