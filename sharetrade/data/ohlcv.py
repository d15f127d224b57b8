"""Raw OHLCV minute bars for the GRU(256) policy: loading, the bar -> 8-feature definition, training windows.

The policy's input row is eight features of a minute bar (``data.minute_bars``).  Seven of them are functions of the
bar and the few bars before it; the eighth is the synthetic generator's *latent* volatility ``sig``, which no client
can observe.  Here the row is defined from what a client does observe -- open, high, low, close, volume and the
bar's index within its session -- by replaying the bar through a GARCH(1,1) *filter*: the generator's variance
recursion driven by the observed return instead of the drawn one.  On the generator's own bars the filter recovers
the generator's features (``sig`` to ~2e-5 relative, the return to the float32 rounding of the stored close, the
other five bit for bit), so a net trained on the synthetic bank sees the rows it was trained on.

The definition is causal and carries a 32-byte state per series (``ops.bar_features.STATE_FIELDS``), so it exists
in three forms that agree: :func:`featurise_gpu` (``csrc/bar_features.hip``, whole histories),
``GruSessionServer.step_raw`` (one bar per session) and :func:`featurise_numpy`, the host reference with the
kernel's operation order (``dtype=np.float64``: the accuracy yardstick).  A history featurised in pieces with the
carried state equals the whole bit for bit.

Per bar, with ``minute`` = index within the session (0 .. day - 1) and the series' fitted ``sigma`` / ``vol_scale``::

    ref  = open if minute == 0 or no bar yet else previous close      (no overnight gap enters a return)
    ush  = 1 + 0.8 x^2,  x = 2 minute / day - 1                       (intraday U-shape)
    sig  = sqrt(var) * ush                                            (before var advances)
    ret  = log(close / ref);  dsr = ret / ush
    var' = sigma^2 (1 - alpha - beta) + alpha dsr^2 + beta var        (var starts at sigma^2)
    mom  = ret + the previous four returns
    row  = ret %, (h - l) / c %, (c - l) / max(h - l, 1e-12) - 0.5, log(max(v / vol_scale, 1e-6)),
           sin / cos(2 pi minute / day), mom %, sig %
"""
from __future__ import annotations

import datetime as _dt
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import bar_features as BF
from ..utils import rng
from . import minute_bars as mb

PLANES = ("open", "high", "low", "close", "volume")


@dataclass
class Bars:
    """N series of T raw bars: five [N, T] planes (numpy, or torch tensors on a device), ``minute`` [N, T] or
    [T] (None: ``t % day``) and the series' names."""
    open: object
    high: object
    low: object
    close: object
    volume: object
    minute: Optional[np.ndarray] = None
    names: Optional[List[str]] = None

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.close.shape[0]), int(self.close.shape[1])

    def minutes(self, day: int) -> np.ndarray:
        """``minute`` as an int64 [N, T] array (``t % day`` when the bars carry none)."""
        N, T = self.shape
        m = np.arange(T, dtype=np.int64) % int(day) if self.minute is None else np.asarray(self.minute, np.int64)
        return np.ascontiguousarray(np.broadcast_to(m, (N, T)))

    def piece(self, a: int, b: int) -> "Bars":
        """Bars a .. b - 1 of every series."""
        day_m = None if self.minute is None else np.asarray(self.minute)[..., a:b]
        return Bars(*(getattr(self, k)[:, a:b] for k in PLANES), minute=day_m, names=self.names)

    def names_or_default(self) -> List[str]:
        return list(self.names) if self.names is not None else [f"series{i}" for i in range(self.shape[0])]


@dataclass
class FeatureParams:
    """What the definition needs beside the bars: the session length, the GARCH coefficients and, per series, the
    long-run per-bar volatility and the volume unit."""
    day: int
    alpha: float
    beta: float
    sigma: np.ndarray       # [N] float32
    vol_scale: np.ndarray   # [N] float32

    def __post_init__(self):
        self.day, self.alpha, self.beta = int(self.day), float(self.alpha), float(self.beta)
        self.sigma = np.atleast_1d(np.asarray(self.sigma, dtype=np.float32))
        self.vol_scale = np.atleast_1d(np.asarray(self.vol_scale, dtype=np.float32))
        if self.day < 1 or self.sigma.shape != self.vol_scale.shape or self.sigma.ndim != 1:
            raise ValueError("need day >= 1 and one sigma and one vol_scale per series")
        if not (np.all(self.sigma > 0) and np.all(self.vol_scale > 0)):
            raise ValueError("sigma and vol_scale must be positive")

    def initial_state(self) -> np.ndarray:
        """[N, 8] float32: no bar yet (``prev_close == 0``; the variance then starts at ``sigma^2``)."""
        st = np.zeros((self.sigma.shape[0], BF.NSTATE), np.float32)
        st[:, BF.STATE_COL["sigma"]] = self.sigma
        st[:, BF.STATE_COL["vol_scale"]] = self.vol_scale
        return st

    def to_meta(self, names: Sequence[str]) -> dict:
        return {"day": self.day, "alpha": self.alpha, "beta": self.beta, "names": list(names),
                "sigma": [float(x) for x in self.sigma], "vol_scale": [float(x) for x in self.vol_scale]}

    @classmethod
    def from_meta(cls, m: dict) -> "FeatureParams":
        return cls(m["day"], m["alpha"], m["beta"], m["sigma"], m["vol_scale"])


class Featurised(NamedTuple):
    close: object    # [N, T] fp32
    feat: object     # [N, T, 8]: the reference's dtype; bf16 on the GPU
    state: object    # [N, 8] fp32, to carry into the next piece
    feat32: object = None   # [N, T, 8] fp32 of the GPU form (tests), else None


# ---------------------------------------------------------------------------- loading
def _parse_minute_rows(lines) -> Tuple[List[_dt.datetime], np.ndarray]:
    rows = {}
    for line in lines:
        fields = [x.strip() for x in line.rstrip("\n").split(",")]
        if len(fields) < 6:
            continue
        try:
            ts = _dt.datetime.strptime(fields[0], "%Y-%m-%d %H:%M")
            vals = [float(x) for x in fields[1:6]]
        except ValueError:
            continue
        if not all(np.isfinite(vals)) or min(vals[:4]) <= 0.0 or vals[4] < 0.0:
            continue
        rows[ts] = vals   # a later duplicate of a timestamp wins
    stamps = sorted(rows)
    return stamps, np.asarray([rows[s] for s in stamps], dtype=np.float32).reshape(len(stamps), 5)


def load_bars(path: str, day: int = 390) -> Bars:
    """``.npz``: ``open, high, low, close, volume`` [N, T], optionally ``minute`` ([N, T] or [T]) and ``names``.
    ``.csv``: one series of ``yyyy-MM-dd HH:mm,open,high,low,close,volume`` rows in time order; a row that does not
    parse or holds a non-positive price is dropped (as ``data.prices`` drops rows), and ``minute`` is the row's
    index within its calendar date.  Without ``minute`` in an npz it is ``t % day``."""
    if path.endswith(".npz"):
        z = np.load(path)          # arrays only (allow_pickle stays False)
        planes = [np.ascontiguousarray(np.atleast_2d(z[k]), dtype=np.float32) for k in PLANES]
        if any(p.shape != planes[0].shape or p.ndim != 2 for p in planes):
            raise ValueError(f"{path}: the five planes must share one [N, T] shape")
        N, T = planes[0].shape
        minute = np.asarray(z["minute"], np.int64) if "minute" in z.files else np.arange(T, dtype=np.int64) % int(day)
        if minute.shape not in ((N, T), (T,)):
            raise ValueError(f"{path}: minute must be [N, T] or [T]")
        names = [str(x) for x in z["names"]] if "names" in z.files else None
        if names is not None and len(names) != N:
            raise ValueError(f"{path}: one name per series")
        return Bars(*planes, minute=minute, names=names)
    with open(path, "r", encoding="utf-8") as f:
        stamps, vals = _parse_minute_rows(f)
    if not stamps:
        raise ValueError(f"{path}: no bar parsed")
    minute = np.zeros(len(stamps), np.int64)
    for i in range(1, len(stamps)):
        minute[i] = minute[i - 1] + 1 if stamps[i].date() == stamps[i - 1].date() else 0
    import os

    return Bars(*(np.ascontiguousarray(vals[None, :, k]) for k in range(5)), minute=minute,
                names=[os.path.splitext(os.path.basename(path))[0]])


def save_bars(path: str, bars: Bars) -> None:
    """Write ``bars`` as the ``.npz`` :func:`load_bars` reads."""
    d = {k: np.asarray(getattr(bars, k), np.float32) for k in PLANES}
    if bars.minute is not None:
        d["minute"] = np.asarray(bars.minute, np.int64)
    if bars.names is not None:
        d["names"] = np.asarray(list(bars.names))
    np.savez(path, **d)


def file_crc32c(path: str) -> int:
    """CRC32C of a bars file (the runtime's, ``persist.native``): what a checkpoint records of its bars."""
    from ..persist import native as pn

    with open(path, "rb") as f:
        return int(pn.crc32c(f.read()))


# ---------------------------------------------------------------------------- the parameters
def _ushape(minute: np.ndarray, day: int) -> np.ndarray:
    x = 2.0 * minute.astype(np.float64) / float(day) - 1.0
    return 1.0 + 0.8 * x * x


def fit_feature_params(bars: Bars, upto: Optional[int] = None, day: Optional[int] = None,
                       alpha: float = mb.BarParams.alpha, beta: float = mb.BarParams.beta) -> FeatureParams:
    """Per series, from bars ``< upto`` only (default: all): ``sigma = sqrt(mean(dsr^2))`` of the de-seasonalised
    log return and ``vol_scale = exp(mean(log(volume / ush)))``.  ``day`` defaults to the longest session of those
    bars.  ``alpha`` / ``beta`` are not fitted."""
    N, T = bars.shape
    upto = T if upto is None else int(upto)
    if not 1 <= upto <= T:
        raise ValueError(f"upto must be 1 .. {T}")
    m_all = bars.minutes(day if day is not None else mb.BarParams.day)[:, :upto]
    day = int(m_all.max()) + 1 if day is None else int(day)
    o, c, v = (np.asarray(getattr(bars, k), np.float64)[:, :upto] for k in ("open", "close", "volume"))
    ref = o.copy()
    carry = m_all[:, 1:] != 0
    ref[:, 1:][carry] = c[:, :-1][carry]
    ush = _ushape(m_all, day)
    dsr = np.log(c / ref) / ush
    sigma = np.sqrt(np.mean(dsr * dsr, axis=1))
    vol_scale = np.exp(np.mean(np.log(np.maximum(v, 1e-12) / ush), axis=1))
    return FeatureParams(day, alpha, beta, np.maximum(sigma, 1e-12), vol_scale)


# ---------------------------------------------------------------------------- the definition on the host
def featurise_numpy(bars: Bars, fp: FeatureParams, state: Optional[np.ndarray] = None,
                    dtype=np.float32) -> Featurised:
    """The host reference of ``csrc/bar_features.h``: the same operations in the same order in ``dtype``
    (float32: the kernel's arithmetic up to the transcendental functions' ulps; float64: the accuracy yardstick,
    with the kernel's float32 constants and inputs).  ``state`` [N, 8] continues an earlier piece."""
    f = np.dtype(dtype).type
    k = lambda v: f(np.float32(v))   # noqa: E731 -- the kernel's float32 literals, exactly
    N, T = bars.shape
    if fp.sigma.shape[0] != N:
        raise ValueError(f"{N} series, parameters of {fp.sigma.shape[0]}")
    st = fp.initial_state() if state is None else np.asarray(state, np.float32)
    if st.shape != (N, BF.NSTATE):
        raise ValueError(f"state must be [{N}, {BF.NSTATE}]")
    O, H, L, Cl, V = (np.asarray(getattr(bars, p), np.float32) for p in PLANES)
    M = bars.minutes(fp.day)
    prev, r1, r2, r3, r4, var, sigma, vs = (st[:, i].astype(dtype) for i in range(BF.NSTATE))
    alpha, beta, dayf = k(fp.alpha), k(fp.beta), f(fp.day)
    omega = sigma * sigma * (f(1) - alpha - beta)
    twopi, c08, c100, half = k(6.2831853), k(0.8), f(100), f(0.5)
    feat = np.zeros((N, T, BF.NF), dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            o, h, l, c, v = (np.ascontiguousarray(P[:, t]).astype(dtype) for P in (O, H, L, Cl, V))
            m = M[:, t]
            mf = m.astype(dtype)
            first = prev == 0
            ref = np.where((m == 0) | first, o, prev)
            var = np.where(first, sigma * sigma, var)
            x = f(2) * mf / dayf - f(1)
            ush = f(1) + c08 * x * x
            sig = np.sqrt(var).astype(dtype) * ush
            ret = np.log(c / ref).astype(dtype)
            dsr = ret / ush
            var = omega + alpha * dsr * dsr + beta * var
            mom = ret + r1 + r2 + r3 + r4
            r4, r3, r2, r1 = r3, r2, r1, ret
            prev = c
            ang = twopi * mf / dayf
            feat[:, t, 0] = ret * c100
            feat[:, t, 1] = (h - l) / c * c100
            feat[:, t, 2] = (c - l) / np.maximum(h - l, k(1e-12)) - half
            feat[:, t, 3] = np.log(np.maximum(v / vs, k(1e-6)))
            feat[:, t, 4] = np.sin(ang)
            feat[:, t, 5] = np.cos(ang)
            feat[:, t, 6] = mom * c100
            feat[:, t, 7] = sig * c100
    out = np.stack([prev, r1, r2, r3, r4, var, sigma, vs], axis=1).astype(np.float32)
    return Featurised(np.ascontiguousarray(Cl), feat, out)


# ---------------------------------------------------------------------------- the definition on the GPU
def featurise_gpu(bars: Bars, fp: FeatureParams, device: torch.device, state=None, want32: bool = False,
                  variant: int = BF.AUTO) -> Featurised:
    """``csrc/bar_features.hip`` on N series of T bars: ``close`` fp32 [N, T], ``feat`` bf16 [N, T, 8] and the
    carried ``state`` [N, 8] on ``device`` (``want32``: also the unrounded rows, fp32).  ``variant``:
    ``ops.bar_features.AUTO`` (the tiled kernel from 64 series on), ``NAIVE`` or ``TILED``."""
    from ..ops import native

    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("featurise_gpu runs on the GPU (host form: featurise_numpy)")
    N, T = bars.shape
    if fp.sigma.shape[0] != N:
        raise ValueError(f"{N} series, parameters of {fp.sigma.shape[0]}")
    if fp.day > 32767:
        raise ValueError("the minute plane is int16: day must be below 32768")
    f32 = torch.float32
    planes = [torch.as_tensor(getattr(bars, p)).to(device, f32).contiguous() for p in PLANES]
    minute = torch.from_numpy(bars.minutes(fp.day).astype(np.int16)).to(device)
    st_in = torch.as_tensor(fp.initial_state() if state is None else state).to(device, f32).contiguous()
    if tuple(st_in.shape) != (N, BF.NSTATE):
        raise ValueError(f"state must be [{N}, {BF.NSTATE}]")
    with torch.cuda.device(device):
        close = torch.empty(N, T, dtype=f32, device=device)
        feat = torch.empty(N, T, BF.NF, dtype=torch.bfloat16, device=device)
        st_out = torch.empty(N, BF.NSTATE, dtype=f32, device=device)
        feat32 = torch.empty(N, T, BF.NF, dtype=f32, device=device) if want32 else None
        a = BF.BarFeaturesArgs()
        a.open, a.high, a.low, a.close_in, a.volume = (p.data_ptr() for p in planes)
        a.minute, a.state_in = minute.data_ptr(), st_in.data_ptr()
        a.feat, a.close, a.state_out = feat.data_ptr(), close.data_ptr(), st_out.data_ptr()
        a.feat32 = native.ptr(feat32)
        a.N, a.T, a.day, a.alpha, a.beta = N, T, fp.day, fp.alpha, fp.beta
        native.check(BF.lib().st_bar_features_launch(a, int(variant), native.stream_handle()),
                     "st_bar_features_launch")
    return Featurised(close, feat, st_out, feat32)


# ---------------------------------------------------------------------------- synthetic bars with their OHLCV
def generate_ohlcv_numpy(E: int, T: int, bp: mb.BarParams = mb.BarParams(), seed: int = 0) -> Tuple[Bars, np.ndarray]:
    """``minute_bars.generate_numpy`` with the bars themselves: (:class:`Bars`, feat [E, T, 8] float32); ``close``
    and ``feat`` are ``generate_numpy``'s."""
    ohlv: dict = {}
    close, feat = mb._generate_numpy(E, T, bp, seed, ohlv)
    return Bars(ohlv["open"], ohlv["high"], ohlv["low"], close, ohlv["volume"],
                minute=np.arange(T, dtype=np.int64) % bp.day), feat


def generate_ohlcv_gpu(E: int, T: int, device: torch.device, bp: mb.BarParams = mb.BarParams(),
                       seed: int = 0) -> Tuple[Bars, torch.Tensor]:
    """``minute_bars.generate_gpu`` with the bars themselves (``csrc/bar_features.hip`` minute_bars_ohlcv_kernel:
    same Philox counters): (:class:`Bars` of fp32 device tensors, feat bf16 [E, T, 8])."""
    from ..ops import native

    f32 = torch.float32
    with torch.cuda.device(device):
        pl = {k: torch.empty(E, T, dtype=f32, device=device) for k in PLANES}
        feat = torch.empty(E, T, BF.NF, dtype=torch.bfloat16, device=device)
        k0, k1 = (int(x) for x in rng.key_for(seed, 0))
        a = BF.MinuteBarsOhlcvArgs(pl["close"].data_ptr(), feat.data_ptr(), pl["open"].data_ptr(),
                                   pl["high"].data_ptr(), pl["low"].data_ptr(), pl["volume"].data_ptr(), E, T, bp.day,
                                   bp.sigma, bp.phi, bp.alpha, bp.beta, bp.p0, k0, k1)
        native.check(BF.lib().st_minute_bars_ohlcv(a, native.stream_handle()), "st_minute_bars_ohlcv")
    return Bars(*(pl[k] for k in PLANES), minute=np.arange(T, dtype=np.int64) % bp.day), feat


def true_params(E: int, bp: mb.BarParams = mb.BarParams()) -> FeatureParams:
    """The generator's own parameters as :class:`FeatureParams` (``vol_scale = 1``)."""
    return FeatureParams(bp.day, bp.alpha, bp.beta, np.full(E, bp.sigma, np.float32), np.ones(E, np.float32))


# ---------------------------------------------------------------------------- training windows
def window_bank(close: torch.Tensor, feat: torch.Tensor, E: int, T: int, seed: int = 0):
    """A learner's bank cut from N featurised series of L bars: env ``e`` takes ``T`` consecutive bars of series
    ``e % N`` from a start drawn from ``np.random.default_rng(seed)``.  Returns (``close`` fp32 [E, T], ``feat``
    [E, T, 8]) on the inputs' device; the bank holds ``E * T * 24`` bytes with bf16 features (4 of close, 16 of
    features, and 4 of the per-bar returns the learner derives from close).  Raises when ``L < T``."""
    if close.dim() != 2 or feat.dim() != 3 or feat.shape[:2] != close.shape or feat.shape[2] != BF.NF:
        raise ValueError("close must be [N, L] and feat [N, L, 8]")
    N, L = (int(v) for v in close.shape)
    E, T = int(E), int(T)
    if L < T:
        raise ValueError(f"the series hold {L} bars, a window needs {T}")
    g = np.random.default_rng(seed)
    start = torch.from_numpy(g.integers(0, L - T + 1, size=E).astype(np.int64)).to(close.device)
    series = (torch.arange(E, device=close.device) % N)[:, None]
    idx = start[:, None] + torch.arange(T, device=close.device)[None, :]
    return close[series, idx].contiguous(), feat[series, idx].contiguous()
