"""Backtesting a frozen policy: whole episodes in one launch (``csrc/qrollout.hip``) and their PyTorch oracle.

"What would this policy have done over this price history?"  For env ``e`` and day ``t = start ..
start + steps - 1`` the rule is the engine's: window ``prices[e, t : t+H]`` -> features -> Q-net -> argmax ->
epsilon-greedy (Philox stream 4 over ``(env_offset + e, t)``, exploit ramp on the day ``t``) -> Buy / Sell /
Hold at ``prices[e, t+H]``.  The kernel owns an env for the whole episode (weights and env state on chip,
each price read from HBM once); :func:`reference_rollout` is the same computation day by day in PyTorch
(``tr.features``, ``qn.forward``, ``tr.env_transition``): the numerics oracle of
``tests/test_gpu_backtest.py`` and the CPU backend of :meth:`PolicyServer.backtest`.

An episode can be run in pieces: pass a piece's final ``budget`` / ``shares`` and the next ``start`` to the
following call; the pieces reproduce the whole episode bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..env import trading as tr
from ..models import qnet as qn
from ..ops import native
from ..utils import rng
from .kernel import epsilon_greedy, fill_net_params

ROLLOUT_STREAM = 4        # Philox counter word 3 of the backtest draws: (env, day_lo, day_hi, 4)


class RolloutParams(C.Structure):
    _fields_ = [
        ("prices", C.c_void_p), ("wq", C.c_void_p), ("wf", C.c_void_p),
        ("budget", C.c_void_p), ("shares", C.c_void_p),
        ("out_budget", C.c_void_p), ("out_shares", C.c_void_p), ("out_portfolio", C.c_void_p),
        ("out_buys", C.c_void_p), ("out_sells", C.c_void_p),
        ("tr_actions", C.c_void_p), ("tr_q", C.c_void_p), ("tr_equity", C.c_void_p),
        ("E", C.c_int), ("ld", C.c_int), ("T", C.c_int), ("H", C.c_int), ("start", C.c_int), ("steps", C.c_int),
        ("off_w0", C.c_int), ("off_w1", C.c_int), ("off_b1", C.c_int), ("off_w2", C.c_int), ("off_b2", C.c_int),
        ("feat_mode", C.c_int), ("output_relu", C.c_int), ("compat_env", C.c_int),
        ("s0", C.c_int),
        ("b0", C.c_float), ("inv_b0", C.c_float), ("eps", C.c_float), ("inv_ramp", C.c_float),
        ("key0", C.c_uint32), ("key1", C.c_uint32), ("env_offset", C.c_uint32),
    ]


class LedgerOut(C.Structure):
    _fields_ = [("state_in", C.c_void_p), ("state_out", C.c_void_p), ("part", C.c_void_p), ("curve", C.c_void_p),
                ("part_stride", C.c_int), ("pad_", C.c_int)]


class RolloutLedger(C.Structure):
    _fields_ = [("r", RolloutParams), ("l", LedgerOut)]


# The ledger record of one env: 24 32-bit words (``struct LedgerOut`` of ``csrc/qrollout.hip``).  Words 0 .. 9 fp32,
# 10 .. 18 int32, 19 zero, 20 .. 23 two int64 (low word first).
LEDGER_WORDS = 24
LEDGER_F32 = ("eq_prev", "eq0", "v0", "v_last", "peak", "max_dd", "sumsq", "sum_d", "sum_d2", "sum_sd")
LEDGER_I32 = ("run", "dd_days", "days", "chose_buy", "chose_sell", "refused_buy", "refused_sell", "flat_days",
              "max_shares")
LEDGER_I64 = ("sum_s", "sum_s2")
LEDGER_FIELDS = LEDGER_F32 + LEDGER_I32 + LEDGER_I64
CHUNK = 16   # envs whose gains one wave sums per day (the kernel's 16-env tile)

_bound = False


def _lib() -> C.CDLL:
    global _bound
    L = native.lib()
    if not _bound:
        L.st_qrollout_launch.argtypes = [C.POINTER(RolloutParams), C.c_int, C.c_void_p]
        L.st_qrollout_launch.restype = C.c_int
        L.st_qrollout_lds_bytes.restype = C.c_int
        L.st_qrollout_day_block.restype = C.c_int
        L.st_qrollout_ledger_launch.argtypes = [C.POINTER(RolloutLedger), C.c_int, C.c_void_p]
        L.st_qrollout_ledger_launch.restype = C.c_int
        _bound = True
    return L


def day_block() -> int:
    """Days per price block of the kernel (episode lengths around its multiples take every loop path)."""
    return int(_lib().st_qrollout_day_block())


class RolloutKernel:
    """One reusable parameter block for ``st_qrollout_launch`` (weights by pointer: the caller keeps
    ``params`` / ``params_bf`` alive and may update them in place between launches)."""

    def __init__(self, layout: qn.QNetLayout, params: torch.Tensor, params_bf: torch.Tensor, *,
                 history: int, feat_mode: int, output_relu: bool, budget0: float, shares0: int, compat: bool,
                 epsilon: float, ramp: float, key: Tuple[int, int]):
        p = RolloutParams()
        fill_net_params(p, "rollout", layout, params, params_bf, history, feat_mode, output_relu, budget0, key)
        p.compat_env, p.b0, p.s0 = int(bool(compat)), float(budget0), int(shares0)
        self.p = p
        self.epsilon, self.inv_ramp = float(epsilon), float(np.float32(1.0 / ramp))
        self.device = params.device
        self._keep = (params, params_bf)

    def run(self, prices: torch.Tensor, *, T: Optional[int] = None, start: int = 0, steps: Optional[int] = None,
            budget: Optional[torch.Tensor] = None, shares: Optional[torch.Tensor] = None, greedy: bool = True,
            trace: bool = False, env_offset: int = 0, grid: int = 0, ledger: bool = False,
            ledger_state: Optional[torch.Tensor] = None, curve: bool = True) -> Dict[str, torch.Tensor]:
        """``prices`` [E, >= T] fp32 on the GPU (row stride = ``prices.stride(0)``, ``T`` valid values per row,
        default all); ``budget`` [E] fp32 / ``shares`` [E] int32 or None (the configured start).  One launch on
        the current stream; returns the per-env results (and the traces with ``trace``).

        ``ledger``: the kernel's ledger instance (``st_qrollout_ledger_launch``) also writes ``ledger_state``
        [E, 24] int32, the cumulative risk record of every env (:class:`QLedger`), and with ``curve`` the float64
        ``curve`` [steps] (one more small launch on the same stream).  ``ledger_state=`` [E, 24] int32 is the record
        of the piece before (with that piece's ``budget`` / ``shares``).  The curve needs a scratch buffer of
        ``ceil(E / 16) * part_stride * 4`` bytes, ``part_stride`` = steps rounded up to 32 (one fp32 per 16 envs and
        day: 96 MB at 65,536 envs and 5,846 days), freed after the launch."""
        if ledger_state is not None and not ledger:
            raise ValueError("ledger_state continues a ledger: pass ledger=True")
        if ledger and self.p.compat_env:
            raise ValueError("env.compat_decisions trades from the initial holding every day: it has no position "
                             "ledger")
        if prices.dim() != 2 or prices.dtype != torch.float32 or prices.stride(1) != 1 or not prices.is_cuda:
            raise ValueError("prices must be fp32 device rows [E, T], unit column stride")
        E = int(prices.shape[0])
        T = int(prices.shape[1] if T is None else T)
        H = self.p.H
        if T > prices.shape[1] or T < H + 1:
            raise ValueError(f"T = {T}: need H + 1 = {H + 1} <= T <= {prices.shape[1]} values per row")
        steps = T - H - int(start) if steps is None else int(steps)
        if start < 0 or steps < 1 or start + steps > T - H:
            raise ValueError(f"days start .. start + steps - 1 = {start} .. {start + steps - 1} outside 0 .. {T - H - 1}")
        dev = prices.device
        if budget is not None and (budget.dtype != torch.float32 or budget.numel() != E or not budget.is_contiguous()
                                   or budget.device != dev):
            raise ValueError("budget must be a contiguous fp32 device buffer of E entries")
        if shares is not None and (shares.dtype != torch.int32 or shares.numel() != E or not shares.is_contiguous()
                                   or shares.device != dev):
            raise ValueError("shares must be a contiguous int32 device buffer of E entries")
        out = {
            "budget": torch.empty(E, dtype=torch.float32, device=dev),
            "shares": torch.empty(E, dtype=torch.int32, device=dev),
            "portfolio": torch.empty(E, dtype=torch.float32, device=dev),
            "buys": torch.empty(E, dtype=torch.int32, device=dev),
            "sells": torch.empty(E, dtype=torch.int32, device=dev),
        }
        if trace:
            out["actions"] = torch.empty(E, steps, dtype=torch.int8, device=dev)
            out["q"] = torch.empty(E, steps, 3, dtype=torch.float32, device=dev)
            out["equity"] = torch.empty(E, steps, dtype=torch.float32, device=dev)
        p = self.p
        ld = int(prices.stride(0)) if E > 1 else T   # (a single row's stride is never used)
        if ld < T:
            raise ValueError("price rows overlap (row stride < T)")
        p.prices, p.ld, p.E, p.T = native.ptr(prices), ld, E, T
        p.start, p.steps = int(start), steps
        p.budget, p.shares = native.ptr(budget), native.ptr(shares)
        p.out_budget, p.out_shares, p.out_portfolio = (native.ptr(out[k]) for k in ("budget", "shares", "portfolio"))
        p.out_buys, p.out_sells = native.ptr(out["buys"]), native.ptr(out["sells"])
        p.tr_actions, p.tr_q, p.tr_equity = (native.ptr(out.get(k)) for k in ("actions", "q", "equity"))
        p.eps = math.inf if greedy else self.epsilon
        p.inv_ramp = math.inf if greedy else self.inv_ramp
        p.env_offset = int(env_offset) & 0xFFFFFFFF
        if not ledger:
            if E > 0:
                native.check(_lib().st_qrollout_launch(C.byref(p), int(grid), native.stream_handle()),
                             "st_qrollout_launch")
            return out
        if ledger_state is not None and (ledger_state.dtype != torch.int32 or ledger_state.device != dev or
                                         tuple(ledger_state.shape) != (E, LEDGER_WORDS) or
                                         not ledger_state.is_contiguous()):
            raise ValueError(f"ledger_state must be a contiguous int32 device tensor of shape {(E, LEDGER_WORDS)}")
        q = RolloutLedger()
        q.r = p
        out["ledger_state"] = torch.empty(E, LEDGER_WORDS, dtype=torch.int32, device=dev)
        q.l.state_in, q.l.state_out = native.ptr(ledger_state), native.ptr(out["ledger_state"])
        part = None
        if curve:
            q.l.part_stride = -(-steps // 32) * 32
            part = torch.empty(-(-E // CHUNK), q.l.part_stride, dtype=torch.float32, device=dev)
            out["curve"] = torch.empty(steps, dtype=torch.float64, device=dev)
            q.l.part, q.l.curve = native.ptr(part), native.ptr(out["curve"])
        if E > 0:
            native.check(_lib().st_qrollout_ledger_launch(C.byref(q), int(grid), native.stream_handle()),
                         "st_qrollout_ledger_launch")
        return out   # (part goes back to the allocator of the launch's stream: reuse is in stream order)


def reference_rollout(params: torch.Tensor, layout: qn.QNetLayout, prices: torch.Tensor, *, history: int,
                      feat_mode: str, output_relu: bool, budget0: float, shares0: int, compat: bool, epsilon: float,
                      ramp: float, key_seed: int, start: int = 0, steps: Optional[int] = None,
                      budget: Optional[torch.Tensor] = None, shares: Optional[torch.Tensor] = None,
                      env_offset: int = 0, forced_actions: Optional[torch.Tensor] = None,
                      emulate_bf16: bool = True) -> Dict[str, torch.Tensor]:
    """The rollout day by day in PyTorch, for price series [E, T] (CPU or GPU tensors).  Returns the kernel's
    fields: ``budget``, ``shares``, ``portfolio``, ``buys``, ``sells`` [E] and the traces ``actions`` int8
    [E, steps], ``q`` [E, steps, 3], ``equity`` [E, steps].  ``epsilon = inf`` is the greedy policy;
    ``forced_actions`` [E, steps] replaces the policy's choice (``q`` is still the net's)."""
    P = prices.float()
    E, T = P.shape
    H = int(history)
    steps = T - H - int(start) if steps is None else int(steps)
    if start < 0 or steps < 1 or start + steps > T - H:
        raise ValueError(f"days start .. start + steps - 1 = {start} .. {start + steps - 1} outside 0 .. {T - H - 1}")
    dev = P.device
    w = params.float().to(dev)
    b = torch.full((E,), float(budget0), dtype=torch.float32, device=dev) if budget is None else \
        budget.to(dev, torch.float32).clone()
    s = torch.full((E,), int(shares0), dtype=torch.int32, device=dev) if shares is None else \
        shares.to(dev, torch.int32).clone()
    buys = torch.zeros(E, dtype=torch.int32, device=dev)
    sells = torch.zeros(E, dtype=torch.int32, device=dev)
    actions = torch.empty(E, steps, dtype=torch.int8, device=dev)
    qs = torch.empty(E, steps, layout.n_actions, dtype=torch.float32, device=dev)
    equity = torch.empty(E, steps, dtype=torch.float32, device=dev)
    ids = (np.arange(E, dtype=np.uint64) + np.uint64(int(env_offset) & 0xFFFFFFFF)).astype(np.uint32)
    greedy_policy = math.isinf(epsilon)
    v = torch.zeros(E, dtype=torch.float32, device=dev)
    for i in range(steps):
        t = int(start) + i
        x = tr.features(P[:, t: t + H], b, s, feat_mode, budget0)
        q, _, _ = qn.forward(w, layout, x, output_relu, emulate_bf16=emulate_bf16)
        q = q[:, : layout.n_actions]
        a = torch.argmax(q, dim=1)   # first max on ties (TF ArgMax)
        if not greedy_policy:
            u1, u2 = rng.uniforms(key_seed, 0, ids, t, stream=ROLLOUT_STREAM)
            a = epsilon_greedy(a, u1, u2, epsilon, ramp, t)
        if forced_actions is not None:
            a = forced_actions[:, i].to(dev).long()
        v = P[:, t + H]
        sd = torch.full_like(s, int(shares0)) if compat else s
        b, s2, _ = tr.env_transition(a, b, s, v, v, compat, budget0, shares0)
        buys += (s2 > sd).int()
        sells += (s2 < sd).int()
        s = s2
        actions[:, i] = a.to(torch.int8)
        qs[:, i] = q
        equity[:, i] = b + s.float() * v
    return {"budget": b, "shares": s, "portfolio": b + s.float() * v, "buys": buys, "sells": sells,
            "actions": actions, "q": qs, "equity": equity}


def simulate_actions(prices: torch.Tensor, actions: torch.Tensor, *, history: int, budget0: float, shares0: int,
                     compat: bool, start: int = 0) -> Dict[str, torch.Tensor]:
    """The env alone under given ``actions`` [E, steps] (no net): the per-env fields of :func:`reference_rollout`
    and the equity trace, e.g. for the buy-and-hold (all Buy) and random baselines of a backtest."""
    P = prices.float()
    E, steps = actions.shape
    H = int(history)
    if start < 0 or steps < 1 or start + steps > P.shape[1] - H:
        raise ValueError(f"days {start} .. {start + steps - 1} outside 0 .. {P.shape[1] - H - 1}")
    dev = P.device
    b = torch.full((E,), float(budget0), dtype=torch.float32, device=dev)
    s = torch.full((E,), int(shares0), dtype=torch.int32, device=dev)
    buys = torch.zeros(E, dtype=torch.int32, device=dev)
    sells = torch.zeros(E, dtype=torch.int32, device=dev)
    equity = torch.empty(E, steps, dtype=torch.float32, device=dev)
    for i in range(steps):
        v = P[:, start + i + H]
        sd = torch.full_like(s, int(shares0)) if compat else s
        b, s2, _ = tr.env_transition(actions[:, i].to(dev).long(), b, s, v, v, compat, budget0, shares0)
        buys += (s2 > sd).int()
        sells += (s2 < sd).int()
        s = s2
        equity[:, i] = b + s.float() * v
    return {"budget": b, "shares": s, "portfolio": equity[:, -1].clone(), "buys": buys, "sells": sells,
            "equity": equity}


@dataclass
class QLedger:
    """The risk ledger of a run: what ``csrc/qrollout.hip``'s ledger instance keeps per series.

    ``state`` [E, 24] int32 holds one cumulative record per series (the ledger of the whole run so far, whatever
    pieces it was cut into) and is what the next piece takes as ``ledger_state=``.  Every name of
    ``LEDGER_FIELDS`` is an attribute: a view of its words as fp32 / int32 / int64 [E].  ``curve`` [steps]
    float64 is, per day of this piece, the sum over the series of ``eq - eq0``."""

    state: torch.Tensor
    curve: Optional[torch.Tensor] = None

    def field(self, name: str) -> torch.Tensor:
        if name in LEDGER_F32:
            return self.state[:, LEDGER_F32.index(name)].view(torch.float32)
        if name in LEDGER_I32:
            return self.state[:, len(LEDGER_F32) + LEDGER_I32.index(name)]
        if name in LEDGER_I64:
            return self.state.view(torch.int64)[:, 10 + LEDGER_I64.index(name)]
        raise AttributeError(name)

    def __getattr__(self, name: str) -> torch.Tensor:
        if name in LEDGER_FIELDS:
            return self.field(name)
        raise AttributeError(name)

    def fields64(self) -> Dict[str, torch.Tensor]:
        """Every field as a float64 CPU tensor [E] (the input of :func:`report_from_fields`)."""
        return {n: self.field(n).double().cpu() for n in LEDGER_FIELDS}


def chunk_sums(gain: torch.Tensor) -> torch.Tensor:
    """[chunks, ...]: the sum of every 16-series chunk of ``gain`` [E, ...] fp32 by the kernel's tree (lanes 8, 4,
    2, 1 apart, lane l taking lane l + w), rows past E contributing 0."""
    E = gain.shape[0]
    nch = -(-E // CHUNK)
    v = torch.zeros((nch * CHUNK,) + tuple(gain.shape[1:]), dtype=torch.float32, device=gain.device)
    v[:E] = gain
    v = v.view((nch, CHUNK) + tuple(gain.shape[1:]))
    for w in (8, 4, 2, 1):
        v = v[:, :w] + v[:, w:2 * w]
    return v[:, 0]


def curve_from_chunks(part: torch.Tensor) -> torch.Tensor:
    """[steps] float64: the chunks' fp32 partial sums added in ascending order from 0
    (``qrollout_curve_reduce_kernel``)."""
    curve = torch.zeros(part.shape[1], dtype=torch.float64, device=part.device)
    for c in range(part.shape[0]):
        curve = curve + part[c].double()
    return curve


def ledger_from_trace(prices: torch.Tensor, actions: torch.Tensor, *, history: int, budget0: float, shares0: int,
                      start: int = 0, budget: Optional[torch.Tensor] = None, shares: Optional[torch.Tensor] = None,
                      ledger_state: Optional[torch.Tensor] = None, curve: bool = True) -> QLedger:
    """The ledger of a run under given ``actions`` [E, steps] (0 Buy, 1 Sell, 2 Hold) over ``prices`` [E, T]: the
    env as :func:`simulate_actions` runs it (never ``compat_decisions``), from ``budget`` / ``shares`` [E] (default
    the configured start), CPU or GPU tensors.

    Float32 in the kernel's order, operation by operation (every product is rounded before it is added), with the
    kernel's chunk tree for the curve, so a ledger launch equals this on its own action trace bit for bit.  A
    fresh ledger starts from ``v0 = prices[:, start + H - 1]`` and ``eq0 = eq_prev = peak = b + s * v0``, all else
    0.  Day t trades at ``v`` from ``s_before`` to ``(b, s)`` under action ``a``::

        eq = b + s * v;  pnl = eq - eq_prev;  sumsq += pnl * pnl;  eq_prev = eq
        peak = max(peak, eq);  max_dd = max(max_dd, peak - eq)
        run = run + 1 if eq < peak else 0;  dd_days = max(dd_days, run)
        d = v - v0;  sum_d += d;  sum_d2 += d * d;  sum_sd += float(s) * d
        sum_s += s;  sum_s2 += s * s  (int64);  days += 1
        chose_buy += a == 0;  chose_sell += a == 1
        refused_buy += a == 0 and s == s_before;  refused_sell += a == 1 and s == s_before
        flat_days += s == 0;  max_shares = max(max_shares, s);  v_last = v

    and the curve's entry of the day is the sum of ``eq - eq0`` over the series.  ``ledger_state`` [E, 24] int32
    (``QLedger.state`` of the piece before, with that piece's final ``budget`` / ``shares``) continues a cut run
    exactly."""
    P = prices.float()
    dev = P.device
    A = actions.to(dev)
    E, steps = (int(v) for v in A.shape)
    H, start = int(history), int(start)
    if P.shape[0] != E or start < 0 or steps < 1 or start + steps > P.shape[1] - H:
        raise ValueError(f"days {start} .. {start + steps - 1} outside 0 .. {P.shape[1] - H - 1}")
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    b = torch.full((E,), float(budget0), dtype=f32, device=dev) if budget is None else \
        budget.to(dev, f32).reshape(-1).clone()
    s = torch.full((E,), int(shares0), dtype=i32, device=dev) if shares is None else \
        shares.to(dev, i32).reshape(-1).clone()
    if ledger_state is None:
        st = torch.zeros(E, LEDGER_WORDS, dtype=i32, device=dev)
        v0 = P[:, start + H - 1].clone()
        eq0 = b + s.float() * v0
        fl = st[:, :10].view(f32)
        fl[:, 0], fl[:, 1], fl[:, 2], fl[:, 4] = eq0, eq0, v0, eq0
    else:
        st = ledger_state.to(dev, i32).contiguous().clone()
        if tuple(st.shape) != (E, LEDGER_WORDS):
            raise ValueError(f"ledger_state must be [E, 24] = {(E, LEDGER_WORDS)}, got {tuple(st.shape)}")
    led = QLedger(state=st)
    eq_prev, eq0, v0, _, peak, max_dd, sumsq, sum_d, sum_d2, sum_sd = (led.field(n).clone() for n in LEDGER_F32)
    run, dd_days, days, chose_buy, chose_sell, refused_buy, refused_sell, flat_days, max_shares = \
        (led.field(n).clone() for n in LEDGER_I32)
    sum_s, sum_s2 = (led.field(n).clone() for n in LEDGER_I64)
    zi = torch.zeros(E, dtype=i32, device=dev)
    part = torch.empty(-(-E // CHUNK), steps, dtype=f32, device=dev) if curve else None
    for i in range(steps):
        v = P[:, start + i + H]
        a = A[:, i].long()
        b, s2, _ = tr.env_transition(a, b, s, v, v, False, budget0, shares0)
        kept = s2 == s
        s = s2
        eq = b + s.float() * v
        pnl = eq - eq_prev
        sumsq = sumsq + pnl * pnl
        eq_prev = eq
        peak = torch.where(eq > peak, eq, peak)
        dd = peak - eq
        max_dd = torch.where(dd > max_dd, dd, max_dd)
        run = torch.where(eq < peak, run + 1, zi)
        dd_days = torch.maximum(dd_days, run)
        d = v - v0
        sum_d = sum_d + d
        sum_d2 = sum_d2 + d * d
        sum_sd = sum_sd + s.float() * d
        sl = s.to(i64)
        sum_s = sum_s + sl
        sum_s2 = sum_s2 + sl * sl
        days = days + 1
        chose_buy = chose_buy + (a == 0).to(i32)
        chose_sell = chose_sell + (a == 1).to(i32)
        refused_buy = refused_buy + ((a == 0) & kept).to(i32)
        refused_sell = refused_sell + ((a == 1) & kept).to(i32)
        flat_days = flat_days + (s == 0).to(i32)
        max_shares = torch.maximum(max_shares, s)
        if curve:
            part[:, i] = chunk_sums(eq - eq0)
    out = torch.zeros(E, LEDGER_WORDS, dtype=i32, device=dev)
    out[:, :10] = torch.stack([eq_prev, eq0, v0, v.clone(), peak, max_dd, sumsq, sum_d, sum_d2, sum_sd],
                              dim=1).view(i32)
    out[:, 10:19] = torch.stack([run, dd_days, days, chose_buy, chose_sell, refused_buy, refused_sell, flat_days,
                                 max_shares], dim=1)
    out[:, 20:24] = torch.stack([sum_s, sum_s2], dim=1).view(i32)
    return QLedger(state=out, curve=curve_from_chunks(part) if curve else None)


def _div(a: float, b: float) -> Optional[float]:
    return None if b == 0 else a / b


def _sharpe(total: float, sumsq: float, n: int, per_year: float) -> Optional[float]:
    """Annualised per-day Sharpe ratio from the sum and the sum of squares of n per-day gains."""
    if n == 0:
        return None
    m = total / n
    var = sumsq / n - m * m
    return None if var <= 0.0 else m / math.sqrt(var) * math.sqrt(per_year)


def _mean_median(x) -> Tuple[Optional[float], Optional[float]]:
    x = [v for v in x if v is not None]
    return (sum(x) / len(x), float(np.median(x))) if x else (None, None)


def report_from_fields(f: Dict[str, torch.Tensor], curve: Optional[torch.Tensor],
                       days_per_year: float = 252.0) -> Dict[str, object]:
    """:meth:`BacktestResult.report` from the ledger's fields as float64 CPU tensors [E] (``QLedger.fields64()``, or
    the same sums taken in float64 from a trace) and the float64 ``curve`` [steps] or None."""
    n = int(f["days"].numel())
    dpy = float(days_per_year)
    ret = f["eq_prev"] - f["eq0"]
    days = f["days"]
    tot_days = float(days.sum())
    sh = [_sharpe(r, q, int(d), dpy) for r, q, d in zip(ret.tolist(), f["sumsq"].tolist(), days.tolist())]
    sh_mean, sh_median = _mean_median(sh)
    buy, sell = float(f["chose_buy"].sum()), float(f["chose_sell"].sum())
    safe = torch.where(days > 0, days, torch.ones_like(days))
    exposure = f["sum_s"] / safe * (f["v_last"] - f["v0"])
    timing = ret - exposure
    # position / price correlation of a series from its five sums
    cov = f["sum_sd"] - f["sum_s"] * f["sum_d"] / safe
    var_s = f["sum_s2"] - f["sum_s"] * f["sum_s"] / safe
    var_d = f["sum_d2"] - f["sum_d"] * f["sum_d"] / safe
    ok = (var_s > 0) & (var_d > 0)
    corr = cov[ok] / torch.sqrt(var_s[ok] * var_d[ok])
    series = {"n": n, "ret_mean": float(ret.sum()) / n, "ret_median": float(ret.median()),
              "max_dd_mean": float(f["max_dd"].sum()) / n, "max_dd_worst": float(f["max_dd"].max()),
              "dd_days_longest": int(f["dd_days"].max()),
              "sharpe_mean": sh_mean, "sharpe_median": sh_median, "sharpe_undefined": sum(v is None for v in sh),
              "shares_mean": _div(float(f["sum_s"].sum()), tot_days),
              "flat_frac": _div(float(f["flat_days"].sum()), tot_days),
              "buy_frac": _div(buy, tot_days), "sell_frac": _div(sell, tot_days),
              "hold_frac": _div(tot_days - buy - sell, tot_days),
              "refused_buy_frac": _div(float(f["refused_buy"].sum()), buy),
              "refused_sell_frac": _div(float(f["refused_sell"].sum()), sell),
              "exposure_mean": float(exposure.sum()) / n, "exposure_median": float(exposure.median()),
              "timing_mean": float(timing.sum()) / n, "timing_median": float(timing.median()),
              "corr_median": float(corr.median()) if corr.numel() else None,
              "corr_undefined": n - int(corr.numel())}
    portfolio = None
    if curve is not None:
        c = curve.double().cpu() / n
        peak = torch.cummax(torch.clamp(c, min=0.0), 0).values
        inc = torch.diff(c, prepend=torch.zeros(1, dtype=torch.float64))
        portfolio = {"total": float(c[-1]), "max_dd": float((peak - c).max()),
                     "sharpe": _sharpe(float(c[-1]), float((inc * inc).sum()), int(c.numel()), dpy)}
    return {"days_per_year": dpy, "series": series, "portfolio": portfolio}


@dataclass
class BacktestResult:
    """What a policy did over ``steps`` days from day ``start`` of every series: per-env tensors and, when
    traced, the per-day actions (0 Buy, 1 Sell, 2 Hold), Q rows and portfolio values."""

    budget: torch.Tensor            # [E] fp32 final budget
    shares: torch.Tensor            # [E] int32 final shares
    final_portfolio: torch.Tensor   # [E] fp32 budget + shares * last trade price
    buys: torch.Tensor              # [E] int32 executed buys
    sells: torch.Tensor             # [E] int32 executed sells
    budget0: float
    start: int
    steps: int
    actions: Optional[torch.Tensor] = None   # [E, steps] int8
    q: Optional[torch.Tensor] = None         # [E, steps, 3] fp32
    equity: Optional[torch.Tensor] = None    # [E, steps] fp32
    ledger: Optional[QLedger] = None         # the risk ledger (``ledger=True``)

    def report(self, days_per_year: float = 252.0) -> Dict[str, object]:
        """The risk report of a run made with ``ledger=True``, computed in float64 on the host from the ledger's
        records; a ratio with a zero denominator is None.  With a carried ``ledger_state`` the ``series`` block is
        of the whole run so far, the ``portfolio`` block of this piece's curve.

        * ``series``: mean / median return ``eq_prev - eq0``; mean / worst ``max_dd``; the longest drawdown in
          days; mean / median of the per-series annualised Sharpe ratio (from the return, ``sumsq`` and ``days``;
          series with zero variance are left out and counted in ``sharpe_undefined``); mean shares, the
          zero-share fraction of the env-days, the chosen Buy / Sell / Hold mix, the refused share of the chosen
          Buys and Sells; ``exposure = sum_s / days * (v_last - v0)`` (what the mean position earned on the
          series' price move) and ``timing = return - exposure``, each as mean and median; the median
          position / price correlation (from ``sum_s, sum_s2, sum_d, sum_d2, sum_sd``; series with a constant
          position or price are counted in ``corr_undefined``);
        * ``portfolio`` (None without a curve): the equal-weight book ``curve / E``: its total, max drawdown
          (peak from 0) and Sharpe ratio of its daily changes.

        fp32 accuracy (``profiles/backtest_ledger.md``): worst relative difference per entry between this report
        and the same report from float64 sums over the trace of the same launch, a full 5,846-day episode of
        8,192 series, greedy and epsilon-greedy: 0 for every entry of returns, drawdowns, counts, shares, mix,
        exposure and timing (their fields are exact or integer); ``sharpe_mean`` 5.2e-7, ``sharpe_median``
        4.4e-7 (``sumsq``); ``portfolio`` total 2.0e-9, max_dd 3.9e-7, sharpe 5.4e-8 (the fp32 16-series
        partial sums); ``corr_median`` 1.4e-3: the covariance ``sum_sd - sum_s * sum_d / days`` is a small
        difference of large sums, and the fp32 ``sum_sd`` (and ``sum_d``) carry 5,846 roundings each, so the
        correlation is good to about three digits."""
        if self.ledger is None:
            raise ValueError("report() needs a backtest made with ledger=True")
        return report_from_fields(self.ledger.fields64(), self.ledger.curve, days_per_year)

    def summary(self) -> Dict[str, float]:
        """Mean / population std / median of ``final_portfolio - budget0`` over the series (the statistics of
        ``benchkit._reduce_returns``; the median is an element of the sample) and the executed trades."""
        fin = self.final_portfolio.double() - float(self.budget0)
        n = int(fin.numel())
        m = float(fin.sum()) / n
        return {"n": n, "mean": m, "std": math.sqrt(max(0.0, float((fin * fin).sum()) / n - m * m)),
                "median": float(fin.median()), "steps": int(self.steps), "buys": int(self.buys.sum()),
                "sells": int(self.sells.sum())}


def result_from(out: Dict[str, torch.Tensor], budget0: float, start: int, steps: int, trace: bool,
                ledger: Optional[QLedger] = None) -> BacktestResult:
    if ledger is None and "ledger_state" in out:
        ledger = QLedger(state=out["ledger_state"], curve=out.get("curve"))
    return BacktestResult(budget=out["budget"], shares=out["shares"], final_portfolio=out["portfolio"],
                          buys=out["buys"], sells=out["sells"], budget0=float(budget0), start=int(start),
                          steps=int(steps), actions=out.get("actions") if trace else None,
                          q=out["q"] if trace else None, equity=out["equity"] if trace else None,
                          ledger=ledger)
