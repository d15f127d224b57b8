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


_bound = False


def _lib() -> C.CDLL:
    global _bound
    L = native.lib()
    if not _bound:
        L.st_qrollout_launch.argtypes = [C.POINTER(RolloutParams), C.c_int, C.c_void_p]
        L.st_qrollout_launch.restype = C.c_int
        L.st_qrollout_lds_bytes.restype = C.c_int
        L.st_qrollout_day_block.restype = C.c_int
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
            trace: bool = False, env_offset: int = 0, grid: int = 0) -> Dict[str, torch.Tensor]:
        """``prices`` [E, >= T] fp32 on the GPU (row stride = ``prices.stride(0)``, ``T`` valid values per row,
        default all); ``budget`` [E] fp32 / ``shares`` [E] int32 or None (the configured start).  One launch on
        the current stream; returns the per-env results (and the traces with ``trace``)."""
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
        if E > 0:
            native.check(_lib().st_qrollout_launch(C.byref(p), int(grid), native.stream_handle()), "st_qrollout_launch")
        return out


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

    def summary(self) -> Dict[str, float]:
        """Mean / population std / median of ``final_portfolio - budget0`` over the series (the statistics of
        ``benchkit._reduce_returns``; the median is an element of the sample) and the executed trades."""
        fin = self.final_portfolio.double() - float(self.budget0)
        n = int(fin.numel())
        m = float(fin.sum()) / n
        return {"n": n, "mean": m, "std": math.sqrt(max(0.0, float((fin * fin).sum()) / n - m * m)),
                "median": float(fin.median()), "steps": int(self.steps), "buys": int(self.buys.sum()),
                "sells": int(self.sells.sum())}


def result_from(out: Dict[str, torch.Tensor], budget0: float, start: int, steps: int, trace: bool) -> BacktestResult:
    return BacktestResult(budget=out["budget"], shares=out["shares"], final_portfolio=out["portfolio"],
                          buys=out["buys"], sells=out["sells"], budget0=float(budget0), start=int(start),
                          steps=int(steps), actions=out.get("actions") if trace else None,
                          q=out["q"] if trace else None, equity=out["equity"] if trace else None)
