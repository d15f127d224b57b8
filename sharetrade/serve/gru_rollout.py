"""Backtesting a frozen GRU(256) policy on minute bars: whole episodes in one launch
(``csrc/gru_rollout.hip``) and their PyTorch oracle.

"What would this recurrent policy have done, greedily, over bars it was not trained on?"  For env ``e`` and
bar ``t = start .. start + steps - 1`` a bar is the actor's (``csrc/gru.hip::gru_act_kernel``): x row (8 market
features, position, unrealised pnl %, elapsed fraction, 1) -> GRU cell (bf16 W_ih, MX-fp8 W_hh and h) -> Q
head -> first maximum -> optional epsilon rule -> ``env/minute.py::step`` without the random restart.
Episodes are consecutive ``ep_len``-bar stretches counted from ``origin``; after an episode's last bar the
position goes flat at no cost, the entry price is cleared and ``h`` restarts from 0.

* :class:`GruPolicy` holds the parameters and their packed form; it builds no learner (no replay, no bank).
* :func:`reference_gru_rollout` is the same computation bar by bar in PyTorch: the CPU backend and the
  numerics oracle of ``tests/test_gpu_gru_backtest.py`` (env in float32 in the kernel's operation order, net
  in float64 with every rounding point of the kernel emulated).
* :func:`simulate_minute_actions` is the env alone, for baselines.

A run can be cut into pieces: pass a piece's final ``h`` / ``position`` / ``entry`` and the next ``start``
with the same ``origin``; the pieces reproduce the whole bit for bit.

``ledger=True`` also keeps the risk ledger on the chip (the ledger instance of the kernel): per series the
running equity curve's peak, deepest and longest drawdown and sum of squared rewards, every episode's return and
trades, the round trips and their wins, and the portfolio's per-bar sum of rewards (:class:`GruLedger`).
:func:`ledger_from_trace` is the same arithmetic in PyTorch float32 on a trace: the ``torch`` backend's ledger,
the kernel's oracle (bit for bit) and the ledger of the baselines.  ``GruBacktestResult.report()`` turns a ledger
into drawdown, Sharpe, hit rate, per-episode and portfolio figures.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Union

import numpy as np
import torch

from ..data import minute_bars as mb
from ..models import gru_qnet as gq
from ..ops import gru as G
from ..utils import rng

TAG_ROLLOUT = 0x47524231   # "GRB1": Philox counter word 3 of the backtest draws, (env_offset + e, t, 0, tag)
KEY_RANK = 5               # the actors' key: rng.key_for(seed, 5)
PARAM_NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_q", "b_q")
ROUNDING_POINTS = frozenset({"x", "w_ih", "w_hh", "h", "q"})


def _shapes() -> Dict[str, tuple]:
    H, N = gq.HID, gq.N_ACT
    return {"w_ih": (3 * H, gq.X_PAD), "w_hh": (3 * H, H), "b_ih": (3 * H,), "b_hh": (3 * H,), "w_q": (N, H),
            "b_q": (N,)}


def split_flat(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The learner's flat fp32 parameter buffer (``RecurrentDQN.flat``) -> named tensors (copies)."""
    out, o = {}, 0
    for n, shp in _shapes().items():
        k = int(np.prod(shp))
        out[n] = flat[o:o + k].detach().clone().float().reshape(shp)
        o += k
    if flat.numel() < o:
        raise ValueError(f"flat parameter buffer holds {flat.numel()} values, a GRU(256) policy needs {o}")
    return out


def draws(seed: int, env_ids: np.ndarray, t: int):
    """The backtest's Philox draws for bar ``t``: (explore coin u0, random action u1) per env."""
    k0, k1 = rng.key_for(seed, KEY_RANK)
    n = env_ids.shape[0]
    c0, c1, _, _ = rng.philox4x32(env_ids, np.full(n, t & 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32),
                                  np.full(n, TAG_ROLLOUT, np.uint32), np.full(n, k0), np.full(n, k1))
    return rng.u24(c0), rng.u24(c1)


def policy_actions(greedy_a: torch.Tensor, seed: int, env_ids: np.ndarray, t: int, epsilon: float) -> torch.Tensor:
    """The epsilon rule on one bar: exploit iff u0 < epsilon, else min(int(u1 * 3), 2); inf = greedy, no draws."""
    if math.isinf(epsilon):
        return greedy_a
    u0, u1 = draws(seed, env_ids, t)
    exploit = torch.from_numpy(u0 < np.float32(epsilon)).to(greedy_a.device)
    rnd = torch.from_numpy(np.minimum((u1 * np.float32(3)).astype(np.int64), 2)).to(greedy_a.device)
    return torch.where(exploit, greedy_a, rnd)


def _check_run(E: int, T: int, start: int, steps: Optional[int], ep_len: int, origin: Optional[int]):
    start = int(start)
    steps = T - 1 - start if steps is None else int(steps)
    origin = start if origin is None else int(origin)
    if E < 1 or ep_len < 1:
        raise ValueError("need at least one series and ep_len >= 1")
    if start < 0 or steps < 1 or start + steps > T - 1:
        raise ValueError(f"bars start .. start + steps - 1 = {start} .. {start + steps - 1} outside 0 .. {T - 2} "
                         "(every reward needs the next close)")
    if origin > start:
        raise ValueError(f"origin {origin} lies after start {start}")
    return start, steps, origin


class _Env:
    """The minute env for E series at once, float32, in the kernel's operation order (``csrc/minute_rule.h``)."""

    def __init__(self, E: int, cost: float, position, entry, dev):
        self.pz = torch.zeros(E, dtype=torch.int32, device=dev) if position is None else \
            position.to(dev, torch.int32).clone()
        self.entry = torch.zeros(E, dtype=torch.float32, device=dev) if entry is None else \
            entry.to(dev, torch.float32).clone()
        self.ret = torch.zeros(E, dtype=torch.float32, device=dev)
        self.trades = torch.zeros(E, dtype=torch.int32, device=dev)
        self.long = torch.zeros(E, dtype=torch.int32, device=dev)
        self.cost = torch.tensor(float(cost), dtype=torch.float32, device=dev)
        self.zero = torch.zeros((), dtype=torch.float32, device=dev)

    def x_env(self, c: torch.Tensor, elapsed: int, inv_ep_len) -> torch.Tensor:
        """Columns 8 .. 11 of the x row (fp32, before the bf16 rounding)."""
        held = self.pz != 0
        safe = torch.where(held, self.entry, torch.ones_like(self.entry))
        upnl = torch.where(held, (c / safe - 1.0) * 100.0, torch.zeros_like(c))
        frac = torch.full_like(c, float(np.float32(elapsed) * np.float32(inv_ep_len)))
        return torch.stack([self.pz.float(), upnl, frac, torch.ones_like(c)], dim=1)

    def step(self, a: torch.Tensor, c: torch.Tensor, r: torch.Tensor, done: bool) -> torch.Tensor:
        a = a.to(torch.int32)
        np_ = torch.where(a == 0, torch.ones_like(self.pz), torch.where(a == 1, torch.zeros_like(self.pz), self.pz))
        trade = np_ != self.pz
        self.entry = torch.where(trade & (np_ == 1), c, self.entry)
        rew = np_.float() * r - torch.where(trade, self.cost, self.zero)
        self.ret = self.ret + rew
        self.trades = self.trades + trade.int()
        self.long = self.long + np_
        if done:
            self.pz = torch.zeros_like(np_)
            self.entry = torch.zeros_like(self.entry)
        else:
            self.pz = np_
        return rew


def simulate_minute_actions(close: torch.Tensor, actions: torch.Tensor, *, start: int = 0, ep_len: int = 390,
                            cost: float = 0.01, origin: Optional[int] = None,
                            position: Optional[torch.Tensor] = None, entry: Optional[torch.Tensor] = None,
                            ret: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The env alone under given ``actions`` [E, steps] (no net): ``ret``, ``trades``, ``long``, ``position``,
    ``entry`` [E] and the ``reward`` trace [E, steps], e.g. for the always-long and random baselines."""
    Cl = close.float()
    E, T = Cl.shape
    start, steps, origin = _check_run(E, T, start, actions.shape[1], ep_len, origin)
    R = mb.bar_returns(Cl) if ret is None else ret.to(Cl.device, torch.float32)
    env = _Env(E, cost, position, entry, Cl.device)
    reward = torch.empty(E, steps, dtype=torch.float32, device=Cl.device)
    for i in range(steps):
        t = start + i
        done = (t + 1 - origin) % ep_len == 0
        reward[:, i] = env.step(actions[:, i].to(Cl.device), Cl[:, t], R[:, t], done)
    return {"ret": env.ret, "trades": env.trades, "long": env.long, "position": env.pz, "entry": env.entry,
            "reward": reward}


class GruBarNet:
    """The net arithmetic of one bar, shared by :func:`reference_gru_rollout` and the serving oracle
    (``serve/gru_serve.py::reference_gru_serve``): the weights prepared once (gate pre-scale, rounding points
    ``pts`` emulated), then ``bar(x, h) -> (h', q)`` on fp32 x rows [N, 12] and the state ``h`` [N, 256]."""

    def __init__(self, params: Dict[str, torch.Tensor], pts, dtype: torch.dtype, dev):
        H = gq.HID
        bf = self.bf
        self.pts, self.dtype = pts, dtype
        P = {n: params[n].detach().to(dev).float().reshape(_shapes()[n]) for n in PARAM_NAMES}
        # the packed weights carry the gate pre-scale (gru_pack_kernel): fp32 product, then the rounding; the
        # gates are evaluated on the pre-scaled pre-activations as 1 / (1 + 2^y) and 2 / (1 + 2^y) - 1
        gs = G.gate_prescale().to(dev)
        wih = P["w_ih"][:, :gq.X_ACT] * gs[:, None]
        whh = P["w_hh"] * gs[:, None]
        self.Wih = (bf(wih) if "w_ih" in pts else wih).to(dtype)
        self.Whh = (G.mx_roundtrip(whh) if "w_hh" in pts else whh).to(dtype)
        self.b_rz = ((P["b_ih"] + P["b_hh"])[:2 * H] * G.GS_RZ).to(dtype)
        self.b_in = (P["b_ih"][2 * H:] * G.GS_N).to(dtype)
        self.b_hn = (P["b_hh"][2 * H:] * G.GS_N).to(dtype)
        self.Wq = (bf(P["w_q"]) if "q" in pts else P["w_q"]).to(dtype)
        self.bq = P["b_q"].to(dtype)

    @staticmethod
    def bf(v: torch.Tensor) -> torch.Tensor:
        return v.float().to(torch.bfloat16).float()

    def bar(self, x: torch.Tensor, h: torch.Tensor):
        H, pts, dtype, bf = gq.HID, self.pts, self.dtype, self.bf
        b_rz, b_in, b_hn = self.b_rz, self.b_in, self.b_hn
        x = (bf(x) if "x" in pts else x).to(dtype)
        hq = G.mx_roundtrip(h.float()).to(dtype) if "h" in pts else h   # (the kernel's state is fp32)
        gx = x @ self.Wih[:, :x.shape[1]].t()
        gh = hq @ self.Whh.t()
        r = 1.0 / (1.0 + torch.exp2(gx[:, :H] + gh[:, :H] + b_rz[:H]))
        z = 1.0 / (1.0 + torch.exp2(gx[:, H:2 * H] + gh[:, H:2 * H] + b_rz[H:]))
        n = 2.0 / (1.0 + torch.exp2(r * (gh[:, 2 * H:] + b_hn) + (gx[:, 2 * H:] + b_in))) - 1.0
        h = z * (h - n) + n
        hb = (bf(h) if "q" in pts else h.float()).to(dtype)
        q = (hb @ self.Wq.t() + self.bq).float()
        return h, q


def rounding_points(emulate: Union[bool, Iterable[str]]) -> set:
    """The ``emulate=`` switch of the oracles as a set of names from ``ROUNDING_POINTS``."""
    pts = set(ROUNDING_POINTS) if emulate is True else set() if emulate is False else set(emulate)
    if not pts <= ROUNDING_POINTS:
        raise ValueError(f"unknown rounding points {sorted(pts - ROUNDING_POINTS)}")
    return pts


def reference_gru_rollout(params: Dict[str, torch.Tensor], close: torch.Tensor, feat: torch.Tensor, *,
                          start: int = 0, steps: Optional[int] = None, ep_len: int = 390, cost: float = 0.01,
                          origin: Optional[int] = None, epsilon: float = math.inf, seed: int = 0,
                          h0: Optional[torch.Tensor] = None, position: Optional[torch.Tensor] = None,
                          entry: Optional[torch.Tensor] = None, env_offset: int = 0,
                          forced_actions: Optional[torch.Tensor] = None,
                          emulate: Union[bool, Iterable[str]] = True, dtype: torch.dtype = torch.float64,
                          ret: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The rollout bar by bar in PyTorch for ``close`` [E, T] and ``feat`` [E, T, 8] (CPU or GPU tensors).

    Returns the kernel's fields: ``ret``, ``trades``, ``long``, ``position``, ``entry`` [E], ``h`` [E, 256] and
    the traces ``actions`` int8 [E, steps], ``q`` [E, steps, 3], ``reward`` [E, steps].

    The env is float32 in the kernel's operation order.  The net runs in ``dtype`` with the kernel's rounding
    points emulated (``emulate=True``; a collection of names from ``ROUNDING_POINTS`` emulates only those):
    ``x`` bf16 x row; ``w_ih`` bf16 of the pre-scaled W_ih rows; ``w_hh`` MX-fp8 of the pre-scaled W_hh rows;
    ``h`` MX-fp8 of the fp32 state entering the recurrent product; ``q`` bf16 h' and bf16 W_q in the Q head.
    ``emulate=False`` is the plain GRU cell.  ``forced_actions`` [E, steps] replaces the policy's choice
    (``q`` is still the net's); ``epsilon = inf`` is greedy."""
    pts = rounding_points(emulate)
    Cl = close.float()
    E, T = Cl.shape
    dev = Cl.device
    start, steps, origin = _check_run(E, T, start, steps, ep_len, origin)
    F = feat.to(dev).float()
    R = mb.bar_returns(Cl) if ret is None else ret.to(dev, torch.float32)
    H = gq.HID
    net = GruBarNet(params, pts, dtype, dev)
    env = _Env(E, cost, position, entry, dev)
    h = torch.zeros(E, H, dtype=dtype, device=dev) if h0 is None else h0.to(dev, torch.float32).to(dtype).clone()
    ids = (np.arange(E, dtype=np.uint64) + np.uint64(int(env_offset) & 0xFFFFFFFF)).astype(np.uint32)
    inv_ep_len = np.float32(1.0 / ep_len)
    actions = torch.empty(E, steps, dtype=torch.int8, device=dev)
    qs = torch.empty(E, steps, gq.N_ACT, dtype=torch.float32, device=dev)
    reward = torch.empty(E, steps, dtype=torch.float32, device=dev)
    es = origin + (start - origin) // ep_len * ep_len
    for i in range(steps):
        t = start + i
        done = (t + 1 - es) >= ep_len
        x = torch.cat([F[:, t], env.x_env(Cl[:, t], t - es, inv_ep_len)], dim=1)
        h, q = net.bar(x, h)
        a = policy_actions(torch.argmax(q, dim=1), seed, ids, t, float(epsilon))   # first max on ties
        if forced_actions is not None:
            a = forced_actions[:, i].to(dev).long()
        reward[:, i] = env.step(a, Cl[:, t], R[:, t], done)
        actions[:, i] = a.to(torch.int8)
        qs[:, i] = q
        if done:
            es = t + 1
            h = torch.zeros_like(h)
    return {"ret": env.ret, "trades": env.trades, "long": env.long, "position": env.pz, "entry": env.entry,
            "h": h.float(), "actions": actions, "q": qs, "reward": reward}


CHUNK = G.RN   # envs whose rewards one workgroup sums per bar (the kernel's 32-env chunk)


def episode_columns(start: int, steps: int, origin: int, ep_len: int):
    """(es0, n_ep, full): the start of the episode that holds bar ``start``, the episode columns bars
    ``start .. start + steps - 1`` touch, and per column whether all ``ep_len`` of its bars lie in the run."""
    es0 = origin + (start - origin) // ep_len * ep_len
    n_ep = (start + steps - 1 - es0) // ep_len + 1
    full = [es0 + k * ep_len >= start and es0 + (k + 1) * ep_len <= start + steps for k in range(n_ep)]
    return es0, n_ep, full


@dataclass
class GruLedger:
    """The risk ledger of one run (piece): what ``csrc/gru_rollout.hip``'s ledger instance keeps per series.

    ``state`` continues a cut run (``ledger_state=`` of the next piece); the other per-series fields are of this
    piece alone, with drawdowns measured on the curve carried in through ``state``."""

    ep_ret: torch.Tensor      # [E, n_ep] fp32 return of every episode column
    ep_trades: torch.Tensor   # [E, n_ep] int32 position changes of every episode column
    max_dd: torch.Tensor      # [E] fp32 deepest peak - cum (the peak starts at 0)
    dd_bars: torch.Tensor     # [E] int32 longest stretch of bars with cum < peak
    sumsq: torch.Tensor       # [E] fp32 sum of squared rewards
    trips: torch.Tensor       # [E] int32 closed round trips (a long forced flat at an episode end closes)
    wins: torch.Tensor        # [E] int32 closed trips with a positive sum of rewards
    win_sum: torch.Tensor     # [E] fp32 sum of the winning trips
    loss_sum: torch.Tensor    # [E] fp32 sum of the other trips (<= 0)
    state: torch.Tensor       # [E, 8] int32 records {cum, peak, trip, ep (fp32 bits), run, ep_tr, 0, 0}
    full: List[bool]          # per column: a whole episode (the first and last may be partial)
    curve: Optional[torch.Tensor] = None   # [steps] fp32 sum over the series of the bar's rewards

    def state_field(self, name: str) -> torch.Tensor:
        """Column ``name`` of ``state`` (``cum``, ``peak``, ``trip``, ``ep`` as fp32; ``run``, ``ep_tr`` int32)."""
        col = self.state[:, G.LEDGER_STATE_COLS.index(name)]
        return col.view(torch.float32) if name in G.LEDGER_STATE_FLOAT else col


def _ledger_of_records(ep_ret, ep_trades, stats, state, full, curve) -> GruLedger:
    f = {n: (stats[:, i].view(torch.float32) if n in G.LEDGER_STATS_FLOAT else stats[:, i])
         for i, n in enumerate(G.LEDGER_STATS_COLS)}
    return GruLedger(ep_ret=ep_ret, ep_trades=ep_trades, state=state, full=full, curve=curve, **f)


def chunk_sums(reward: torch.Tensor) -> torch.Tensor:
    """[chunks, steps]: per bar the sum of every 32-series chunk's rewards by the kernel's butterfly (lanes 16,
    8, 4, 2, 1 apart), rows past E contributing 0."""
    E, steps = reward.shape
    nch = -(-E // CHUNK)
    v = torch.zeros(nch * CHUNK, steps, dtype=torch.float32, device=reward.device)
    v[:E] = reward
    v = v.view(nch, CHUNK, steps)
    for w in (16, 8, 4, 2, 1):
        v = v[:, :w] + v[:, w:2 * w]
    return v[:, 0]


def curve_from_chunks(part: torch.Tensor) -> torch.Tensor:
    """[steps]: the chunks' partial sums added in ascending order from 0 (``gru_curve_reduce_kernel``)."""
    curve = torch.zeros(part.shape[1], dtype=torch.float32, device=part.device)
    for c in range(part.shape[0]):
        curve = curve + part[c]
    return curve


def ledger_from_trace(actions: torch.Tensor, reward: torch.Tensor, *, position: Optional[torch.Tensor] = None,
                      start: int, origin: int, ep_len: int, ledger_state: Optional[torch.Tensor] = None,
                      curve: bool = True) -> GruLedger:
    """The ledger of a traced run: ``actions`` [E, steps] (0 Buy, 1 Sell, 2 Hold) and ``reward`` [E, steps] of
    bars ``start .. start + steps - 1``, ``position`` [E] the position before bar ``start`` (None: flat).

    Float32 in the kernel's order, operation by operation (every product is rounded before it is added), so a
    ledger launch equals this on its own trace bit for bit.  After bar t gives ``reward``, ``trade`` and
    ``position'``:

    * curve: ``cum += reward``; ``peak = cum if cum > peak``; ``max_dd`` the largest ``peak - cum``; ``run`` counts
      the bars since ``cum < peak`` began and ``dd_bars`` is its maximum; ``sumsq += reward * reward``;
    * episodes: ``ep += reward``, ``ep_tr += trade``, stored in column k on an episode's last bar and on the run's
      last bar; an episode's last bar then clears both and moves to column k + 1;
    * round trips: a bar that opens a long starts ``trip = reward``; any other bar that began long adds its
      reward (a Sell's cost included); a Sell from long, or an episode end with a long held (flat at no cost),
      closes the trip: ``trips``, ``wins`` if ``trip > 0``, ``win_sum`` / ``loss_sum``, ``trip = 0``.

    ``ledger_state`` [E, 8] int32 (``GruLedger.state`` of the piece before) continues a cut run exactly."""
    R = reward.float()
    E, steps = (int(v) for v in R.shape)
    dev = R.device
    A = actions.to(dev)
    start, origin, ep_len = int(start), int(origin), int(ep_len)
    es0, n_ep, full = episode_columns(start, steps, origin, ep_len)
    i32, f32 = torch.int32, torch.float32
    if ledger_state is None:
        st = torch.zeros(E, 8, dtype=i32, device=dev)
    else:
        st = ledger_state.to(dev, i32).contiguous().clone()
        if tuple(st.shape) != (E, 8):
            raise ValueError(f"ledger_state must be [E, 8] = {(E, 8)}, got {tuple(st.shape)}")
    fl = st[:, :4].contiguous().view(f32)
    cum, peak, trip, ep = (fl[:, j].clone() for j in range(4))
    run, ep_tr = st[:, 4].clone(), st[:, 5].clone()
    pz = torch.zeros(E, dtype=i32, device=dev) if position is None else position.to(dev, i32).clone()
    zf, zi, one = torch.zeros(E, dtype=f32, device=dev), torch.zeros(E, dtype=i32, device=dev), \
        torch.ones(E, dtype=i32, device=dev)
    mdd, ssq, wsum, lsum = zf.clone(), zf.clone(), zf.clone(), zf.clone()
    ddb, trips, wins = zi.clone(), zi.clone(), zi.clone()
    ep_ret = torch.zeros(E, n_ep, dtype=f32, device=dev)
    ep_trades = torch.zeros(E, n_ep, dtype=i32, device=dev)
    es, k = es0, 0
    for i in range(steps):
        t = start + i
        done = (t + 1 - es) >= ep_len
        a, rw = A[:, i], R[:, i]
        np_ = torch.where(a == 0, one, torch.where(a == 1, zi, pz))
        trade = np_ != pz
        # running curve
        cum = cum + rw
        peak = torch.where(cum > peak, cum, peak)
        dd = peak - cum
        mdd = torch.where(dd > mdd, dd, mdd)
        run = torch.where(cum < peak, run + 1, zi)
        ddb = torch.maximum(ddb, run)
        ssq = ssq + rw * rw
        # episode ledger
        ep = ep + rw
        ep_tr = ep_tr + trade.to(i32)
        if done or i == steps - 1:
            ep_ret[:, k] = ep
            ep_trades[:, k] = ep_tr
        if done:
            ep, ep_tr = zf.clone(), zi.clone()
        # round trips
        opens = trade & (np_ == 1)
        trip = torch.where(opens, rw, torch.where(pz != 0, trip + rw, trip))
        closes = trade & (np_ == 0)
        if done:
            closes = closes | (np_ == 1)
        won = trip > 0
        trips = trips + closes.to(i32)
        wins = wins + (closes & won).to(i32)
        wsum = torch.where(closes & won, wsum + trip, wsum)
        lsum = torch.where(closes & ~won, lsum + trip, lsum)
        trip = torch.where(closes, zf, trip)
        pz = zi.clone() if done else np_
        if done:
            es, k = t + 1, k + 1
    state = torch.zeros(E, 8, dtype=i32, device=dev)
    state[:, :4] = torch.stack([cum, peak, trip, ep], dim=1).view(i32)
    state[:, 4], state[:, 5] = run, ep_tr
    return GruLedger(ep_ret=ep_ret, ep_trades=ep_trades, max_dd=mdd, dd_bars=ddb, sumsq=ssq, trips=trips, wins=wins,
                     win_sum=wsum, loss_sum=lsum, state=state, full=full,
                     curve=curve_from_chunks(chunk_sums(R)) if curve else None)


def _div(a: float, b: float) -> Optional[float]:
    return None if b == 0 else a / b


def _sharpe(total: float, sumsq: float, n: int, bars_per_year: float) -> Optional[float]:
    """Annualised per-bar Sharpe ratio from the sum and the sum of squares of n per-bar returns."""
    m = total / n
    var = sumsq / n - m * m
    return None if var <= 0.0 else m / math.sqrt(var) * math.sqrt(bars_per_year)


def _moments(x: torch.Tensor) -> Dict[str, Optional[float]]:
    """mean / population std / worst / share positive of a float64 sample (None when it is empty)."""
    n = int(x.numel())
    if n == 0:
        return {"n": 0, "mean": None, "std": None, "worst": None, "positive": None}
    m = float(x.sum()) / n
    return {"n": n, "mean": m, "std": math.sqrt(max(0.0, float((x * x).sum()) / n - m * m)),
            "worst": float(x.min()), "positive": float((x > 0).sum()) / n}


@dataclass
class GruBacktestResult:
    """What a GRU policy did over ``steps`` bars from bar ``start`` of every series: per-env tensors and, when
    traced, the per-bar actions (0 Buy, 1 Sell, 2 Hold), Q rows and rewards."""

    ret: torch.Tensor        # [E] fp32 sum of rewards (%, in bar order)
    trades: torch.Tensor     # [E] int32 position changes
    long: torch.Tensor       # [E] int32 bars held long
    position: torch.Tensor   # [E] int32 final position
    entry: torch.Tensor      # [E] fp32 final entry price
    start: int
    steps: int
    ep_len: int
    origin: int
    backend: str = "hip"
    h: Optional[torch.Tensor] = None         # [E, 256] fp32 final recurrent state (None: the env alone)
    actions: Optional[torch.Tensor] = None   # [E, steps] int8
    q: Optional[torch.Tensor] = None         # [E, steps, 3] fp32
    reward: Optional[torch.Tensor] = None    # [E, steps] fp32
    ledger: Optional[GruLedger] = None       # the risk ledger (``ledger=True``)

    def summary(self) -> Dict[str, float]:
        """Mean / population std / median of the per-env return (the median is an element of the sample),
        the mean return per full episode (``mean * ep_len / steps``), the position changes and the fraction
        of (env, bar) pairs held long."""
        r = self.ret.double()
        n = int(r.numel())
        m = float(r.sum()) / n
        return {"n": n, "mean": m, "std": math.sqrt(max(0.0, float((r * r).sum()) / n - m * m)),
                "median": float(r.median()), "per_episode": m * self.ep_len / self.steps, "steps": int(self.steps),
                "trades": int(self.trades.sum()), "long_frac": float(self.long.sum()) / (n * self.steps)}

    def report(self, bars_per_year: Optional[float] = None) -> Dict[str, object]:
        """The risk report of a run made with ``ledger=True``, computed in float64 on the host; a ratio with a
        zero denominator is None.  ``bars_per_year`` (default ``252 * ep_len``) annualises the Sharpe ratios.

        * ``series``: mean / median return, mean / worst ``max_dd``, the longest drawdown in bars, mean / median
          of the per-series Sharpe ratio (from the piece's return, ``cum`` of a fresh ledger, and ``sumsq``;
          series with zero variance left out), and over all series' round trips the hit rate ``wins / trips``,
          the profit factor ``win_sum / |loss_sum|`` and the mean trip;
        * ``episodes``: mean / std / worst / share positive of the (series, full episode) returns;
        * ``portfolio`` (None without a curve): the equal-weight book ``curve / E``: total, max drawdown (peak
          from 0), Sharpe, and the return of every episode column with ``full`` telling the whole ones."""
        L = self.ledger
        if L is None:
            raise ValueError("report() needs a backtest made with ledger=True")
        bpy = float(252 * self.ep_len if bars_per_year is None else bars_per_year)
        n, steps = int(self.ret.numel()), int(self.steps)
        r = self.ret.double().cpu()
        mdd = L.max_dd.double().cpu()
        ssq = L.sumsq.double().cpu()
        sh = [v for v in (_sharpe(float(a), float(b), steps, bpy) for a, b in zip(r.tolist(), ssq.tolist()))
              if v is not None]
        trips, wins = int(L.trips.sum()), int(L.wins.sum())
        wsum, lsum = float(L.win_sum.double().sum()), float(L.loss_sum.double().sum())
        series = {"n": n, "ret_mean": float(r.sum()) / n, "ret_median": float(r.median()),
                  "max_dd_mean": float(mdd.sum()) / n, "max_dd_worst": float(mdd.max()),
                  "dd_bars_longest": int(L.dd_bars.max()),
                  "sharpe_mean": _div(sum(sh), len(sh)), "sharpe_median": float(np.median(sh)) if sh else None,
                  "trips": trips, "hit_rate": _div(wins, trips), "profit_factor": _div(wsum, abs(lsum)),
                  "trip_mean": _div(wsum + lsum, trips)}
        full = [k for k, f in enumerate(L.full) if f]
        episodes = _moments(L.ep_ret.double().cpu()[:, full].flatten())
        portfolio = None
        if L.curve is not None:
            c = L.curve.double().cpu() / n
            eq = torch.cumsum(c, 0)
            peak = torch.cummax(torch.clamp(eq, min=0.0), 0).values
            es0 = episode_columns(self.start, steps, self.origin, self.ep_len)[0]
            cols = []
            for k in range(len(L.full)):
                lo = max(es0 + k * self.ep_len, self.start) - self.start
                hi = min(es0 + (k + 1) * self.ep_len, self.start + steps) - self.start
                cols.append(float(c[lo:hi].sum()))
            portfolio = {"total": float(c.sum()), "max_dd": float((peak - eq).max()),
                         "sharpe": _sharpe(float(c.sum()), float((c * c).sum()), steps, bpy),
                         "episodes": cols, "full": list(L.full)}
        return {"bars_per_year": bpy, "series": series, "episodes": episodes, "portfolio": portfolio}


def result_from(out: Dict[str, torch.Tensor], start, steps, ep_len, origin, backend, trace,
                ledger: Optional[GruLedger] = None) -> GruBacktestResult:
    """The fields of :func:`reference_gru_rollout` / :func:`simulate_minute_actions` as a result object."""
    return GruBacktestResult(ret=out["ret"], trades=out["trades"], long=out["long"], position=out["position"],
                             entry=out["entry"], h=out.get("h"), start=int(start), steps=int(steps),
                             ep_len=int(ep_len), origin=int(origin), backend=backend,
                             actions=out["actions"] if trace else None,
                             q=out["q"] if trace else None, reward=out["reward"] if trace else None,
                             ledger=ledger)


def _run_dir(path: str) -> str:
    """A run's checkpoint directory: ``path`` itself, or rank 0's sub-directory of a data-parallel run
    (every rank holds the same model; ``trainer/runs.py`` writes ``<dir>/rank<r>/``)."""
    from ..persist.checkpoint import CheckpointManager

    sub = os.path.join(path, "rank0")
    return sub if not CheckpointManager(path).list() and os.path.isdir(sub) else path


def checkpoint_kind(path: str) -> Optional[str]:
    """``meta["kind"]`` of a ``.stck`` file or of the newest file of a ``CheckpointManager`` directory, read from
    the archive's header alone (a recurrent checkpoint carries its replay ring); None when there is none."""
    meta = checkpoint_meta(path)
    return None if meta is None else meta.get("kind")


def checkpoint_meta(path: str) -> Optional[dict]:
    """The meta dict of a ``.stck`` file or of the newest file of a ``CheckpointManager`` directory, read from the
    archive's header alone; None when there is none."""
    import json
    import struct

    from ..persist.checkpoint import CheckpointManager

    if os.path.isdir(path):
        path = _run_dir(path)
        files = CheckpointManager(path).list()
        if not files:
            return None
        path = os.path.join(path, files[-1])
    with open(path, "rb") as f:
        head = f.read(24)
        if len(head) < 24:
            return None
        _, _, meta_len = struct.unpack_from("<IIQ", head, 8)
        try:
            meta = json.loads(f.read(meta_len).decode() or "{}")
        except ValueError:
            return None
    return meta if isinstance(meta, dict) else None


class GruPolicy:
    """A frozen GRU(256) Q-net: the fp32 parameter tensors and (on a GPU) their packed form (``st_gru_pack``:
    MX-fp8 W_hh fragments, bf16 W_ih fragments, pre-scaled biases, W_q)."""

    def __init__(self, params: Dict[str, torch.Tensor], device: Optional[torch.device] = None, seed: int = 0,
                 epsilon: float = 0.9):
        dev = torch.device(device) if device is not None else \
            torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        self.device, self.seed, self.epsilon = dev, int(seed), float(epsilon)
        shapes = _shapes()
        self.params = {}
        for n in PARAM_NAMES:
            if n not in params:
                raise KeyError(f"GRU policy parameters lack {n!r}")
            t = params[n].detach().to(dev, torch.float32).reshape(shapes[n]).contiguous().clone()
            self.params[n] = t
        self.packed = None
        if dev.type == "cuda":
            self._pack()

    def _pack(self) -> None:
        from ..ops import native

        dev, i32 = self.device, torch.int32
        nfr = G.RW * 3 * 2 * 2 * 64
        with torch.cuda.device(dev):
            pk = {"whh8": torch.zeros(nfr * 8, dtype=i32, device=dev), "whhs": torch.zeros(nfr, dtype=i32, device=dev),
                  "wih": torch.zeros(G.RW * 6 * 64 * 8, dtype=torch.int16, device=dev),
                  "bias4": torch.zeros(4 * G.HID, device=dev), "wq": torch.zeros(4 * G.HID, device=dev)}
            p = G.PackArgs()
            for n in PARAM_NAMES:
                setattr(p, n, self.params[n].data_ptr())
            G.set_netw(p, pk)
            p.whhT8, p.whhTs = None, None
            native.check(G.lib().st_gru_pack(p, native.stream_handle()), "st_gru_pack")
        self.packed = pk

    # ---------------------------------------------------------------- constructors
    @classmethod
    def from_learner(cls, d, net: str = "online") -> "GruPolicy":
        """The learner's online or target net as it is now (a copy: later updates do not reach it)."""
        if net not in ("online", "target"):
            raise ValueError(f"net must be online/target, got {net!r}")
        flat = d.flat if net == "online" else d.tflat
        return cls(split_flat(flat), device=d.dev, seed=d.seed, epsilon=float(d.cfg.agent.epsilon))

    @classmethod
    def from_checkpoint(cls, path: str, net: str = "online", device=None) -> "GruPolicy":
        """From a ``CheckpointManager`` directory (its latest file; rank 0's of a data-parallel run) or one
        ``.stck`` of a ``recurrent`` run."""
        from ..persist.checkpoint import CheckpointManager, load

        if net not in ("online", "target"):
            raise ValueError(f"net must be online/target, got {net!r}")
        if os.path.isdir(path):
            path = _run_dir(path)
            latest = CheckpointManager(path).latest()
            if latest is None:
                raise FileNotFoundError(f"no checkpoint under {path}")
            path = latest
        state, meta = load(path)
        kind = meta.get("kind")
        if kind != "recurrent":
            raise ValueError(f"{path} is a checkpoint of a {kind!r} run; a GRU policy needs a 'recurrent' one")
        key = "flat" if net == "online" else "tflat"
        if key not in state:
            raise KeyError(f"{path} holds no {key!r} tensor")
        agent = (meta.get("config") or {}).get("agent") or {}
        return cls(split_flat(state[key]), device=device, seed=int(agent.get("seed", 0)),
                   epsilon=float(agent.get("epsilon", 0.9)))

    # ---------------------------------------------------------------- backtest
    def backtest(self, close: torch.Tensor, feat: torch.Tensor, *, start: int = 0, steps: Optional[int] = None,
                 ep_len: int = 390, cost: float = 0.01, origin: Optional[int] = None, greedy: bool = True,
                 epsilon: Optional[float] = None, h0: Optional[torch.Tensor] = None,
                 position: Optional[torch.Tensor] = None, entry: Optional[torch.Tensor] = None, trace: bool = False,
                 env_offset: int = 0, backend: str = "auto", grid: int = 0,
                 ret: Optional[torch.Tensor] = None, ledger: bool = False,
                 ledger_state: Optional[torch.Tensor] = None) -> GruBacktestResult:
        """Run the policy over bars ``start .. start + steps - 1`` (default: to the last bar with a next
        close) of ``close`` [E, T] fp32 and ``feat`` [E, T, 8] bf16, episodes of ``ep_len`` bars counted from
        ``origin`` (default ``start``).  ``greedy`` (default) takes the first maximum of Q; else the epsilon
        rule with ``epsilon`` (default the policy's own; 0 = uniform random).  ``h0`` [E, 256] fp32,
        ``position`` [E] int32 and ``entry`` [E] fp32 continue an earlier piece.  ``backend``: ``hip`` (one
        launch on the current stream), ``torch`` (:func:`reference_gru_rollout`) or ``auto``.  ``ret`` [E, T]
        fp32: ``minute_bars.bar_returns(close)`` when the caller already holds it (else computed here).
        ``ledger``: also keep the risk ledger (``result.ledger``, a :class:`GruLedger`; the kernel's ledger
        instance, nothing more is written per bar than one partial sum per 32 series); ``ledger_state`` [E, 8]
        int32 is ``ledger.state`` of the piece before."""
        if ledger_state is not None and not ledger:
            raise ValueError("ledger_state continues a ledger: pass ledger=True")
        if backend not in ("auto", "hip", "torch"):
            raise ValueError(f"backend must be auto/hip/torch, got {backend!r}")
        if backend == "auto":
            backend = "hip" if self.device.type == "cuda" else "torch"
        if close.dim() != 2 or feat.dim() != 3 or feat.shape[:2] != close.shape or feat.shape[2] != mb.NFEAT:
            raise ValueError("close must be [E, T] and feat [E, T, 8]")
        E, T = (int(v) for v in close.shape)
        start, steps, origin = _check_run(E, T, start, steps, ep_len, origin)
        eps = math.inf if greedy else float(self.epsilon if epsilon is None else epsilon)
        if backend == "torch":
            out = reference_gru_rollout(self.params, close.to(self.device), feat.to(self.device), start=start,
                                        steps=steps, ep_len=ep_len, cost=cost, origin=origin, epsilon=eps,
                                        seed=self.seed, h0=h0, position=position, entry=entry, env_offset=env_offset,
                                        ret=ret)
            led = ledger_from_trace(out["actions"], out["reward"], position=position, start=start, origin=origin,
                                    ep_len=ep_len, ledger_state=ledger_state) if ledger else None
            return result_from(out, start, steps, ep_len, origin, "torch", trace, led)
        return self._backtest_hip(close, feat, start, steps, ep_len, cost, origin, eps, h0, position, entry, trace,
                                  env_offset, grid, ret, ledger, ledger_state)

    def _backtest_hip(self, close, feat, start, steps, ep_len, cost, origin, eps, h0, position, entry, trace,
                      env_offset, grid, ret, ledger=False, ledger_state=None) -> GruBacktestResult:
        from ..ops import native

        if self.packed is None:
            raise RuntimeError("the hip backend needs a policy on a GPU")
        dev = self.device
        E, T = (int(v) for v in close.shape)
        if close.dtype != torch.float32 or close.device != dev or not close.is_contiguous():
            raise ValueError("close must be a contiguous fp32 [E, T] tensor on the policy's device")
        if feat.dtype != torch.bfloat16 or feat.device != dev or not feat.is_contiguous():
            raise ValueError("feat must be a contiguous bf16 [E, T, 8] tensor on the policy's device")
        for name, t, dt, shp in (("h0", h0, torch.float32, (E, G.HID)), ("position", position, torch.int32, (E,)),
                                 ("entry", entry, torch.float32, (E,)), ("ret", ret, torch.float32, (E, T)),
                                 ("ledger_state", ledger_state, torch.int32, (E, 8))):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shp or t.device != dev or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} device tensor of shape {shp}")
        with torch.cuda.device(dev):
            if ret is None:
                ret = mb.bar_returns(close)
            out = {"ret": torch.empty(E, device=dev), "trades": torch.empty(E, dtype=torch.int32, device=dev),
                   "long": torch.empty(E, dtype=torch.int32, device=dev),
                   "position": torch.empty(E, dtype=torch.int32, device=dev), "entry": torch.empty(E, device=dev),
                   "h": torch.empty(E, G.HID, device=dev)}
            if trace:
                out["actions"] = torch.empty(E, steps, dtype=torch.int8, device=dev)
                out["q"] = torch.empty(E, steps, 3, device=dev)
                out["reward"] = torch.empty(E, steps, device=dev)
            args = G.RolloutLedgerArgs() if ledger else G.RolloutArgs()
            a = args.r if ledger else args
            G.set_netw(a, self.packed)
            a.feat, a.close, a.ret = feat.data_ptr(), close.data_ptr(), ret.data_ptr()
            a.h0, a.position, a.entry = native.ptr(h0), native.ptr(position), native.ptr(entry)
            a.out_ret, a.out_trades, a.out_long = (out[k].data_ptr() for k in ("ret", "trades", "long"))
            a.out_position, a.out_entry, a.out_h = (out["position"].data_ptr(), out["entry"].data_ptr(),
                                                    out["h"].data_ptr())
            a.tr_actions, a.tr_q, a.tr_reward = (native.ptr(out.get(k)) for k in ("actions", "q", "reward"))
            a.E, a.T, a.start, a.steps, a.origin, a.ep_len = E, T, start, steps, origin, int(ep_len)
            a.eps, a.cost, a.inv_ep_len = eps, float(cost), float(np.float32(1.0 / ep_len))
            a.key0, a.key1 = (int(x) for x in rng.key_for(self.seed, KEY_RANK))
            a.env_offset = int(env_offset) & 0xFFFFFFFF
            if grid <= 0:
                grid = self._auto_grid(E)
            led = None
            if ledger:
                _, n_ep, full = episode_columns(start, steps, origin, int(ep_len))
                i32 = torch.int32
                stride = -(-steps // CHUNK) * CHUNK
                ep_ret, ep_trades = torch.empty(E, n_ep, device=dev), torch.empty(E, n_ep, dtype=i32, device=dev)
                state, stats = torch.empty(E, 8, dtype=i32, device=dev), torch.empty(E, 8, dtype=i32, device=dev)
                part, curve = torch.empty(-(-E // G.RN), stride, device=dev), torch.empty(steps, device=dev)
                l = args.l
                l.ep_ret, l.ep_trades, l.state_in = ep_ret.data_ptr(), ep_trades.data_ptr(), native.ptr(ledger_state)
                l.state_out, l.stats, l.part, l.curve = (t.data_ptr() for t in (state, stats, part, curve))
                l.n_ep, l.part_stride = n_ep, stride
                native.check(G.lib().st_gru_rollout_ledger_launch(C.byref(args), int(grid), native.stream_handle()),
                             "st_gru_rollout_ledger_launch")
                led = _ledger_of_records(ep_ret, ep_trades, stats, state, full, curve)
            else:
                native.check(G.lib().st_gru_rollout_launch(C.byref(a), int(grid), native.stream_handle()),
                             "st_gru_rollout_launch")
        return result_from(out, start, steps, ep_len, origin, "hip", trace, led)

    def _auto_grid(self, E: int) -> int:
        """Workgroups: one per 32-env chunk up to one per CU, then the fewest that finish the chunks in the same
        number of rounds (a workgroup loads the weights once for all its chunks)."""
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        work = -(-E // G.RN)
        rounds = -(-work // cus)
        return -(-work // rounds)
