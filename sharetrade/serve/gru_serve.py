"""Serving a trained GRU(256) policy: stateful sessions, one bar per launch (``csrc/gru_serve.hip``).

A recurrent policy cannot be served statelessly: the recurrent state ``h``, the position and the entry price
belong to a *session* and live on the GPU between requests.  A session is a slot of a device-resident table
(``h`` [S, 256] and one 64-byte scalar record per slot); a request names its session and brings the next minute
bar (8 features, close).  One launch advances any batch of sessions by one bar each, every session at its own
point of its own episode; the arithmetic of a bar is the backtest's (``csrc/gru_rollout.hip``), so serving T bars
one launch at a time gives what one rollout launch gives, bit for bit.

The next close is not known when a bar is served, so the reward of a bar is realised -- returned, and added to
the session's running return -- when the session's next bar arrives.

* :class:`GruSessionServer` owns the table and the weights (a :class:`GruPolicy`); ``step`` checks a batch on the
  host and launches it, ``step_into`` is the launch alone on preallocated device tensors.
* :func:`reference_gru_serve` is the same bar in PyTorch on the net arithmetic of ``reference_gru_rollout``: the
  ``torch`` backend and the oracle of the GPU tests.
* Raw bars: a session opened with ``open_raw`` also owns a feature-state row (``csrc/bar_features.h``), and
  ``step_raw`` / ``step_raw_into`` take the bar as a client observes it (open, high, low, close, volume, minute of
  the session): one featurise launch (``csrc/bar_features.hip`` bar_features_sessions_kernel) writes the rows'
  features and closes, then the unchanged serve launch runs on the same stream.
* :class:`GruBatcher` collects single requests of many client threads into batches with at most one request per
  session, so a session's bars are applied in submission order.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
import time
from concurrent.futures import Future
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ..data import minute_bars as mb
from ..ops import bar_features as BF
from ..ops import gru as G
from ..utils import rng
from .gru_rollout import KEY_RANK, TAG_ROLLOUT, GruBarNet, GruPolicy, rounding_points

REC = G.SERVE_REC_WORDS
COL = G.SERVE_REC_COLS
STATE_FIELDS = ("position", "entry", "elapsed", "ret", "trades", "long", "bars")


def new_table(S: int, device, h_dtype: torch.dtype = torch.float32) -> Dict[str, torch.Tensor]:
    """An empty session table: ``h`` [S, 256] and ``rec`` int32 [S, 16] (``ops.gru.ServeRec`` per row)."""
    return {"h": torch.zeros(S, G.HID, dtype=h_dtype, device=device),
            "rec": torch.zeros(S, REC, dtype=torch.int32, device=device)}


def rec_view(rec: torch.Tensor, name: str) -> torch.Tensor:
    """The named column of a ``rec`` tensor as a view [S] (float32 or int32 by the field's type)."""
    t = rec.view(torch.float32) if name in G.SERVE_REC_FLOAT else rec
    return t[:, COL[name]]


def serve_draws(seed: int, draw_ids: np.ndarray, bars: np.ndarray):
    """A served bar's Philox draws, counter (draw_id, bars served, 0, "GRB1") under the actors' key: the
    backtest's draws of env ``draw_id`` at bar ``bars``.  Returns (explore coin u0, random action u1)."""
    k0, k1 = rng.key_for(seed, KEY_RANK)
    n = draw_ids.shape[0]
    c0, c1, _, _ = rng.philox4x32(draw_ids.astype(np.uint32), bars.astype(np.uint32), np.zeros(n, np.uint32),
                                  np.full(n, TAG_ROLLOUT, np.uint32), np.full(n, k0), np.full(n, k1))
    return rng.u24(c0), rng.u24(c1)


def reference_gru_serve(params: Optional[Dict[str, torch.Tensor]], table: Dict[str, torch.Tensor],
                        slots: torch.Tensor, feat: torch.Tensor, close: torch.Tensor, *,
                        flags: Optional[torch.Tensor] = None, ep_len: int = 390, cost: float = 0.01,
                        epsilon: float = math.inf, seed: int = 0, emulate: Union[bool, Iterable[str]] = True,
                        dtype: torch.dtype = torch.float64, net: Optional[GruBarNet] = None
                        ) -> Dict[str, torch.Tensor]:
    """One served bar per request row in PyTorch; ``table`` (:func:`new_table`) is updated in place.

    ``slots`` [B] (a slot outside the table, e.g. -1, is a padding row: action -1, nothing touched), ``feat``
    [B, 8], ``close`` [B], ``flags`` [B] (bit 0: a new episode starts at this bar).  Returns ``actions`` int8,
    ``position`` int32 (after the action, before any end-of-episode flattening), ``reward`` fp32 (the realised
    reward of the session's previous bar) and ``q`` [B, 3].  The env is float32 in the kernel's operation
    order; the net is :class:`GruBarNet` (``emulate`` / ``dtype`` as in ``reference_gru_rollout``, or a
    prepared ``net``).  A table whose ``h`` is float64 carries the state unrounded between bars, as the
    rollout oracle does within one call."""
    h_t, rec = table["h"], table["rec"]
    dev = rec.device
    if net is None:
        net = GruBarNet(params, rounding_points(emulate), dtype, dev)
    dtype = net.dtype
    S = int(rec.shape[0])
    sl = torch.as_tensor(slots).to(dev).long().reshape(-1)
    B = int(sl.numel())
    ok = (sl >= 0) & (sl < S)
    idx = sl[ok]
    n = int(idx.numel())
    F = torch.as_tensor(feat).to(dev).float().reshape(B, mb.NFEAT)[ok]
    c = torch.as_tensor(close).to(dev, torch.float32).reshape(B)[ok]
    fresh = torch.zeros(n, dtype=torch.bool, device=dev) if flags is None else \
        (torch.as_tensor(flags).to(dev).reshape(B)[ok].to(torch.int32) & 1) != 0
    out = {"actions": torch.full((B,), -1, dtype=torch.int8, device=dev),
           "position": torch.zeros(B, dtype=torch.int32, device=dev),
           "reward": torch.zeros(B, dtype=torch.float32, device=dev),
           "q": torch.zeros(B, 3, dtype=torch.float32, device=dev)}
    if n == 0:
        return out
    R = rec[idx]
    Rf = R.view(torch.float32)
    zi, zf = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    one = torch.ones(n, dtype=torch.float32, device=dev)
    pz = torch.where(fresh, zi, R[:, COL["position"]])
    en = torch.where(fresh, zf, Rf[:, COL["entry"]])
    el = torch.where(fresh, zi, R[:, COL["elapsed"]])
    lc = torch.where(fresh, zf, Rf[:, COL["last_close"]])
    ppos, pfee = R[:, COL["pend_pos"]], Rf[:, COL["pend_fee"]]
    ret, ntr, nlong = Rf[:, COL["ret"]], R[:, COL["trades"]], R[:, COL["long"]]
    bars, draw = R[:, COL["bars"]], R[:, COL["draw_id"]]
    h = h_t[idx]
    h = (h if h.dtype == dtype else h.float()).to(dtype)
    h = torch.where(fresh[:, None], torch.zeros_like(h), h)
    # the realised reward of the previous bar
    has = lc > 0
    r = (c / torch.where(has, lc, one) - 1.0) * 100.0
    rew = torch.where(has, ppos.float() * r - pfee, zf)
    ret = torch.where(has, ret + rew, ret)
    # the bar
    held = pz != 0
    upnl = torch.where(held, (c / torch.where(held, en, one) - 1.0) * 100.0, zf)
    frac = el.float() * torch.tensor(float(np.float32(1.0 / ep_len)), dtype=torch.float32, device=dev)
    x = torch.cat([F, torch.stack([pz.float(), upnl, frac, one], dim=1)], dim=1)
    h, q = net.bar(x, h)
    a = torch.argmax(q, dim=1)   # first max on ties
    if not math.isinf(epsilon):
        u0, u1 = serve_draws(seed, draw.cpu().numpy().view(np.uint32), bars.cpu().numpy().view(np.uint32))
        exploit = torch.from_numpy(u0 < np.float32(epsilon)).to(dev)
        rnd = torch.from_numpy(np.minimum((u1 * np.float32(3)).astype(np.int64), 2)).to(dev)
        a = torch.where(exploit, a, rnd)
    a = a.to(torch.int32)
    np_ = torch.where(a == 0, torch.ones_like(pz), torch.where(a == 1, zi, pz))
    trade = np_ != pz
    en = torch.where(trade & (np_ == 1), c, en)
    done = (el + 1) >= int(ep_len)
    W = torch.zeros(n, REC, dtype=torch.int32, device=dev)
    Wf = W.view(torch.float32)
    W[:, COL["position"]] = torch.where(done, zi, np_)
    Wf[:, COL["entry"]] = torch.where(done, zf, en)
    W[:, COL["elapsed"]] = torch.where(done, zi, el + 1)
    Wf[:, COL["last_close"]] = c
    W[:, COL["pend_pos"]] = np_
    Wf[:, COL["pend_fee"]] = torch.where(trade, torch.full_like(zf, float(np.float32(cost))), zf)
    Wf[:, COL["ret"]] = ret
    W[:, COL["trades"]] = ntr + trade.int()
    W[:, COL["long"]] = nlong + np_
    W[:, COL["bars"]] = bars + 1
    W[:, COL["draw_id"]] = draw
    rec[idx] = W
    h_t[idx] = torch.where(done[:, None], torch.zeros_like(h), h).to(h_t.dtype)
    out["actions"][ok] = a.to(torch.int8)
    out["position"][ok] = np_
    out["reward"][ok] = rew
    out["q"][ok] = q
    return out


@dataclass
class GruDecision:
    """What a batch of served bars gave, one entry per request row."""

    actions: torch.Tensor              # [B] int8: 0 Buy, 1 Sell, 2 Hold; -1 on a padding row
    position: torch.Tensor             # [B] int32 after the action
    reward: torch.Tensor               # [B] fp32 realised reward of the session's previous bar
    q: Optional[torch.Tensor] = None   # [B, 3] fp32


ArrayLike = Union[torch.Tensor, np.ndarray, Sequence]


class GruSessionServer:
    """Sessions of a GRU(256) policy on one device: a table of ``max_sessions`` slots, ``open`` / ``close`` /
    ``step``.  ``backend``: ``hip`` (``csrc/gru_serve.hip``), ``torch`` (:func:`reference_gru_serve`, any
    device) or ``auto`` (``hip`` on a GPU).  Launches go to the caller's current stream; the table is one, so
    two streams stepping the same server must be ordered by the caller (the :class:`GruBatcher` owns a stream
    and is meant to be the only stepper while it runs)."""

    def __init__(self, policy: GruPolicy, max_sessions: int, ep_len: int = 390, cost: float = 0.01,
                 backend: str = "auto", bar_day: int = mb.BarParams.day, bar_alpha: float = mb.BarParams.alpha,
                 bar_beta: float = mb.BarParams.beta):
        if backend not in ("auto", "hip", "torch"):
            raise ValueError(f"backend must be auto/hip/torch, got {backend!r}")
        if backend == "auto":
            backend = "hip" if policy.device.type == "cuda" else "torch"
        if int(max_sessions) < 1 or int(ep_len) < 1:
            raise ValueError("need max_sessions >= 1 and ep_len >= 1")
        self.backend, self.device = backend, policy.device
        self.S, self.ep_len, self.cost = int(max_sessions), int(ep_len), float(cost)
        # the torch backend carries h unrounded (float64), as the rollout oracle does within one call
        self.table = new_table(self.S, self.device, torch.float32 if backend == "hip" else torch.float64)
        # raw-bar sessions: the feature state of a slot (ops.bar_features.STATE_FIELDS) and what the definition
        # needs beside it (data.ohlcv.FeatureParams: session length, GARCH coefficients)
        if int(bar_day) < 1:
            raise ValueError("need bar_day >= 1")
        self.bar_day, self.bar_alpha, self.bar_beta = int(bar_day), float(bar_alpha), float(bar_beta)
        self.fstate = torch.zeros(self.S, BF.NSTATE, dtype=torch.float32, device=self.device)
        self._raw = np.zeros(self.S, dtype=bool)
        self._raw_feat = self._raw_close = None
        self._open = np.zeros(self.S, dtype=bool)
        self._free: List[int] = list(range(self.S - 1, -1, -1))   # pop() hands out the lowest slot first
        self._lock = threading.Lock()   # one weight set per launch; the free list
        self.batches = 0
        self.bars_served = 0
        self._net = None
        self.load_policy(policy)

    # ---------------------------------------------------------------- weights
    def load_policy(self, policy: GruPolicy) -> None:
        """Swap the weights; every session keeps its state."""
        if policy.device != self.device:
            raise ValueError(f"the policy lives on {policy.device}, the sessions on {self.device}")
        if self.backend == "hip" and policy.packed is None:
            raise RuntimeError("the hip backend needs a policy on a GPU")
        with self._lock:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)   # launches already queued keep the old set alive
            self.policy = policy
            self.seed = policy.seed
            self._key = tuple(int(x) for x in rng.key_for(policy.seed, KEY_RANK))
            if self.backend == "torch":
                self._net = GruBarNet(policy.params, rounding_points(True), torch.float64, self.device)

    # ---------------------------------------------------------------- the table
    def view(self, name: str) -> torch.Tensor:
        """A named view of the table: ``h`` [S, 256] or a scalar field [S] (``ops.gru.ServeRec``)."""
        return self.table["h"] if name == "h" else rec_view(self.table["rec"], name)

    def open(self, n: int = 1, draw_ids: Optional[Sequence[int]] = None) -> List[int]:
        """Take ``n`` free slots, zero their table rows and set their ``draw_id`` (default: the slot index)."""
        n = int(n)
        if draw_ids is not None and len(draw_ids) != n:
            raise ValueError("one draw id per opened session")
        with self._lock:
            if n < 1 or n > len(self._free):
                raise RuntimeError(f"{n} sessions asked for, {len(self._free)} of {self.S} slots are free")
            slots = [self._free.pop() for _ in range(n)]
            ids = slots if draw_ids is None else [int(d) & 0xFFFFFFFF for d in draw_ids]
            idx = torch.tensor(slots, dtype=torch.long, device=self.device)
            row = torch.zeros(n, REC, dtype=torch.int64)
            row[:, COL["draw_id"]] = torch.tensor(ids, dtype=torch.int64)
            row = torch.where(row >= 2 ** 31, row - 2 ** 32, row).to(torch.int32)
            self.table["h"][idx] = 0
            self.table["rec"][idx] = row.to(self.device)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()   # zeroed before any stream can step them
            self._open[slots] = True
        return slots

    def open_raw(self, n: int, sigma, vol_scale, draw_ids: Optional[Sequence[int]] = None) -> List[int]:
        """:meth:`open` for sessions fed raw bars: also zeroes the slots' feature-state rows and sets their
        ``sigma`` and ``vol_scale`` (a scalar for all, or one per session; ``data.ohlcv.fit_feature_params``)."""
        n = int(n)
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (n,))
        vs = np.broadcast_to(np.asarray(vol_scale, dtype=np.float32), (n,))
        if not (np.all(np.isfinite(sg)) and np.all(sg > 0) and np.all(np.isfinite(vs)) and np.all(vs > 0)):
            raise ValueError("sigma and vol_scale must be positive")
        slots = self.open(n, draw_ids)
        row = np.zeros((n, BF.NSTATE), np.float32)
        row[:, BF.STATE_COL["sigma"]], row[:, BF.STATE_COL["vol_scale"]] = sg, vs
        with self._lock:
            idx = torch.tensor(slots, dtype=torch.long, device=self.device)
            self.fstate[idx] = torch.from_numpy(row).to(self.device)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()
            self._raw[slots] = True
        return slots

    def is_raw(self, slot: int) -> bool:
        return self.is_open(slot) and bool(self._raw[int(slot)])

    def _check_raw(self, s: np.ndarray) -> None:
        if not bool(self._raw[s].all()):
            raise ValueError(f"session {int(s[~self._raw[s]][0])} was opened without raw-bar state (open_raw)")

    def close(self, slots: Union[int, Sequence[int]]) -> None:
        s = self._host_slots(slots)
        with self._lock:
            self._check_open(s)
            self._open[s] = False
            self._raw[s] = False
            self._free.extend(int(v) for v in s[::-1])

    def _host_slots(self, slots) -> np.ndarray:
        if isinstance(slots, torch.Tensor):
            slots = slots.detach().cpu().numpy()
        return np.atleast_1d(np.asarray(slots)).astype(np.int64).reshape(-1)

    def _check_open(self, s: np.ndarray) -> None:
        if s.size == 0:
            raise ValueError("an empty batch")
        if int(s.min()) < 0 or int(s.max()) >= self.S:
            raise ValueError(f"slot outside 0 .. {self.S - 1}")
        if not bool(self._open[s].all()):
            raise ValueError(f"slot {int(s[~self._open[s]][0])} is not open")
        if np.unique(s).size != s.size:
            raise ValueError("a slot appears twice in the batch (a session takes one bar per launch)")

    def is_open(self, slot: int) -> bool:
        return 0 <= int(slot) < self.S and bool(self._open[int(slot)])

    def state(self, slots: Union[int, Sequence[int]]) -> Dict[str, torch.Tensor]:
        """Copies of the sessions' state: ``h`` [n, 256] fp32 and the scalar fields [n]."""
        s = self._host_slots(slots)
        self._check_open(s)
        idx = torch.from_numpy(s).to(self.device)
        out = {"h": self.table["h"][idx].float()}
        for k in STATE_FIELDS:
            out[k] = self.view(k)[idx].clone()
        return out

    # ---------------------------------------------------------------- stepping
    def _eps(self, greedy: bool, epsilon: Optional[float]) -> float:
        return math.inf if greedy else float(self.policy.epsilon if epsilon is None else epsilon)

    def step(self, slots: ArrayLike, feat: ArrayLike, close: ArrayLike, new_episode: Optional[ArrayLike] = None,
             greedy: bool = True, epsilon: Optional[float] = None, return_q: bool = False,
             grid: int = 0) -> GruDecision:
        """One bar for each session of ``slots`` [B]: ``feat`` [B, 8], ``close`` [B] and ``new_episode`` [B]
        (bool) as host or device arrays.  Raises ``ValueError`` before anything is launched when a slot is out
        of range, not open, or named twice.  The decision's tensors live on the server's device."""
        s = self._host_slots(slots)
        with self._lock:
            self._check_open(s)
        B, dev = int(s.size), self.device
        F = torch.as_tensor(feat)
        F = (F if F.dtype == torch.bfloat16 else F.float().to(torch.bfloat16)).reshape(-1, mb.NFEAT)
        c = torch.as_tensor(close).to(torch.float32).reshape(-1)
        if F.shape[0] != B or c.numel() != B:
            raise ValueError("one feature row [8] and one close per slot")
        fl = None
        if new_episode is not None:
            fl = torch.as_tensor(new_episode).reshape(-1).to(torch.uint8).to(dev).contiguous()
            if fl.numel() != B:
                raise ValueError("one new_episode flag per slot")
        out = GruDecision(actions=torch.empty(B, dtype=torch.int8, device=dev),
                          position=torch.empty(B, dtype=torch.int32, device=dev),
                          reward=torch.empty(B, dtype=torch.float32, device=dev),
                          q=torch.empty(B, 3, dtype=torch.float32, device=dev) if return_q else None)
        self.step_into(torch.from_numpy(s.astype(np.int32)).to(dev), F.to(dev).contiguous(), c.to(dev).contiguous(),
                       fl, out.actions, out.position, out.reward, out.q, epsilon=self._eps(greedy, epsilon), grid=grid)
        return out

    def step_into(self, slots: torch.Tensor, feat: torch.Tensor, close: torch.Tensor, flags: Optional[torch.Tensor],
                  actions: torch.Tensor, position: torch.Tensor, reward: torch.Tensor,
                  q: Optional[torch.Tensor] = None, *, epsilon: float = math.inf, grid: int = 0) -> None:
        """The launch alone on device tensors and preallocated outputs, on the current stream: no host check,
        no sync, no allocation.  ``slots`` int32 [B] (-1 = a padding row; the caller guarantees the others are
        open and distinct), ``feat`` bf16 [B, 8], ``close`` fp32 [B], ``flags`` uint8 [B] or None; ``actions``
        int8, ``position`` int32, ``reward`` fp32 [>= B] and ``q`` fp32 [>= B, 3] or None.  ``epsilon = inf`` is
        greedy (no draws)."""
        B = int(slots.shape[0])
        for name, t, dt, k in (("slots", slots, torch.int32, 1), ("feat", feat, torch.bfloat16, mb.NFEAT),
                               ("close", close, torch.float32, 1), ("flags", flags, torch.uint8, 1),
                               ("actions", actions, torch.int8, 1), ("position", position, torch.int32, 1),
                               ("reward", reward, torch.float32, 1), ("q", q, torch.float32, 3)):
            if t is None and name in ("flags", "q"):
                continue
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() < B * k:
                raise ValueError(f"{name} must be a contiguous {dt} tensor of at least {B * k} values on "
                                 f"{self.device}")
        if B < 1:
            raise ValueError("an empty batch")
        with self._lock:
            self.batches += 1
            self.bars_served += B
            if self.backend == "torch":
                o = reference_gru_serve(None, self.table, slots, feat, close, flags=flags, ep_len=self.ep_len,
                                        cost=self.cost, epsilon=epsilon, seed=self.seed, net=self._net)
                actions[:B], position[:B], reward[:B] = o["actions"], o["position"], o["reward"]
                if q is not None:
                    q[:B] = o["q"]
                return
            self._launch(B, slots, feat, close, flags, actions, position, reward, q, epsilon, grid)

    # ---------------------------------------------------------------- stepping on raw bars
    def step_raw(self, slots: ArrayLike, ohlcv: ArrayLike, minute: ArrayLike,
                 new_episode: Optional[ArrayLike] = None, greedy: bool = True, epsilon: Optional[float] = None,
                 return_q: bool = False, grid: int = 0) -> GruDecision:
        """:meth:`step` on bars as a client observes them: ``ohlcv`` [B, 5] (open, high, low, close, volume) and
        ``minute`` [B] (the bar's index within its session, 0 .. bar_day - 1).  Also raises ``ValueError`` before
        anything is launched for a session that was opened without raw-bar state, a non-positive price or a
        minute out of range."""
        s = self._host_slots(slots)
        with self._lock:
            self._check_open(s)
            self._check_raw(s)
        B, dev = int(s.size), self.device
        x = torch.as_tensor(ohlcv).detach().to("cpu", torch.float32).reshape(-1, 5)
        m = torch.as_tensor(minute).detach().to("cpu").reshape(-1).to(torch.int32)
        if x.shape[0] != B or m.numel() != B:
            raise ValueError("one bar [5] and one minute per slot")
        if not bool(torch.isfinite(x).all()) or bool((x[:, :4] <= 0).any()) or bool((x[:, 4] < 0).any()):
            raise ValueError("a bar needs finite values, positive prices and a non-negative volume")
        if bool((m < 0).any()) or bool((m >= self.bar_day).any()):
            raise ValueError(f"minute outside 0 .. {self.bar_day - 1}")
        fl = None
        if new_episode is not None:
            fl = torch.as_tensor(new_episode).reshape(-1).to(torch.uint8).to(dev).contiguous()
            if fl.numel() != B:
                raise ValueError("one new_episode flag per slot")
        out = GruDecision(actions=torch.empty(B, dtype=torch.int8, device=dev),
                          position=torch.empty(B, dtype=torch.int32, device=dev),
                          reward=torch.empty(B, dtype=torch.float32, device=dev),
                          q=torch.empty(B, 3, dtype=torch.float32, device=dev) if return_q else None)
        self.step_raw_into(torch.from_numpy(s.astype(np.int32)).to(dev), x.to(dev).contiguous(),
                           m.to(dev).contiguous(), fl, out.actions, out.position, out.reward, out.q,
                           epsilon=self._eps(greedy, epsilon), grid=grid)
        return out

    def step_raw_into(self, slots: torch.Tensor, ohlcv: torch.Tensor, minute: torch.Tensor,
                      flags: Optional[torch.Tensor], actions: torch.Tensor, position: torch.Tensor,
                      reward: torch.Tensor, q: Optional[torch.Tensor] = None, *, epsilon: float = math.inf,
                      grid: int = 0, feat: Optional[torch.Tensor] = None,
                      close: Optional[torch.Tensor] = None) -> None:
        """:meth:`step_into` on raw bars: the featurise launch, then the serve launch, on the current stream; no
        host check, no sync.  ``ohlcv`` fp32 [B, 5], ``minute`` int32 [B]; the caller guarantees that the slots
        other than -1 are open raw sessions.  ``feat`` bf16 [>= B, 8] and ``close`` fp32 [>= B] receive the rows
        the serve launch reads (default: the server's own scratch, grown when a larger batch comes)."""
        B = int(slots.shape[0])
        if B < 1:
            raise ValueError("an empty batch")
        for name, t, dt, k in (("slots", slots, torch.int32, 1), ("ohlcv", ohlcv, torch.float32, 5),
                               ("minute", minute, torch.int32, 1)):
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() < B * k:
                raise ValueError(f"{name} must be a contiguous {dt} tensor of at least {B * k} values on "
                                 f"{self.device}")
        if feat is None or close is None:
            if self._raw_feat is None or self._raw_feat.shape[0] < B:
                self._raw_feat = torch.zeros(B, mb.NFEAT, dtype=torch.bfloat16, device=self.device)
                self._raw_close = torch.zeros(B, dtype=torch.float32, device=self.device)
            feat, close = self._raw_feat, self._raw_close
        if (feat.dtype != torch.bfloat16 or close.dtype != torch.float32 or feat.device != self.device
                or close.device != self.device or not feat.is_contiguous() or not close.is_contiguous()
                or feat.numel() < B * mb.NFEAT or close.numel() < B):
            raise ValueError("feat must be bf16 [>= B, 8] and close fp32 [>= B], contiguous, on the server's device")
        if self.backend == "torch":
            self._featurise_torch(B, slots, ohlcv, minute, feat, close)
        else:
            from ..ops import native

            a = BF.BarSessionsArgs(slots.data_ptr(), ohlcv.data_ptr(), minute.data_ptr(), self.fstate.data_ptr(),
                                   feat.data_ptr(), close.data_ptr(), B, self.S, self.bar_day, self.bar_alpha,
                                   self.bar_beta)
            with torch.cuda.device(self.device):
                native.check(BF.lib().st_bar_features_sessions(C.byref(a), native.stream_handle()),
                             "st_bar_features_sessions")
        self.step_into(slots, feat.view(-1, mb.NFEAT)[:B], close.view(-1)[:B], flags, actions, position, reward, q,
                       epsilon=epsilon, grid=grid)

    def _featurise_torch(self, B, slots, ohlcv, minute, feat, close) -> None:
        """The featurise launch on the host: ``data.ohlcv.featurise_numpy`` on one bar per valid row."""
        from ..data import ohlcv as ov

        sl = slots[:B].long()
        ok = (sl >= 0) & (sl < self.S)
        idx = sl[ok]
        if int(idx.numel()) == 0:
            return
        st = self.fstate[idx].cpu().numpy()
        x = ohlcv.view(-1, 5)[:B][ok].cpu().numpy()
        bars = ov.Bars(*(np.ascontiguousarray(x[:, k:k + 1]) for k in range(5)),
                       minute=minute[:B][ok].cpu().numpy().astype(np.int64)[:, None])
        fp = ov.FeatureParams(self.bar_day, self.bar_alpha, self.bar_beta, st[:, BF.STATE_COL["sigma"]],
                              st[:, BF.STATE_COL["vol_scale"]])
        r = ov.featurise_numpy(bars, fp, state=st)
        self.fstate[idx] = torch.from_numpy(r.state).to(self.device)
        okc = ok.to(feat.device)
        feat.view(-1, mb.NFEAT)[:B][okc] = torch.from_numpy(r.feat[:, 0]).to(torch.bfloat16).to(feat.device)
        close.view(-1)[:B][okc] = torch.from_numpy(r.close[:, 0]).to(close.device)

    def _launch(self, B, slots, feat, close, flags, actions, position, reward, q, epsilon, grid) -> None:
        from ..ops import native

        a = G.ServeArgs()
        G.set_netw(a, self.policy.packed)
        a.slot, a.feat, a.close, a.flags = slots.data_ptr(), feat.data_ptr(), close.data_ptr(), native.ptr(flags)
        a.h, a.rec = self.table["h"].data_ptr(), self.table["rec"].data_ptr()
        a.action, a.position, a.reward, a.q = (actions.data_ptr(), position.data_ptr(), reward.data_ptr(),
                                               native.ptr(q))
        a.B, a.S, a.ep_len = B, self.S, self.ep_len
        a.eps, a.cost, a.inv_ep_len = float(epsilon), self.cost, float(np.float32(1.0 / self.ep_len))
        a.key0, a.key1 = self._key
        with torch.cuda.device(self.device):
            native.check(G.lib().st_gru_serve_launch(C.byref(a), int(grid), native.stream_handle()),
                         "st_gru_serve_launch")


class GruBatcher:
    """Collects single bars from client threads into :class:`GruSessionServer` batches.

    ``submit`` returns a ``Future`` resolving to ``(action, position, reward)``.  A batch closes at
    ``max_batch`` requests or ``max_delay_us`` after its first request, and holds at most one request per
    session: a second bar of a session waits for the next batch, so a session's bars are applied in submission
    order.  The hip path stages rows in pinned host memory and steps on its own stream."""

    def __init__(self, server: GruSessionServer, max_batch: int = 4096, max_delay_us: float = 200.0):
        self.server = server
        self.max_batch = int(max_batch)
        self.max_delay = float(max_delay_us) * 1e-6
        self._cv = threading.Condition()
        # (slot, features [8] | ohlcv [5], close | minute, new_episode, future, raw)
        self._q: List[Tuple[int, np.ndarray, float, bool, Future, bool]] = []
        self._stop = False
        self.batch_sizes: List[int] = []
        self._native = server.backend == "hip"
        if self._native:
            dev, n = server.device, self.max_batch
            pin = dict(pin_memory=True)
            self._h = {"slot": torch.empty(n, dtype=torch.int32, **pin),
                       "feat": torch.empty(n, mb.NFEAT, dtype=torch.bfloat16, **pin),
                       "close": torch.empty(n, dtype=torch.float32, **pin),
                       "flags": torch.empty(n, dtype=torch.uint8, **pin),
                       "ohlcv": torch.empty(n, 5, dtype=torch.float32, **pin),
                       "minute": torch.empty(n, dtype=torch.int32, **pin),
                       "act": torch.empty(n, dtype=torch.int8, **pin),
                       "pos": torch.empty(n, dtype=torch.int32, **pin),
                       "rew": torch.empty(n, dtype=torch.float32, **pin)}
            self._d = {k: torch.empty_like(t, device=dev) for k, t in self._h.items()}
            self._stream = torch.cuda.Stream(dev)
        self._thread = threading.Thread(target=self._loop, name="sharetrade-gru-batcher", daemon=True)
        self._thread.start()

    def submit(self, slot: int, feat8: ArrayLike, close: float, new_episode: bool = False) -> Future:
        row = np.asarray(feat8.float().cpu() if isinstance(feat8, torch.Tensor) else feat8,
                         dtype=np.float32).reshape(-1)
        if row.size != mb.NFEAT:
            raise ValueError(f"a bar holds {mb.NFEAT} features, got {row.size}")
        if not self.server.is_open(slot):
            raise ValueError(f"session {slot} is not open")
        fut: Future = Future()
        with self._cv:
            if self._stop:
                raise RuntimeError("batcher is closed")
            self._q.append((int(slot), row, float(close), bool(new_episode), fut, False))
            self._cv.notify()
        return fut

    def submit_raw(self, slot: int, ohlcv5: ArrayLike, minute: int, new_episode: bool = False) -> Future:
        """:meth:`submit` of a raw bar (open, high, low, close, volume; ``minute`` of its session) to a session
        opened with ``open_raw``.  Raw and featurised bars go in separate batches, each session's in order."""
        row = np.asarray(ohlcv5.float().cpu() if isinstance(ohlcv5, torch.Tensor) else ohlcv5,
                         dtype=np.float32).reshape(-1)
        if row.size != 5:
            raise ValueError(f"a raw bar holds open, high, low, close, volume, got {row.size} values")
        if not np.all(np.isfinite(row)) or np.any(row[:4] <= 0) or row[4] < 0:
            raise ValueError("a bar needs finite values, positive prices and a non-negative volume")
        if not 0 <= int(minute) < self.server.bar_day:
            raise ValueError(f"minute outside 0 .. {self.server.bar_day - 1}")
        if not self.server.is_open(slot):
            raise ValueError(f"session {slot} is not open")
        if not self.server.is_raw(slot):
            raise ValueError(f"session {slot} was opened without raw-bar state (open_raw)")
        fut: Future = Future()
        with self._cv:
            if self._stop:
                raise RuntimeError("batcher is closed")
            self._q.append((int(slot), row, int(minute), bool(new_episode), fut, True))
            self._cv.notify()
        return fut

    def close(self) -> None:
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join()

    def __enter__(self) -> "GruBatcher":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def _take(self):
        with self._cv:
            while not self._q and not self._stop:
                self._cv.wait()
            if not self._q:
                return []
            deadline = time.perf_counter() + self.max_delay
            while len(self._q) < self.max_batch and not self._stop:
                left = deadline - time.perf_counter()
                if left <= 0:
                    break
                self._cv.wait(left)
            # the first request of each session, in order; a session's later requests wait (in order); a batch
            # holds bars of one kind (the first request's), and a session with a deferred bar defers its later ones
            batch, rest, seen = [], [], set()
            raw = self._q[0][5]
            for item in self._q:
                if item[0] in seen or len(batch) >= self.max_batch or item[5] != raw:
                    rest.append(item)
                    seen.add(item[0])
                else:
                    seen.add(item[0])
                    batch.append(item)
            self._q = rest
            return batch

    def _loop(self) -> None:
        while True:
            batch = self._take()
            if not batch:
                return
            try:
                acts, pos, rew = self._run(batch)
            except BaseException as e:  # noqa: BLE001 -- every waiting client gets the error
                for item in batch:
                    item[4].set_exception(e)
                continue
            self.batch_sizes.append(len(batch))
            for item, a, p, r in zip(batch, acts, pos, rew):
                item[4].set_result((int(a), int(p), float(r)))

    def _run(self, batch):
        n = len(batch)
        slots = np.asarray([b[0] for b in batch], dtype=np.int32)
        fl = np.asarray([b[3] for b in batch], dtype=np.uint8)
        srv = self.server
        if batch[0][5]:
            return self._run_raw(batch, n, slots, fl)
        F = torch.from_numpy(np.stack([b[1] for b in batch])).to(torch.bfloat16)
        c = np.asarray([b[2] for b in batch], dtype=np.float32)
        if not self._native:
            d = srv.step(slots, F, c, new_episode=fl)
            return d.actions.cpu().numpy(), d.position.cpu().numpy(), d.reward.cpu().numpy()
        with srv._lock:
            srv._check_open(slots.astype(np.int64))   # a session closed since its submit fails the batch
        h, d = self._h, self._d
        h["slot"][:n].numpy()[:] = slots
        h["feat"][:n].copy_(F)
        h["close"][:n].numpy()[:] = c
        h["flags"][:n].numpy()[:] = fl
        with torch.cuda.stream(self._stream):
            for k in ("slot", "feat", "close", "flags"):
                d[k][:n].copy_(h[k][:n], non_blocking=True)
            srv.step_into(d["slot"][:n], d["feat"][:n], d["close"][:n], d["flags"][:n], d["act"], d["pos"], d["rew"])
            for k in ("act", "pos", "rew"):
                h[k][:n].copy_(d[k][:n], non_blocking=True)
        self._stream.synchronize()
        return h["act"][:n].numpy().copy(), h["pos"][:n].numpy().copy(), h["rew"][:n].numpy().copy()

    def _run_raw(self, batch, n, slots, fl):
        x = np.stack([b[1] for b in batch]).astype(np.float32)
        m = np.asarray([b[2] for b in batch], dtype=np.int32)
        srv = self.server
        if not self._native:
            d = srv.step_raw(slots, x, m, new_episode=fl)
            return d.actions.cpu().numpy(), d.position.cpu().numpy(), d.reward.cpu().numpy()
        with srv._lock:
            srv._check_open(slots.astype(np.int64))   # a session closed since its submit fails the batch
            srv._check_raw(slots.astype(np.int64))
        h, d = self._h, self._d
        h["slot"][:n].numpy()[:] = slots
        h["ohlcv"][:n].numpy()[:] = x
        h["minute"][:n].numpy()[:] = m
        h["flags"][:n].numpy()[:] = fl
        with torch.cuda.stream(self._stream):
            for k in ("slot", "ohlcv", "minute", "flags"):
                d[k][:n].copy_(h[k][:n], non_blocking=True)
            srv.step_raw_into(d["slot"][:n], d["ohlcv"][:n], d["minute"][:n], d["flags"][:n], d["act"], d["pos"],
                              d["rew"], feat=d["feat"], close=d["close"])
            for k in ("act", "pos", "rew"):
                h[k][:n].copy_(d[k][:n], non_blocking=True)
        self._stream.synchronize()
        return h["act"][:n].numpy().copy(), h["pos"][:n].numpy().copy(), h["rew"][:n].numpy().copy()

    def stats(self) -> Dict[str, float]:
        bs = self.batch_sizes
        return {"batches": len(bs), "requests": int(sum(bs)), "mean_batch": float(np.mean(bs)) if bs else 0.0,
                "max_batch": int(max(bs)) if bs else 0}
