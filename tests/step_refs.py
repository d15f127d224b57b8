"""Float64 reference of one fused engine step, exact-case builders and comparisons for the bf16 step kernels
(csrc/qstep_ws.hip, csrc/qstep_wide.hip, csrc/qstep_fused.hip and the target pass csrc/qtarget.hip).  No GPU; numpy.

tests/test_gpu_step_exact.py launches the cases on the GPU and compares with this model through the ``check_*``
functions below; tests/test_step_refs.py ties the model to the torch oracle (``engine_step_ref``) bit for bit and runs
the model with one mutation at a time through the same functions (> 0 differences each).

The model rounds where the kernels round (``qn.forward`` / ``qn.backward`` with ``emulate_bf16=True``; the scalar
rule of csrc/trade_rule.h op by op in fp32) and adds what the oracle lacks: the tick bank, the statistics row, the
static chunk schedule, the per-workgroup slabs in both formats and the reduce.

Exact cases: every operand is a small dyadic number, so every dot product of the forward, the backward, the weight
gradient sums, the reduce and the statistics needs fewer than 24 bits.  fp32 arithmetic is then exact in any order:
the summation order inside the MFMAs, the k permutation of the ws kernel, the per-tile grouping and the schedule
cannot show, and a kernel must equal the model bit for bit.  ``exact_bits`` measures the bits per sum on the case
itself (sum |terms| over the largest power of two dividing every term); ``make_case`` raises when one reaches 24."""
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from gemm_refs import bf16_rne, bf16_round64, bf16_trunc, bf16_val
from sharetrade.models import qnet as qn
from sharetrade.utils import rng as strng

F = np.float32
H = 201
NSTAT = 8
STAT_NAMES = ("reward_sum", "loss_sum", "explore", "episodes_done", "final_sum", "final_sq", "qslot_sum", "_")
STATE_KEYS = ("budget", "shares", "value", "pos", "episodes", "last_final", "ret_sum")
LIMIT_BITS = 24.0

MUTATIONS = (
    "win_first_late", "win_last_late", "win_last_dropped", "xn_tail_old", "shares_next_price", "no_bias_col",
    "tie_last", "next_tie_last", "next_first", "u2_explore", "thr_no_min", "no_env_offset", "gamma_on_reward",
    "scale_stored_reward", "clip_after_coef", "dq_unrounded", "relu_mask_ge", "no_out_relu_mask", "db_tile_dropped",
    "slab_trunc", "slab_row_next", "slab_block_shift4", "no_reset", "loss_from_clipped")


def r32(x):
    """One fp32 rounding of a float64 value (the kernels' ``__f*_rn`` points)."""
    return np.asarray(x, np.float64).astype(F).astype(np.float64)


LAYOUT = qn.QNetLayout(H + 2, [128, 128], 3)   # the flagship's 203 -> 128 -> 128 -> 3, padded (224, 128, 128, 16)


def _w(flat, l):
    s = LAYOUT.segments[f"W{l}"]
    return flat[s.offset:s.offset + s.numel].reshape(s.shape)


def _b(flat, l):
    s = LAYOUT.segments[f"b{l}"]
    return flat[s.offset:s.offset + s.numel]


def real_mask() -> np.ndarray:
    """Entries of the flat layout that are parameters (weights and biases, no padding).  The kernels' slabs are
    compared on these: their pad entries are unspecified (csrc/optim.hip: "padding entries of the 64-env-chunk
    kernel's slabs are not zero" -- the ws kernel keeps dQ in four pad slots of the X row, so pad columns 204..207 of
    its dW0 hold dZ1^T dQ, and the pad action rows of its dW2 hold products with whatever follows dQ there).  The slab
    pass multiplies by the trainable mask, so the reduced gradient is compared on every entry: pads exactly 0."""
    return LAYOUT.trainable_mask(True).numpy().astype(bool)


# ----------------------------------------------------------------------------- case
@dataclass
class Case:
    name: str
    prices: np.ndarray                 # [E, T] fp32
    state: Dict[str, np.ndarray]       # STATE_KEYS
    params: np.ndarray                 # flat fp32
    knobs: Dict[str, object]
    target: Optional[np.ndarray] = None   # flat fp32 target net (knob build)
    pinned: Optional[np.ndarray] = None   # tie cases: per env, the action it must take when it exploits
    notes: Dict[str, object] = field(default_factory=dict)

    @property
    def E(self):
        return self.prices.shape[0]

    @property
    def T(self):
        return self.prices.shape[1]


def default_knobs(**kw):
    k = dict(feature_mode="relative", budget0=4096.0, shares0=0, compat=False, gamma=0.5, epsilon=0.5, ramp=64.0,
             seed=1234, step=5, loss_coef=2.0 / 256, env_offset=0, reward_mode="absolute", td_clip=0.0,
             double_dqn=False, reward_scale=1.0, ramp_global=False)
    k.update(kw)
    # "compat" is the reference's quirk set as the step tests use it: decisions from the constructor budget /
    # shares, the trained slot = argmax Q(x'), and an output ReLU
    k.setdefault("output_relu", bool(k["compat"]))
    return k


def tick_bank(prices):
    """(ticks [E, T] as float64 integers, scale [E]): every row on the coarsest power-of-two grid that keeps its
    ticks at or below 65,535, as csrc/series.hip tick16 chooses it; raises when a price is off that grid."""
    p = np.asarray(prices, np.float64)
    x = np.frexp(p.max(axis=1))[1].astype(np.int64) - 16
    x = np.where(np.ldexp(p.max(axis=1), -x) > 65535.0, x + 1, x)
    t = np.ldexp(p, -x[:, None])
    assert np.all(t == np.rint(t)) and t.min() >= 1 and t.max() <= 65535, "bank off the 16-bit tick grid"
    return t, np.ldexp(1.0, x)


# ----------------------------------------------------------------------------- the network in float64
class Rounder:
    """bf16 round-to-nearest-even at the kernels' rounding points; counts what rounded and what was an exact tie.
    ``flip``: a numpy Generator -- every value that comes with a ``delta`` (the counted fp32 error of the sum or of
    the scalar chain it comes from) is nudged by +- that delta before it rounds, so a value within its own error of
    a rounding boundary lands on either side (the flip-noise runs of the bounded case).  Weights come without a
    delta: their rounding is one conversion of an fp32 parameter, the same everywhere."""

    def __init__(self, on=True, flip=None):
        self.on, self.flip, self.counts = on, flip, {}

    def __call__(self, x, tag=None, delta=None):
        if not self.on:
            return x
        x = np.asarray(x, np.float64)
        if self.flip is not None and delta is not None:
            return bf16_round64(x + delta * self.flip.choice((-1.0, 1.0), size=x.shape) * (x != 0))
        y = bf16_round64(x)
        if tag is not None:
            _, e = np.frexp(x)
            half = np.ldexp(1.0, np.maximum(e, -125) - 9)
            c = self.counts.setdefault(tag, [0, 0])
            c[0] += int((y != x).sum())
            c[1] += int(((np.abs(y - x) == half) & (x != 0)).sum())
        return y


U23 = 2.0 ** -23   # twice the fp32 round-to-nearest unit: the rounding of the MFMA's internal adds is not specified


def pad_input(x):
    xp = np.zeros((x.shape[0], LAYOUT.in_p))
    xp[:, :H + 2] = x
    xp[:, LAYOUT.bias_col] = 1.0
    return xp


def forward(flat, x, output_relu, R, tag=""):
    """(q [E, 16], [H1, H2], xp) with the rounding points of qn.forward(emulate_bf16=True).  ``R.last_qerr`` is left
    holding the counted fp32 error of the last layer's sums, per env and output (the flip runs use it for dQ)."""
    flat = np.asarray(flat, np.float64)
    xin = pad_input(x)
    xp = R(xin, tag + "X", U23 * 2 * (np.abs(xin) + 1.0))   # (w * inv - 1: two fp32 roundings of values near 1)
    a, acts = xp, []
    for l in range(3):
        w = R(_w(flat, l))
        z = a @ w.T
        mag = np.abs(a) @ np.abs(w).T
        if l > 0:
            z = z + _b(flat, l)
            mag = mag + np.abs(_b(flat, l))
        err = (a.shape[1] + 2) * U23 * mag
        if l < 2:
            a = R(np.maximum(z, 0.0), tag + f"H{l + 1}", err)
            acts.append(a)
        else:
            q = np.maximum(z, 0.0) if output_relu else z
            R.last_qerr = err
    return q, acts, xp


def argmax_first(q):
    """csrc/trade_rule.h argmax3: strictly-greater updates, so the first index wins a tie."""
    return np.argmax(q[:, :3], axis=1)


def argmax_last(q):
    return 2 - np.argmax(q[:, 2::-1], axis=1)


# ----------------------------------------------------------------------------- features and the trading rule
def gather(c: Case, bank="fp32"):
    """Windows [E, H + 1] (columns 0..H-1 are x's window, 1..H the window of x'), in the bank's own units, and the
    per-env unit (1 for the fp32 bank, the tick size for the tick bank)."""
    pos = c.state["pos"].astype(np.int64)
    idx = pos[:, None] + np.arange(H + 1)[None, :]
    if bank == "ticks":
        assert c.knobs["feature_mode"] == "relative", "the kernels read the tick bank for relative features only"
        t, sc = tick_bank(c.prices)
        return np.take_along_axis(t, idx, 1), sc
    return np.take_along_axis(c.prices.astype(np.float64), idx, 1), np.ones(c.E)


def features(w, last_units, last_price, budget, shares, k):
    """[E, H] window (bank units), its last value, budget / shares -> [E, H + 2] fp32 feature rows."""
    x = np.empty((w.shape[0], H + 2))
    if k["feature_mode"] == "raw":
        x[:, :H] = w
        x[:, H] = budget
        x[:, H + 1] = shares
        return x
    inv = r32(1.0 / last_units)
    x[:, :H] = r32(r32(w * inv[:, None]) - 1.0)
    ib0 = float(F(1.0 / k["budget0"]))
    x[:, H] = r32(budget * ib0)
    x[:, H + 1] = r32(r32(shares * last_price) * ib0)
    return x


def trade(a, b, s, vnew, k):
    """csrc/trade_rule.h trade_base + trade: (budget', shares')."""
    bd = np.full_like(b, k["budget0"]) if k["compat"] else b
    sd = np.full_like(s, k["shares0"]) if k["compat"] else s
    buy = (a == 0) & (bd >= vnew)
    sell = (a == 1) & (sd > 0)
    b2 = np.where(buy, r32(bd - vnew), np.where(sell, r32(bd + vnew), bd))
    s2 = np.where(buy, sd + 1, np.where(sell, sd - 1, sd))
    return b2, s2


def reward(b, s, vprev, b2, s2, vnew, mode):
    cur = r32(b + r32(s * vprev))
    new = r32(b2 + r32(s2 * vnew))
    r = r32(new - cur)
    if mode in ("relative", "growth"):
        r = np.where(cur > 0, r32(r / np.where(cur > 0, cur, 1.0)), 0.0)
    if mode == "growth":
        r = r32(r - r32(r32(r * 0.5) * r))
    return r


def uniforms(c: Case, mut=None):
    k = c.knobs
    off = 0 if mut == "no_env_offset" else int(k["env_offset"])
    ids = np.arange(off, off + c.E, dtype=np.uint32)
    u1, u2 = strng.uniforms(k["seed"], 0, ids, k["step"])
    return u1.astype(np.float64), u2.astype(np.float64)


def qt_model(c: Case, bank="fp32"):
    """The target pass: QT [E, 3, 4] = Q_target of the next state after each candidate action; column 3 zero."""
    k, st = c.knobs, c.state
    win, unit = gather(c, bank)
    vnew_u = win[:, H]
    vnew = r32(vnew_u * unit)
    out = np.zeros((c.E, 3, 4))
    for a in range(3):
        b2, s2 = trade(np.full(c.E, a), st["budget"].astype(np.float64), st["shares"].astype(np.float64), vnew, k)
        x2 = features(win[:, 1:H + 1], vnew_u, vnew, b2, s2, k)
        q, _, _ = forward(c.target, x2, k["output_relu"], Rounder())
        out[:, a, :3] = q[:, :3]
    return out


# ----------------------------------------------------------------------------- one engine step
def step_model(c: Case, mut=None, bank="fp32", R=None, forced=None):
    """One engine step of every env in float64 with the kernels' rounding points.  Returns a dict: actions, exploit,
    reward, state (the new one), q, q_next, slot, dz (per layer), ins (per layer), per-env statistics terms."""
    assert mut is None or mut in MUTATIONS, mut
    k, st = c.knobs, c.state
    R = R or Rounder()
    E, T = c.E, c.T
    pos = st["pos"].astype(np.int64)
    bud, sh = st["budget"].astype(np.float64), st["shares"].astype(np.float64)
    vprev = st["value"].astype(np.float64)
    win, unit = gather(c, bank)
    last_u, vnew_u = win[:, H - 1], win[:, H]
    last, vnew = r32(last_u * unit), r32(vnew_u * unit)
    # ---- x
    wx = win[:, :H].copy()
    if mut == "win_first_late":
        wx[:, 0] = win[:, 1]
    if mut == "win_last_late":
        wx[:, H - 1] = win[:, H]
    x = features(wx, last_u, vnew if mut == "shares_next_price" else last, bud, sh, k)
    if mut == "win_last_dropped":
        x[:, H - 1] = 0.0
    out_relu = bool(k["output_relu"])
    q, acts, xp = forward(c.params, x, out_relu, R, "")
    qerr = R.last_qerr
    # ---- epsilon-greedy
    u1, u2 = uniforms(c, mut)
    rpos = np.full(E, float(k["step"])) if k["ramp_global"] else pos.astype(np.float64)
    ramp_v = r32(rpos * float(F(1.0 / k["ramp"])))
    if np.isinf(k["epsilon"]):
        thr = np.full(E, np.inf)
    else:
        thr = ramp_v if mut == "thr_no_min" else np.minimum(float(F(k["epsilon"])), ramp_v)
    exploit = (u2 if mut == "u2_explore" else u1) < thr
    greedy = argmax_last(q) if mut == "tie_last" else argmax_first(q)
    rnd = np.minimum(np.floor(r32(u2 * 3.0)).astype(np.int64), 2)
    a = np.where(exploit, greedy, rnd)
    if forced is not None:
        a = np.asarray(forced, np.int64)
    # ---- env step
    b2, s2 = trade(a, bud, sh, vnew, k)
    rew = reward(bud, sh, vprev, b2, s2, vnew, k["reward_mode"])
    # ---- x'
    tb, ts = (bud, sh) if mut == "xn_tail_old" else (b2, s2)
    x2 = features(win[:, 1:H + 1], vnew_u, vnew, tb, ts, k)
    q2, _, _ = forward(c.params, x2, out_relu, R, "n")
    qerr2 = R.last_qerr[:, :3].max(1)
    qa = q2[:, :3]
    qv = qa
    if c.target is not None:
        qt, _, _ = forward(c.target, x2, out_relu, Rounder())
        qv = qt[:, :3]
    am = argmax_last(qa) if mut == "next_tie_last" else argmax_first(qa)
    rows = np.arange(E)
    if k["compat"] or k["double_dqn"]:
        vnext = qv[rows, am]
    elif mut == "next_first":
        vnext = qv[:, 0]
    else:
        vnext = qv.max(axis=1)
    slot = am if k["compat"] else a
    rs = r32(rew * k["reward_scale"]) if k["reward_scale"] != 1.0 else rew
    g = float(F(k["gamma"]))
    y = r32(g * r32(rs + vnext)) if mut == "gamma_on_reward" else r32(rs + r32(g * vnext))
    qs = q[rows, slot]
    diff = r32(qs - y)
    coef, clip = float(F(k["loss_coef"])), float(k["td_clip"])
    d = np.clip(diff, -clip, clip) if clip > 0 else diff
    dqv = r32(coef * d)
    if mut == "clip_after_coef" and clip > 0:
        dqv = np.clip(r32(coef * diff), -clip, clip)
    if out_relu and mut != "no_out_relu_mask":
        dqv = np.where(qs > 0, dqv, 0.0)
    dq = np.zeros((E, 16))
    dq[rows, slot] = dqv
    # ---- backward (qn.backward's rounding points)
    dqerr = np.zeros((E, 16))   # counted: the errors of Q(x)[slot] and of gamma max Q(x'), and three scalar fp32 ops
    dqerr[rows, slot] = coef * (qerr[rows, slot] + g * qerr2) + 4 * U23 * np.abs(dqv)
    dz = dq if mut == "dq_unrounded" else R(dq, "dQ", dqerr)
    ins = [xp] + acts
    dzs = [None, None, dz]
    for l in (2, 1):
        wl = R(_w(np.asarray(c.params, np.float64), l))
        dh = dz @ wl
        m = (ins[l] >= 0) if mut == "relu_mask_ge" else (ins[l] > 0)
        dz = R(dh * m, f"dZ{l}", (dz.shape[1] + 2) * U23 * (np.abs(dz) @ np.abs(wl)))
        dzs[l - 1] = dz
    # ---- new state
    done = pos + 1 >= T - H
    fin = r32(b2 + r32(s2 * vnew))
    ns = {kk: st[kk].copy() for kk in STATE_KEYS}
    rst = done & (mut != "no_reset")
    ns["budget"] = np.where(rst, k["budget0"], b2).astype(F)
    ns["shares"] = np.where(rst, k["shares0"], s2).astype(np.int32)
    ns["value"] = np.where(rst, 0.0, vnew).astype(F)
    ns["pos"] = np.where(rst, 0, pos + 1).astype(np.int32)
    ns["ret_sum"] = np.where(rst, 0.0, r32(st["ret_sum"].astype(np.float64) + rew)).astype(F)
    ns["episodes"] = (st["episodes"] + done).astype(np.int32)
    ns["last_final"] = np.where(done, fin.astype(F), st["last_final"]).astype(F)
    stored_rew = r32(rew * k["reward_scale"]) if mut == "scale_stored_reward" else rew
    dl = d if mut == "loss_from_clipped" else diff
    fd = np.where(done, fin, 0.0)
    terms = np.stack([rew, r32(dl * dl), (~exploit).astype(np.float64), done.astype(np.float64), fd, r32(fd * fd),
                      qs, np.zeros(E)], axis=1)
    return dict(actions=a.astype(np.int32), exploit=exploit, greedy=greedy, reward=stored_rew, state=ns, q=q,
                q_next=q2, slot=slot, target=y, diff=diff, dzs=dzs, ins=ins, terms=terms, x=x, x_next=x2,
                counts=R.counts, thr=thr, u1=u1)


# ----------------------------------------------------------------------------- schedule, slabs, reduce
def owner(E, chunk, grid):
    """Static chunk schedule of all three kernels: workgroup b steps chunks b + k * grid.  -> [E] workgroup of env."""
    return (np.arange(E) // chunk) % grid


def grad_of(res, envs, mut=None, tile_drop=None):
    """The flat gradient summed over ``envs`` (an index array) in float64."""
    g = np.zeros(LAYOUT.numel)
    for l in range(3):
        dz, a = res["dzs"][l][envs], res["ins"][l][envs]
        gw = dz.T @ a
        if l == 0 and mut == "no_bias_col":
            gw[:, LAYOUT.bias_col] = 0.0
        _w(g, l)[...] = gw
        if l > 0:
            keep = envs if tile_drop is None else envs[~np.isin(envs, tile_drop)]
            _b(g, l)[...] = res["dzs"][l][keep].sum(0)
    return g


def partials(c: Case, res, chunk, grid, mut=None):
    """[grid, P] float64: the exact per-workgroup gradient partials of the static schedule."""
    own = owner(c.E, chunk, grid)
    drop = np.arange(16, 32) if mut == "db_tile_dropped" else None   # the second 16-env tile of chunk 0
    return np.stack([grad_of(res, np.nonzero(own == b)[0], mut, drop) for b in range(grid)])


def slab_model(part, bf16, mut=None):
    """What the kernel leaves in its slab: fp32 [grid, P] (the exact sums), or bf16 bit patterns [P/32, grid, 32]
    (one round-to-nearest-even per element, column-blocked)."""
    G, P = part.shape
    if mut == "slab_row_next":
        part = np.roll(part, 1, axis=0)
    if not bf16:
        return part
    bits = (bf16_trunc(r32(part)) if mut == "slab_trunc" else bf16_rne(part))
    out = np.zeros((P // 32, G, 32), np.uint16)
    idx = np.arange(P)
    blk = (idx >> 4) if mut == "slab_block_shift4" else (idx >> 5)
    ok = blk < P // 32
    for b in range(G):
        out[blk[ok], b, idx[ok] & 31] = bits[b, ok]
    return out


def slab_values(slab, bf16):
    """Slab -> [grid, P] float64 values."""
    if not bf16:
        return np.asarray(slab, np.float64)
    nb, G, _ = slab.shape
    return bf16_val(slab).transpose(1, 0, 2).reshape(G, nb * 32)


def reduce_model(slab, bf16):
    """csrc/optim.hip slab pass: the fp32 sum of the slab rows (exact on exact cases)."""
    return slab_values(slab, bf16).sum(0)


def stats_model(c: Case, res, chunk, grid):
    """[grid, NSTAT] float64: per-workgroup statistics rows."""
    own = owner(c.E, chunk, grid)
    return np.stack([res["terms"][own == b].sum(0) for b in range(grid)])


# ----------------------------------------------------------------------------- exactness precondition
def _lowlog(x):
    """log2 of the lowest set bit of every entry (inf where the entry is 0)."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(x != 0, np.log2(np.where(low > 0, low, 1.0)) + e - 53, np.inf)


def dot_bits(A, B, extra=None):
    """max over the outputs of A [M, K] @ B [K, N] (+ extra [N]) of log2(sum |terms| / grid), grid the largest power
    of two dividing every term of that output.  Below 24: the fp32 sum is exact in any order."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    mag = np.abs(A) @ np.abs(B)
    la, lb = _lowlog(A), _lowlog(B)
    g = np.full(mag.shape, np.inf)
    for kk in range(A.shape[1]):
        if np.isfinite(la[:, kk]).any() and np.isfinite(lb[kk]).any():
            g = np.minimum(g, la[:, kk, None] + lb[None, kk, :])
    if extra is not None:
        mag = mag + np.abs(extra)[None, :]
        g = np.minimum(g, _lowlog(extra)[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        bits = np.where(mag > 0, np.log2(mag) - g, 0.0)
    return float(bits.max()) if bits.size else 0.0


def sum_bits(terms):
    """The same for plain column sums of terms [n, m]."""
    t = np.asarray(terms, np.float64)
    return dot_bits(np.ones((1, t.shape[0])), t)


def exact_bits(c: Case, res, chunk=None, grid=None, bf16=False):
    """name -> bits used by the widest sum of that kind (forward and backward dot products, weight-gradient and bias
    sums over ALL envs -- an upper bound for every partial and for the fp32-slab reduce -- the statistics; with
    ``chunk`` / ``grid`` also the reduce over bf16-rounded partials)."""
    P = np.asarray(c.params, np.float64)
    out = {}
    ins, dzs = res["ins"], res["dzs"]
    for tag, xin in (("x", res["x"]), ("xn", res["x_next"])):
        a = bf16_round64(pad_input(xin))
        for l in range(3):
            out[f"fwd{l}({tag})"] = dot_bits(a, bf16_round64(_w(P, l)).T, _b(P, l) if l > 0 else None)
            z = a @ bf16_round64(_w(P, l)).T + (_b(P, l) if l > 0 else 0.0)
            a = bf16_round64(np.maximum(z, 0.0))
    if c.target is not None:
        Tg = np.asarray(c.target, np.float64)
        a = bf16_round64(pad_input(res["x_next"]))
        for l in range(3):
            out[f"fwd{l}(target)"] = dot_bits(a, bf16_round64(_w(Tg, l)).T, _b(Tg, l) if l > 0 else None)
            a = bf16_round64(np.maximum(a @ bf16_round64(_w(Tg, l)).T + (_b(Tg, l) if l > 0 else 0.0), 0.0))
    for l in (2, 1):
        out[f"dH{l}"] = dot_bits(dzs[l], bf16_round64(_w(P, l)))
    for l in range(3):
        out[f"dW{l}"] = dot_bits(dzs[l].T, ins[l])
        if l > 0:
            out[f"db{l}"] = sum_bits(dzs[l])
    out["stats"] = sum_bits(res["terms"])
    if bf16 and grid:
        part = bf16_round64(partials(c, res, chunk, grid))
        out["reduce(bf16)"] = sum_bits(part)
    return out


def assert_exact(c: Case, res, **kw):
    bits = exact_bits(c, res, **kw)
    bad = {k: round(v, 2) for k, v in bits.items() if v >= LIMIT_BITS}
    if bad:
        raise AssertionError(f"case {c.name}: not exact in fp32, bits per sum {bad}")
    return bits


# ----------------------------------------------------------------------------- exact-case builders
def _sparse(g, shape, values, density):
    v = g.choice(np.asarray(values, np.float64), size=shape)
    return v * (g.random(shape) < density)


def exact_params(seed, w0_vals=(-1.0, 1.0), w0_density=1 / 16, w1_vals=(-1.0, 1.0), w1_density=1 / 16,
                 w2_vals=(-1.0, 1.0), w2_density=1 / 16, bias_step=0.5, bias_span=4, tie=None, special=False,
                 raw=False):
    """Dyadic weights, all three layers sparse, biases multiples of ``bias_step``.  ``tie``: rows of W2 / b2 made
    equal -- (0, 1) or (1, 2) (the third row pushed below them by its bias) or (0, 1, 2).  ``special``: three
    hidden units whose values need more than 8 bits, so H1, H2 and dZ2 round (H1 and H2 also on exact ties):
    unit 5 of layer 1 and unit 9 of layer 2 sit at 128 + k / 2 (their outgoing weights are zero: they show in
    dW1's column 5 and dW2's column 9), and unit 17 of layer 2 leaves through weights of 1.5."""
    g = np.random.default_rng(seed)
    P = np.zeros(LAYOUT.numel)
    _w(P, 0)[:128, :H + 2] = _sparse(g, (128, H + 2), w0_vals, w0_density)
    if raw:   # raw features: prices and budgets are multiples of 2048, their weights +-2^-12
        _w(P, 0)[:128, :H + 1] *= 2.0 ** -12
    _w(P, 0)[:128, LAYOUT.bias_col] = g.integers(-bias_span, bias_span + 1, 128) * bias_step
    _w(P, 1)[...] = _sparse(g, (128, 128), w1_vals, w1_density)
    _b(P, 1)[...] = g.integers(-bias_span, bias_span + 1, 128) * bias_step
    _w(P, 2)[:3] = _sparse(g, (3, 128), w2_vals, w2_density)
    _b(P, 2)[:3] = g.integers(-bias_span, bias_span + 1, 3) * bias_step
    if tie:
        _b(P, 2)[tie[0]] += 8.0   # (most envs then keep the tied pair above 0, where an output ReLU lets it through)
        for r in tie[1:]:
            _w(P, 2)[r] = _w(P, 2)[tie[0]]
            _b(P, 2)[r] = _b(P, 2)[tie[0]]
        if len(tie) == 2:   # the third Q below the tied pair on every env
            _b(P, 2)[3 - sum(tie)] = _b(P, 2)[tie[0]] - 4096.0
    if special:
        _w(P, 0)[5, LAYOUT.bias_col] = 128.0
        _w(P, 1)[:, 5] = 0.0
        _b(P, 1)[9] = 128.0
        _w(P, 2)[:, 9] = 0.0
        _b(P, 1)[17] = 2.0
        _w(P, 2)[:3, 17] = (1.5, -1.5, 1.5)
    return P.astype(F)


def exact_bank(E, T, pos, seed):
    """Prices of 16 * ticks, ticks in {128, 256, 384, 512}; the prices that end the windows of x and x' (positions
    pos + H - 1 and pos + H) are 128 or 256 ticks, so 1 / last and w / last - 1 are exact with or without FMA and
    every relative feature is a multiple of 1/2 (coarse on purpose: loss_sum adds squares of TD errors and needs
    twice their bits, see profiles/step_refs.md)."""
    g = np.random.default_rng(seed)
    t = g.integers(1, 5, (E, T)) * 128.0
    e = np.arange(E)
    t[e, pos + H - 1] = g.choice((128.0, 256.0), E)
    t[e, pos + H] = g.choice((128.0, 256.0), E)
    return (16.0 * t).astype(F)


def make_case(name, E, seed=0, T=260, kind="base", knobs=None, tie=None, target=False, check=True, pvals=None,
              value_step=0.5):
    """Build one exact case and check its precondition.

    kind "base": positions spread over [1, 48) (every start parity and every pos % 8), budgets multiples of 2048,
    shares 0..2, value = v_new + {-1, -.5, 0, .5, 1}.  "edges": additionally envs at pos = 0 (threshold 0: never
    exploit), envs on the last position (episode end and reset), budget == v_new (buy allowed), shares == 0 (sell
    refused), and, with a relative reward, envs whose portfolio value is 0 (the cur <= 0 branch)."""
    g = np.random.default_rng(1000 + seed)
    k = default_knobs(**(knobs or {}))
    e = np.arange(E)
    pos = 1 + (e * 5 + e // 16) % 47
    last_pos = T - H - 1
    if kind == "edges":
        pos = np.where(e % 8 == 3, 0, pos)
        pos = np.where(e % 8 == 6, last_pos, pos)
    prices = exact_bank(E, T, pos, 2000 + seed)
    vnew = prices[e, pos + H].astype(np.float64)
    budget = g.integers(1, 5, E) * 2048.0
    shares = g.integers(0, 3, E)
    value = vnew + g.integers(-2, 3, E) * value_step
    if kind == "edges":
        budget = np.where(e % 4 == 1, vnew, budget)
        shares = np.where(e % 4 == 2, 0, shares)
        if k["reward_mode"] != "absolute":
            # portfolio value a power of two (the division is then exact, so the reward sums are), or 0
            shares = np.zeros(E, np.int64)
            budget = np.where(e % 4 == 1, vnew, np.where(e % 8 == 4, 0.0, budget))
            budget = np.where(budget == 6144.0, 4096.0, budget)
    if k["compat"]:
        # the reference's child actor trades from its constructor budget / shares on every step: the state stays
        # beside them (budget within 2 of budget0, so a decision taken from the state's budget would show)
        budget = k["budget0"] + g.integers(-4, 5, E) * 0.5
        shares = np.full(E, k["shares0"], np.int64)
    st = dict(budget=budget.astype(F), shares=shares.astype(np.int32), value=value.astype(F),
              pos=pos.astype(np.int32), episodes=(e % 3).astype(np.int32),
              last_final=np.full(E, np.nan, F), ret_sum=(g.integers(-4, 5, E) * 0.5).astype(F))
    params = exact_params(3000 + seed, tie=tie, **(pvals or {}))
    tgt = None
    if target:
        # the target net: a dyadic perturbation of the online one (its W2 rows are distinct even on tie cases)
        tp = exact_params(3000 + seed, **(pvals or {})).astype(np.float64)
        gg = np.random.default_rng(4000 + seed)
        _w(tp, 2)[:3] += gg.integers(-1, 2, (3, 128)) * (gg.random((3, 128)) < 0.125)
        _b(tp, 2)[:3] += np.array([1.0, -2.0, 3.0])
        _b(tp, 1)[...] += gg.integers(-1, 2, 128) * 0.5
        tgt = tp.astype(F)
    c = Case(name, prices, st, params, k, tgt)
    if check:
        res = step_model(c)
        c.notes["bits"] = assert_exact(c, res)
        c.notes["counts"] = dict(res["counts"])
        _coverage(c, res, kind, tie)
    return c


def _coverage(c: Case, res, kind, tie):
    """What the case must contain; a builder that lost one of these raises."""
    st, k = c.state, c.knobs
    pos = st["pos"]
    a = res["actions"]
    X = res["ins"][0][:, :H]
    assert len({X[:, j].tobytes() for j in range(H)}) == H, "two window columns are equal over the batch"
    if c.E >= 32:   # every window start parity and every pos % 8 (the 16-bit bank's 16-byte phase)
        assert set(pos % 8) == set(range(8)), set(pos % 8)
    q3 = np.sort(res["q"][:, :3], axis=1)
    ties = int(((q3[:, 2] == q3[:, 1])).sum())
    c.notes["q_ties"] = ties
    if tie:
        # the pinned action, from the rule and not from the model's argmax: the first index of the tied pair (the
        # third Q lies 4096 below); with the output ReLU a pair at or below 0 ties with the third at 0 -> index 0
        assert ties == c.E, (ties, c.E)
        first = np.full(c.E, tie[0])
        if k["output_relu"]:
            first = np.where(res["q"][:, tie[0]] > 0, first, 0)
        c.pinned = first
        exploit = res["exploit"]
        assert exploit.sum() > 0 and np.all(a[exploit] == c.pinned[exploit])
        assert len(set(c.pinned)) == (2 if (k["output_relu"] and tie[0]) else 1), set(c.pinned)
        # Q(x') ties the same way: its argmax is the compat slot / the double-DQN action
        qn3 = res["q_next"][:, :3]
        assert np.all(qn3.max(1) == qn3[:, tie[1]])
    if kind == "edges":
        vnew = c.prices[np.arange(c.E), pos + H]
        cover = dict(pos0=int((pos == 0).sum()), reset=int((res["state"]["episodes"] > st["episodes"]).sum()),
                     buy_at_budget=int(((a == 0) & (st["budget"] == vnew)).sum()),
                     sell_without_shares=int(((a == 1) & (st["shares"] == 0)).sum()))
        if k["reward_mode"] != "absolute":
            cover["cur_not_positive"] = int((st["budget"] + st["shares"] * st["value"] <= 0).sum())
        assert all(v > 0 for v in cover.values()), cover
        assert not res["exploit"][pos == 0].any()
        c.notes["cover"] = cover


# the weights of the rounding case (exact_params ``special``): H1, H2, dQ, dZ2 and dZ1 all round, H1 and H2 on ties
ROUNDING_PVALS = dict(special=True)


def rounding_case(E, seed=0, **kw):
    """The scaled variant: every rounding point of the chain rounds on a counted number of entries."""
    c = make_case(f"rounding-E{E}", E, seed, pvals=ROUNDING_PVALS, value_step=1 / 16, **kw)
    n = c.notes["counts"]
    for tag in ("H1", "H2", "dQ", "dZ2", "dZ1"):
        assert n.get(tag, [0, 0])[0] > 0, (tag, n)
    assert sum(v[1] for v in n.values()) > 0, ("no exact bf16 tie", n)
    return c


TIES = {"t01": (0, 1), "t12": (1, 2), "t012": (0, 1, 2)}


def tie_case(E, which, seed=0, **kw):
    """W2 / b2 rows made equal: the greedy action ties on every env (and so do Q(x') and its argmax); with
    epsilon = 1 and ramp = 1 every env beyond position 0 exploits, so the first tied index is pinned."""
    kn = dict(epsilon=1.0, ramp=1.0)
    kn.update(kw.pop("knobs", None) or {})
    return make_case(f"tie-{which}-E{E}", E, seed, tie=TIES[which], knobs=kn, **kw)


# ----------------------------------------------------------------------------- comparisons
def _bits32(v):
    b = np.ascontiguousarray(v, dtype=F).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return b


def check_f32(got, ref, mask=None):
    """(differing fp32 bit patterns, index of the first) against the float64 reference, which must be an fp32 value;
    -0 counts as +0, NaN equals the same NaN."""
    r64 = np.asarray(ref, np.float64)
    b = r64.astype(F)
    ok = np.isnan(r64) | (b.astype(np.float64) == r64)
    assert ok.all(), "reference not exact in fp32"
    d = _bits32(got) != _bits32(b)
    if mask is not None:
        d &= mask
    w = np.argwhere(d)
    return int(d.sum()), (tuple(int(i) for i in w[0]) if len(w) else None)


def check_int(got, ref):
    d = np.asarray(got).astype(np.int64) != np.asarray(ref).astype(np.int64)
    w = np.argwhere(d)
    return int(d.sum()), (tuple(int(i) for i in w[0]) if len(w) else None)


def check_bf16(got_bits, ref_bits, mask=None):
    a = np.asarray(got_bits, np.uint16).copy()
    b = np.asarray(ref_bits, np.uint16).copy()
    assert a.shape == b.shape, (a.shape, b.shape)
    a[a == 0x8000] = 0
    b[b == 0x8000] = 0
    d = a != b
    if mask is not None:
        d &= mask
    w = np.argwhere(d)
    return int(d.sum()), (tuple(int(i) for i in w[0]) if len(w) else None)


def slab_mask(m, grid, bf16):
    """A flat mask in the slab's layout."""
    if not bf16:
        return np.broadcast_to(m[None, :], (grid, m.size))
    return np.broadcast_to(m.reshape(-1, 1, 32), (m.size // 32, grid, 32))


def check_step(got, c: Case, res, chunk, grid, bf16, mut=None, mask=None):
    """Compare everything one launch leaves behind with the model.  ``got``: actions, reward, state (dict), slab (in
    its layout: fp32 [grid, P] or bf16 bits [P/32, grid, 32]), grad [P], stats [grid, NSTAT]; missing keys are not
    compared.  ``mut`` mutates the model's schedule / slab side (the step-side mutations are in ``res``); ``mask``:
    the flat entries of the slab to compare (default: all; the GPU file passes ``real_mask()``).  The reduced gradient
    is compared on every entry.  Returns name -> (differing entries, first location)."""
    out = {}
    mask = np.ones(LAYOUT.numel, bool) if mask is None else mask
    if "actions" in got:
        out["actions"] = check_int(got["actions"], res["actions"])
    if "reward" in got:
        out["reward"] = check_f32(got["reward"], res["reward"])
    for kk, v in got.get("state", {}).items():
        ref = res["state"][kk]
        out["state." + kk] = check_int(v, ref) if ref.dtype == np.int32 else check_f32(v, ref.astype(np.float64))
    part = partials(c, res, chunk, grid, mut)
    slab = slab_model(part, bf16, mut)
    if "slab" in got:
        out["slab"] = (check_bf16 if bf16 else check_f32)(got["slab"], slab, slab_mask(mask, grid, bf16))
    if "grad" in got:
        out["grad"] = check_f32(got["grad"], reduce_model(slab, bf16))
    if "stats" in got:
        out["stats"] = check_f32(got["stats"], stats_model(c, res, chunk, grid))
    return out


def model_outputs(c: Case, res, chunk, grid, bf16, mut=None):
    """What a kernel that computes ``res`` (and the slab-side mutation) would leave behind, in check_step's form."""
    slab = slab_model(partials(c, res, chunk, grid, mut), bf16, mut)
    return dict(actions=res["actions"], reward=res["reward"].astype(F), state=res["state"], slab=slab,
                grad=reduce_model(slab, bf16).astype(F), stats=stats_model(c, res, chunk, grid).astype(F))


def total(diffs) -> int:
    return sum(v[0] for v in diffs.values())


# ----------------------------------------------------------------------------- the committed exact cases
_CACHE = {}


def exact_case(kind, E, compat=False):
    """The exact cases by name (built once per process, never modified by a test):

    base      the plain recipe                                  edges     pos 0, episode end, budget == v_new, ...
    rounding  H1 / H2 / dQ / dZ2 / dZ1 round (E <= 192)         t01, t12, t012   W2 / b2 rows equal
    raw       raw features (prices, budget, shares as they are) on "edges"; the window's weights are +-2^-12
    rel, growth   the relative / growth reward on "edges" (with the cur <= 0 branch)
    clip      td_clip = 4 on "edges"
    knobs05, knobs2   target net + double DQN + reward_scale 0.5 / 2 + the global ramp (ws knob build)
    knobs-t01 the same with tied W2 rows of the online net and distinct rows of the target net
    "edges" and its variants run with env_offset = 3 E, so the Philox counter's env id is not the local index."""
    key = (kind, E, compat)
    if key in _CACHE:
        return _CACHE[key]
    off = dict(env_offset=3 * E)
    name = f"{kind}-E{E}" + ("-compat" if compat else "")
    if kind == "base":
        c = make_case(name, E, 1, knobs=dict(compat=compat))
    elif kind == "raw":
        c = make_case(name, E, 9, kind="edges", knobs=dict(compat=compat, feature_mode="raw", **off),
                      pvals=dict(raw=True))
    elif kind == "edges":
        c = make_case(name, E, 2, kind="edges", knobs=dict(compat=compat, **off))
    elif kind == "rounding":
        c = rounding_case(E, 3, knobs=dict(compat=compat))
        c.name = name
    elif kind in TIES:
        c = tie_case(E, kind, 4, knobs=dict(compat=compat))
        c.name = name
    elif kind in ("rel", "growth"):
        c = make_case(name, E, 5, kind="edges", knobs=dict(compat=compat, **off,
                                                           reward_mode={"rel": "relative"}.get(kind, kind)))
    elif kind == "clip":
        c = make_case(name, E, 6, kind="edges", knobs=dict(compat=compat, td_clip=4.0, **off))
    elif kind in ("knobs05", "knobs2"):
        c = make_case(name, E, 7, target=True, knobs=dict(double_dqn=True, ramp_global=True, step=40,
                                                          reward_scale=0.5 if kind == "knobs05" else 2.0))
    elif kind == "knobs-t01":
        c = tie_case(E, "t01", 8, target=True, knobs=dict(double_dqn=True, reward_scale=2.0))
        c.name = name
    else:
        raise KeyError(kind)
    _CACHE[key] = c
    return c


# ----------------------------------------------------------------------------- the bounded random case
def random_case(E, seed, T=400):
    """Realistic magnitudes: a random-walk bank on the tick grid (as the step tests' ``_prices``), the default
    He-normal init (host mirror), the flagship's relative reward, gamma 0.9, loss_coef 2 / E.  Not exact: compared
    per slice within a bound taken from the reference (``random_bounds``)."""
    from sharetrade.config import preset_config
    from sharetrade.data.prices import random_walk, tick16_quantize

    prices = tick16_quantize(random_walk(T, 50.0, 0.02, seed, n_series=E).astype(F))
    params = qn.init_params(LAYOUT, preset_config("flagship").model, seed=1234, host_mirror=True).numpy()
    params = params * LAYOUT.trainable_mask(True).numpy()
    e = np.arange(E)
    pos = (e * 3 % 190).astype(np.int32)
    shares = (e % 3).astype(np.int32)
    st = dict(budget=np.full(E, 2400.0, F), shares=shares, value=prices[e, pos + H - 1].astype(F), pos=pos,
              episodes=np.zeros(E, np.int32), last_final=np.full(E, np.nan, F), ret_sum=np.zeros(E, F))
    k = default_knobs(budget0=2400.0, gamma=0.9, epsilon=0.5, ramp=64.0, loss_coef=2.0 / E, reward_mode="relative")
    return Case(f"random-E{E}-s{seed}", prices, st, params.astype(F), k)


_SLICES = None


def slices():
    """(layer name, slice name, flat indices): each row and each column of every weight gradient (parameters only)
    and each group of 16 bias elements."""
    global _SLICES
    if _SLICES is None:
        out = []
        idx = np.arange(LAYOUT.numel)
        d = LAYOUT.dims
        for l in range(3):
            w = _w(idx, l)
            nin = d[l] + (1 if l == 0 else 0)   # layer 0: the bias column is a column of W0
            for r in range(d[l + 1]):
                out.append((f"W{l}", f"row{r}", w[r, :nin].copy()))
            for cc in range(nin):
                out.append((f"W{l}", f"col{cc}", w[:d[l + 1], cc].copy()))
            if l > 0:
                b = _b(idx, l)[:d[l + 1]]
                for g0 in range(0, d[l + 1], 16):
                    out.append((f"b{l}", f"grp{g0 // 16}", b[g0:g0 + 16].copy()))
        _SLICES = out
    return _SLICES


def slice_norms(v):
    return np.array([np.sqrt((v[i] ** 2).sum()) for _, _, i in slices()])


def accumulation_term(res, n_terms):
    """Per element (K + 2) 2^-23 sum |terms| of the weight-gradient and bias sums over all envs (K = the number of
    terms: the rounding of the MFMA's internal adds is not specified, hence 2^-23 and not 2^-24)."""
    g = np.zeros(LAYOUT.numel)
    for l in range(3):
        dz, a = np.abs(res["dzs"][l]), np.abs(res["ins"][l])
        _w(g, l)[...] = dz.T @ a
        if l > 0:
            _b(g, l)[...] = dz.sum(0)
    return (n_terms + 2) * U23 * g


def random_bounds(c: Case, seeds=8, actions=None):
    """Everything the bounded comparison needs, from the reference alone:

    ref    the float64 step (bf16 rounding points, no fp32 rounding of sums) with ``actions`` forced if given
    floor  per slice, the largest L2 deviation of the gradient over ``seeds`` flip runs (every bf16 rounding of a
           feature, an activation, dQ and dZ nudged by +- the counted fp32 error of the value that rounds, so
           every value that could round the other way in a kernel does so in about half of the runs)
    acc    per element, the counted fp32 accumulation term
    qdev   per env, 4 x the largest deviation of any Q value over the flip runs + the counted term of the last
           layer: an env whose two largest Q lie closer than 2 qdev may legitimately pick either action."""
    ref = step_model(c, forced=actions)
    whole = np.arange(c.E)
    g0 = grad_of(ref, whole)
    floor = np.zeros(len(slices()))
    qfloor = np.zeros(c.E)
    for s in range(seeds):
        r = step_model(c, R=Rounder(flip=np.random.default_rng(77 + s)), forced=ref["actions"])
        floor = np.maximum(floor, slice_norms(grad_of(r, whole) - g0))
        qfloor = np.maximum(qfloor, np.abs(r["q"][:, :3] - ref["q"][:, :3]).max(1))
    P = np.asarray(c.params, np.float64)
    qacc = (128 + 2) * U23 * (np.abs(ref["ins"][2]) @ np.abs(bf16_round64(_w(P, 2))).T
                                     + np.abs(_b(P, 2)))[:, :3].max(1)
    return dict(ref=ref, grad=g0, floor=floor, acc=accumulation_term(ref, c.E), qdev=4.0 * qfloor + qacc)


def uncertain_envs(rb):
    """Exploiting envs whose two largest float64 Q values lie within 2 qdev of each other."""
    q = np.sort(rb["ref"]["q"][:, :3], axis=1)
    return rb["ref"]["exploit"] & (q[:, 2] - q[:, 1] < 2.0 * rb["qdev"])


def slice_bounds(c: Case, rb, chunk=None, grid=None, bf16=False):
    """Per slice: 4 x the flip-noise floor + the L2 norm of the counted accumulation term; bf16 slabs add one
    round-to-nearest per partial (2^-9 of each workgroup's partial, counted from the format)."""
    acc = rb["acc"]
    if bf16:
        acc = acc + 2.0 ** -9 * np.abs(partials(c, rb["ref"], chunk, grid)).sum(0)
    return 4.0 * rb["floor"] + slice_norms(acc)


def check_random(grad, rb, bound):
    """(slices with err / bound > 1, layer -> largest err / bound) of a reduced gradient against the reference."""
    err = slice_norms(np.asarray(grad, np.float64) - rb["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = {}
    for (layer, _, _), r in zip(slices(), ratio):
        worst[layer] = max(worst.get(layer, 0.0), float(r))
    return int((ratio > 1.0).sum()), worst
