"""Host references, input builders, case lists and layout maps for the kernels of csrc/gru_learn.hip.

tests/test_gpu_gru_learn_kernels.py compares the kernels with these on the GPU; tests/test_gru_learn_refs.py
mutates them on the CPU and shows that the same comparisons (the ``check_*`` functions below, which both
files call) would notice.  Everything is float64 with an error bound counted from the kernel's operations
(u = 2^-24); bf16 outputs are compared with the interval check of tests/deep_kernel_refs.py.  The only
measured bound is the forward chain's flip noise (``fwd_chain_bound``): it is measured on the reference,
never on the kernel.

Gate pre-activations are kept in the kernels' pre-scaled form (csrc/gru_common.h): the r / z rows of W_hh,
W_ih and the biases carry -log2(e), the n rows -2 log2(e); sigmoid(a) = 1 / (1 + 2^a')."""
import numpy as np
import torch

from deep_kernel_refs import U, F, bf16_bits, bf16_round64, bf16_val, interval_ok, ratio   # noqa: F401
from sharetrade.ops.gru import GS_N, GS_RZ, mx_roundtrip
from sharetrade.utils.rng import philox4x32

RH, RG, RF, RFL, RW, NSV, LB, LBB = 256, 768, 32, 64, 8, 5, 32, 16
SV_R, SV_Z, SV_N, SV_GH, SV_HP = range(5)
SV_NAMES = ("r", "z", "n", "gh_n", "h_prev")
KEY0, KEY1 = 0x9E3779B9, 0x0BADC0DE
TAG_SEQ = 0x53455131
GS = np.concatenate([np.full(2 * RH, GS_RZ), np.full(RH, GS_N)])     # fp32 values, as float64
LN2 = float(np.log(2.0))


def start_below(s):
    """A power of two at or below s (1 where s is 0): the start value of an accumulated output."""
    s = np.asarray(s, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(s > 0, np.exp2(np.floor(np.log2(np.where(s > 0, s, 1.0)))), 1.0)


def bf(x) -> np.ndarray:
    """fp32-representable values -> their bf16 roundings (float64)."""
    return bf16_val(bf16_bits(np.asarray(x, F))).reshape(np.shape(x))


def mxrt(x) -> np.ndarray:
    """MX-fp8 round trip of float64 [..., K] in 32-blocks along the last axis (the kernels' quant_h rule)."""
    return mx_roundtrip(torch.from_numpy(np.ascontiguousarray(x, dtype=F))).double().numpy()


def interval_ratio(bits, val, delta, mask=True) -> float:
    """The figure printed beside an interval check: how much of delta the stored values needed.  0 where the
    stored bf16 is rne_bf16(ref) itself; else the distance from ref to the rounding boundary between
    rne_bf16(ref) and the stored value, over delta (above 1: outside the interval)."""
    v = bf16_val(bits).reshape(np.shape(val))
    r = bf16_round64(val)
    need = np.where(mask & (v != r), np.abs((v + r) / 2 - val), 0.0)
    return ratio(need, np.broadcast_to(delta, need.shape))


# ----------------------------------------------------------------------------- layout maps
_ORDER = ("m", "n", "g4", "i")


def _split(b, u):
    b, u = np.asarray(b, np.int64), np.asarray(u, np.int64)
    return {"blk": b // LB, "n": (b % LB) // 16, "l16": b % 16, "wave": u // 32, "m": (u % 32) // 16,
            "g4": (u % 16) // 4, "i": u % 4}


def sv_index(t, b, u, q, B, swap=None):
    """Index (in bf16 elements) into the forward saves of (step t, sequence b, unit u, quantity q):
    [S][B/32][wave][quantity][tile n][lane = 16 g4 + l16][k = 4 m + i].  swap=(x, y) exchanges two of
    (m, n, g4, i): the mutated maps of the CPU test."""
    d = _split(b, u)
    if swap:
        d[swap[0]], d[swap[1]] = d[swap[1]], d[swap[0]]
    nblk = B // LB
    lane, k = 16 * d["g4"] + d["l16"], 4 * d["m"] + d["i"]
    return (((((np.asarray(t, np.int64) * nblk + d["blk"]) * RW + d["wave"]) * NSV + q) * 2 + d["n"]) * 64 + lane) * 8 + k


def sv_coords(idx, B):
    """The inverse of sv_index: (t, b, u, q)."""
    idx = np.asarray(idx, np.int64)
    k, idx = idx % 8, idx // 8
    lane, idx = idx % 64, idx // 64
    n, idx = idx % 2, idx // 2
    q, idx = idx % NSV, idx // NSV
    wave, idx = idx % RW, idx // RW
    blk, t = idx % (B // LB), idx // (B // LB)
    return t, blk * LB + 16 * n + lane % 16, 32 * wave + 16 * (k // 4) + 4 * (lane // 16) + k % 4, q


def sv_size(S, B) -> int:
    return S * (B // LB) * RW * NSV * 2 * 64 * 8


def ht_col(blk, b, B):
    """Column of HT that holds sequence b of block blk (block 0 = h0, block t + 1 = the masked h_t)."""
    return np.asarray(blk, np.int64) * B + b


def row_tb(t, b, B):
    """Row of X / Q / dQ, and column of dGxT / dGhT, of (step t, sequence b): time-major."""
    return np.asarray(t, np.int64) * B + b


def bwd_block(bid, swapped=False):
    """Backward workgroup bid (16 sequences) -> (forward block, tile n) of the saves it reads."""
    return (bid & 1, bid >> 1) if swapped else (bid >> 1, bid & 1)


def sv_pack(q5, S, B, swap=None) -> np.ndarray:
    """Five quantities [5][S][B][RH] (float64, any values) -> the saves as bf16 bit patterns, flat."""
    out = np.zeros(sv_size(S, B), np.uint16)
    t, b, u = np.meshgrid(np.arange(S), np.arange(B), np.arange(RH), indexing="ij")
    for q in range(NSV):
        out[sv_index(t, b, u, q, B, swap)] = bf16_bits(np.asarray(q5[q], np.float64).astype(F)).reshape(S, B, RH)
    return out


def sv_unpack(raw, S, B) -> np.ndarray:
    """The saves' bit patterns -> [5][S][B][RH] uint16."""
    t, b, u = np.meshgrid(np.arange(S), np.arange(B), np.arange(RH), indexing="ij")
    return np.stack([np.asarray(raw, np.uint16)[sv_index(t, b, u, q, B)] for q in range(NSV)])


# ----------------------------------------------------------------------------- gather
GATHER_S = [1, 23, 24, 47, 48, 64]
GATHER_B = [1, 5, 32]
GATHER_CAP = 4099       # 2^16 + 1 slots would take 45 MB at S = 1 and 290 MB at S = 64
GATHER_FILL = [0, 1, 5, GATHER_CAP]
GATHER_STEPS = [0, 3, 2 ** 32 + 1]


def gather_ring(S: int, cap: int, seed: int) -> dict:
    """Random bit patterns in rx / rh0, random ra / rr / rd (rd over the whole byte: D = float(rd))."""
    g = np.random.default_rng(seed)
    return {"rx": g.integers(0, 1 << 16, (cap, S + 1, RF), dtype=np.uint16),
            "rh0": g.integers(0, 1 << 16, (cap, RH), dtype=np.uint16),
            "ra": g.integers(0, 256, (cap, S), dtype=np.uint8), "rr": g.standard_normal((cap, S)).astype(F),
            "rd": g.integers(0, 256, (cap, S), dtype=np.uint8)}


def seq_index(B: int, step: int, size: int, key0=KEY0, key1=KEY1, low_word=False) -> np.ndarray:
    """The sequence gather's draw per row: counter (row, step_lo, step_hi, 'SEQ1'), ((c0 << 32) | c1) % size."""
    rows = np.arange(B, dtype=np.uint32)
    r0, r1, _, _ = philox4x32(rows, np.full(B, step & 0xFFFFFFFF, np.uint32), np.full(B, (step >> 32) & 0xFFFFFFFF, np.uint32),
                              np.full(B, TAG_SEQ, np.uint32), np.full(B, key0, np.uint32), np.full(B, key1, np.uint32))
    n = max(int(size), 1)
    return np.array([(int(b) if low_word else ((int(a) << 32) | int(b))) % n for a, b in zip(r0, r1)], dtype=np.int64)


def gather_ref(ring, S, B, step, size, key0=KEY0, key1=KEY1, low_word=False, one_pass=False, ones_col=True,
               short_ard=False) -> dict:
    """What the gather must write: X bits [(S+1)B][RFL], H0 bits (uint32) [B][RH], A [S][B], R, D (fp32).
    Mutations: low_word, one_pass (rows of pieces >= 192 stay zero: S >= 24), ones_col=False,
    short_ard (A / R / D at lane < S - 1 only; the rest keep the sentinel, here NaN / -1)."""
    idx = seq_index(B, step, size, key0, key1, low_word)
    X = np.zeros((S + 1, B, RFL), np.uint16)
    X[:, :, :RF] = ring["rx"][idx].transpose(1, 0, 2)
    if ones_col:
        X[:, :, RF] = 0x3F80
    if one_pass:
        X[24:] = 0
    n = S - 1 if short_ard else S
    A, R, D = np.full((S, B), -1, np.int32), np.full((S, B), np.nan, F), np.full((S, B), np.nan, F)
    A[:n], R[:n], D[:n] = (ring["ra"][idx].T.astype(np.int32)[:n], ring["rr"][idx].T[:n], ring["rd"][idx].T.astype(F)[:n])
    return {"idx": idx, "X": X.reshape((S + 1) * B, RFL), "H0": ring["rh0"][idx].astype(np.uint32) << np.uint32(16),
            "A": A, "R": R, "D": D}


def check_gather(got: dict, ref: dict) -> int:
    """Differing entries between what the kernel wrote and the reference, bit for bit."""
    bad = int((got["X"].reshape(ref["X"].shape) != ref["X"]).sum())
    bad += int((got["H0"].reshape(ref["H0"].shape) != ref["H0"]).sum())
    bad += int((got["A"].reshape(ref["A"].shape) != ref["A"]).sum())
    for k in ("R", "D"):
        bad += int((np.ascontiguousarray(got[k], F).view(np.uint32).reshape(ref[k].shape) != ref[k].view(np.uint32)).sum())
    return bad


# ----------------------------------------------------------------------------- TD
TD_B = [32, 96]
TD_S = [1, 4, 64]
TD_GAMMA_X, TD_COEF_X = 0.5, 2.0 ** -3
TD_GAMMA_R = float(np.float32(0.99))


def td_burns(S):
    return sorted({0, min(1, S - 1), S - 1})


def td_inputs(B, S, exact, seed) -> dict:
    """Q, Qt [(S+1)B][4] (the fourth column NaN: never read), A, R, D [S][B].  Exact: Q in k/4, Qt in k/2,
    R in k/4 with two- and three-way ties in the next step's Q (rows cycle through the tie patterns)."""
    g = np.random.default_rng(seed)
    n1, n = (S + 1) * B, S * B
    if exact:
        Q = (g.integers(-8, 9, (n1, 4)) / 4.0).astype(F)
        pat = np.array([(1, 1, 1), (2, 2, 1), (1, 2, 2), (2, 1, 2), (0, 1, 2), (2, 1, 0), (1, 3, 2), (-1, -1, -2)], F)
        Q[:, :3] = pat[np.arange(n1) % 8] * (0.25 * (1 + np.arange(n1) % 3))[:, None].astype(F)
        Qt = (g.integers(-8, 9, (n1, 4)) / 2.0).astype(F)
        R = (g.integers(-4, 5, n) / 4.0).astype(F)
    else:
        Q, Qt, R = (g.standard_normal(s).astype(F) for s in ((n1, 4), (n1, 4), (n,)))
    Q[:, 3] = np.nan
    Qt[:, 3] = np.nan
    D = (np.arange(n) % 3 == 1).astype(F)
    D[-1] = 1.0
    return {"Q": Q, "Qt": Qt, "A": g.integers(0, 3, n).astype(np.int32), "R": R, "D": D}


def td_ref(inp, B, S, burn, gamma, coef, target_argmax=False, last_tie=False, no_done=False, burn_off=0,
           coef_masked=False):
    """dQ [S*B][4] float64, its bound, and the squared errors that enter the loss.  Bound of the taken
    column: 4u |coef| (|q| + |r| + gamma |qt|) (product, sum, difference, coef)."""
    Q, Qt = inp["Q"].astype(np.float64)[:, :3], inp["Qt"].astype(np.float64)[:, :3]
    n = S * B
    sel = (Qt if target_argmax else Q)[B:B + n]
    a_s = (2 - np.argmax(sel[:, ::-1], axis=1)) if last_tie else np.argmax(sel, axis=1)
    qt = Qt[B:B + n][np.arange(n), a_s]
    live = 1.0 if no_done else (1.0 - inp["D"].astype(np.float64))
    qa = Q[:n][np.arange(n), inp["A"]]
    d = qa - (inp["R"].astype(np.float64) + gamma * live * qt)
    on = (np.arange(n) // B) >= burn + burn_off
    dQ, bound = np.zeros((n, 4)), np.zeros((n, 4))
    dQ[np.arange(n), inp["A"]] = coef * d if coef_masked else np.where(on, coef * d, 0.0)
    bound[np.arange(n), inp["A"]] = 4 * U * abs(coef) * (np.abs(qa) + np.abs(inp["R"]) + gamma * np.abs(qt)) * on
    return dQ, bound, d * d * on, 4 * U * (np.abs(qa) + np.abs(inp["R"]) + gamma * np.abs(qt)) * 2 * np.abs(d) * on


def check_td(got_dq, got_loss, loss0, inp, B, S, burn, gamma, coef, exact):
    """(failures, dQ err/bound, loss err/bound) of one TD launch against td_ref."""
    dQ, bound, sq, dsq = td_ref(inp, B, S, burn, gamma, coef)
    got = np.asarray(got_dq, F).reshape(S * B, 4)
    want = loss0 + sq.sum()
    if exact:
        bad = int((got.view(np.uint32) != dQ.astype(F).view(np.uint32)).sum()) + int(float(got_loss) != want)
        return bad, 0.0, 0.0
    err = np.abs(got.astype(np.float64) - dQ)
    bad = int((err > bound).sum()) + int((got[:, 3].view(np.uint32) != 0).sum())
    bad += int((got[:burn * B].view(np.uint32) != 0).sum())
    lb = (S * B + 4) * U * sq.sum() + dsq.sum()
    le = abs(float(got_loss) - want)
    return bad + int(le > lb), ratio(err, bound), ratio(le, lb)


# ----------------------------------------------------------------------------- weights
def masters(seed: int, heavy: bool = False) -> dict:
    """Hand-built fp32 masters of one net.  heavy: four entries per column of W_hh are 16 times the rest, so
    that a recurrent product is dominated by a few gate rows (the backward's hi/lo test)."""
    g = np.random.default_rng(seed)
    w_hh = (0.06 * g.standard_normal((RG, RH))).astype(F)
    if heavy:
        for u in range(RH):
            w_hh[g.choice(RG, 4, replace=False), u] *= F(16.0)
    w_ih = np.zeros((RG, RFL), F)
    w_ih[:, :RF] = 0.25 * g.standard_normal((RG, RF))
    return {"w_hh": w_hh, "w_ih": w_ih, "b_ih": (0.2 * g.standard_normal(RG)).astype(F),
            "b_hh": (0.2 * g.standard_normal(RG)).astype(F), "w_q": (0.3 * g.standard_normal((3, RH))).astype(F),
            "b_q": (0.5 * g.standard_normal(3)).astype(F)}


def net_from(m: dict, whh_deq=None, whhT_deq=None, bias4=None) -> dict:
    """What the kernels multiply with.  whh_deq / whhT_deq: W_hh as read back from the packed fragments
    (unpack_whh(unscale=False) / unpack_whhT); None: the host model of the pack (mx_roundtrip, 32-blocks along
    K of the pre-scaled rows; along the gate rows for the transposed pack).  bias4: the packed pre-scaled
    biases [4][RH] as read back (None: the host's fp32 arithmetic, which may round differently)."""
    gs = GS.astype(F)
    w = torch.from_numpy(m["w_hh"])
    if whh_deq is None:
        whh_deq = mx_roundtrip(w * torch.from_numpy(gs)[:, None]).numpy()
    if whhT_deq is None:
        whhT_deq = mx_roundtrip(w.t().contiguous()).t().numpy()
    b = np.zeros((4, RH), F)
    s = (m["b_ih"] + m["b_hh"]).astype(F)
    b[0], b[1] = s[:RH] * F(GS_RZ), s[RH:2 * RH] * F(GS_RZ)
    b[2], b[3] = m["b_ih"][2 * RH:] * F(GS_N), m["b_hh"][2 * RH:] * F(GS_N)
    if bias4 is not None:
        b = np.asarray(bias4, F).reshape(4, RH)
    return {"wih": bf((m["w_ih"][:, :RF] * gs[:, None]).astype(F)), "whh": np.asarray(whh_deq, np.float64),
            "whhT": np.asarray(whhT_deq, np.float64), "bias4": b.astype(np.float64), "wq": m["w_q"].astype(np.float64),
            "wq_bf": bf(m["w_q"]), "bq": m["b_q"].astype(np.float64)}


# ----------------------------------------------------------------------------- forward
FWD_B = [32, 96]
FWD_S_RESET = [1, 2, 3, 24, 64]
FWD_CHAIN = (32, 64)     # (B, S) of the chain case (16 nudged reference runs: kept to one forward block)
NUDGE_RUNS, CHAIN_FACTOR = 8, 4.0


def fwd_inputs(B, S, pattern, seed) -> dict:
    """x [S+1][B][RF] (bf16 values), H0 [B][RH] on the MX-fp8 grid of its 32-unit blocks, D [S][B].
    pattern 'ones': every step ends an episode; 'mixed': episodes of 1..4 steps (0..3 un-reset steps, then
    one that ends the episode), the lengths cycling per sequence (sequence b starts the cycle at b % 4)."""
    g = np.random.default_rng(seed)
    x = bf(g.standard_normal((S + 1, B, RF)).astype(F))
    h0 = mxrt(0.5 * g.standard_normal((B, RH)))
    if pattern == "ones":
        D = np.ones((S, B), F)
    else:
        D = np.zeros((S, B), F)
        for b in range(B):
            t, k = -1, b
            while True:
                t += 1 + k % 4        # k % 4 un-reset steps, then a step that ends the episode
                k += 1
                if t >= S:
                    break
                D[t, b] = 1.0
    return {"x": x, "h0": h0, "D": D}


def _sig(a):
    return 1.0 / (1.0 + np.exp2(a))


def fwd_ref(inp, net, B, S, rng=None, keep_first=False, swap_x=False, gh_scaled=False, hp_after=False, wih=None):
    """The quantisation-aware unroll in float64 and the counted one-step error of each quantity, given an
    exact start of the step.  Returns sv [5][S][B][RH], their deltas, hm [S][B][RH] (masked h after step t,
    HT block t + 1) with delta, Q [S+1][B][3] with the accumulation bound and the bf16 flip allowance, and
    tight [S+1][B]: the step started from an exactly representable h (h = 0 after a reset, H0 at step 0).
    rng: nudge every h by +- its one-step delta just before each re-quantisation (the flip-noise runs).
    Mutations: keep_first (mask before the Q head), swap_x (x_t and x_t+1 trade places), gh_scaled,
    hp_after, wih (another net's W_ih)."""
    x, D = inp["x"], inp["D"].astype(np.float64)
    Wi, Wh, b4 = (net["wih"] if wih is None else wih), net["whh"], net["bias4"]
    h = inp["h0"].copy()
    sv, dl = np.zeros((NSV, S, B, RH)), np.zeros((NSV, S, B, RH))
    hm, dhm = np.zeros((S, B, RH)), np.zeros((S, B, RH))
    Q, dQa, dQf = np.zeros((S + 1, B, 3)), np.zeros((S + 1, B, 3)), np.zeros((S + 1, B, 3))
    tight = np.zeros((S + 1, B), bool)
    dh_in = np.zeros((B, RH))
    for t in range(S + 1):
        if rng is not None:
            h = h + dh_in * rng.choice([-1.0, 1.0], size=h.shape)
        hq = mxrt(h)
        tight[t] = (hq == h).all(1)
        xt = x[(t ^ 1) if (swap_x and (t ^ 1) <= S) else t]
        gx, gh = xt @ Wi.T, hq @ Wh.T
        ax, ah = np.abs(xt) @ np.abs(Wi).T, np.abs(hq) @ np.abs(Wh).T
        cnt = (RF + RH + 8) * U
        a_r, a_z = (b4[g] + gx[:, g * RH:(g + 1) * RH] + gh[:, g * RH:(g + 1) * RH] for g in (0, 1))
        e_r, e_z = (cnt * (np.abs(b4[g]) + ax[:, g * RH:(g + 1) * RH] + ah[:, g * RH:(g + 1) * RH]) for g in (0, 1))
        anx, anh = b4[2] + gx[:, 2 * RH:], b4[3] + gh[:, 2 * RH:]
        e_nx, e_nh = cnt * (np.abs(b4[2]) + ax[:, 2 * RH:]), cnt * (np.abs(b4[3]) + ah[:, 2 * RH:])
        r, z = _sig(a_r), _sig(a_z)
        d_r, d_z = r * (1 - r) * LN2 * e_r + 6 * U * r, z * (1 - z) * LN2 * e_z + 6 * U * z
        y = r * anh + anx
        e_y = np.abs(anh) * d_r + r * e_nh + e_nx + U * np.abs(y)
        s = _sig(y)
        n = 2 * s - 1
        d_n = 2 * (s * (1 - s) * LN2 * e_y + 6 * U * s) + U * np.abs(n)
        ghn = anh / GS_N
        d_g = e_nh / abs(GS_N) + 2 * U * np.abs(ghn)
        hn = z * (h - n) + n
        d_h = d_z * np.abs(h - n) + z * (d_n + U * np.abs(h - n)) + d_n + U * np.abs(hn)
        if t < S:
            for q, v, e in ((SV_R, r, d_r), (SV_Z, z, d_z), (SV_N, n, d_n), (SV_GH, anh if gh_scaled else ghn, d_g),
                            (SV_HP, hn if hp_after else h, 0.0)):
                sv[q, t], dl[q, t] = v, e
        keep = (1.0 - D[t])[:, None] if t < S else 1.0
        hq_in = hn * keep if keep_first else hn
        hb = bf16_round64(hq_in)
        Q[t] = net["bq"] + hb @ net["wq_bf"].T
        dQa[t] = (RF + RW + 4) * U * (np.abs(net["bq"]) + np.abs(hb) @ np.abs(net["wq_bf"]).T)
        dQf[t] = np.abs(bf16_round64(hq_in + d_h) - bf16_round64(hq_in - d_h)) @ np.abs(net["wq_bf"]).T
        h = hn * keep
        dh_in = d_h * keep
        if t < S:
            hm[t], dhm[t] = h, dh_in
    return {"sv": sv, "dsv": dl, "hm": hm, "dhm": dhm, "Q": Q, "dQa": dQa, "dQf": dQf, "tight": tight}


def fwd_chain_bound(inp, net, B, S, seed=7) -> dict:
    """The flip-noise floor of a chain across un-reset steps, measured on the reference: the largest
    difference, per quantity and step, between the plain run and NUDGE_RUNS runs whose h is nudged by +- the
    counted one-step delta before each re-quantisation.  (Multiply by CHAIN_FACTOR for the kernel's bound.)"""
    base = fwd_ref(inp, net, B, S)
    out = {"sv": np.zeros((NSV, S)), "hm": np.zeros(S), "Q": np.zeros(S + 1)}
    for k in range(NUDGE_RUNS):
        run = fwd_ref(inp, net, B, S, rng=np.random.default_rng(seed + k))
        out["sv"] = np.maximum(out["sv"], np.abs(run["sv"] - base["sv"]).max(axis=(2, 3)))
        out["hm"] = np.maximum(out["hm"], np.abs(run["hm"] - base["hm"]).max(axis=(1, 2)))
        out["Q"] = np.maximum(out["Q"], np.abs(run["Q"] - base["Q"]).max(axis=(1, 2)))
    return out


def check_fwd(ref, sv_bits, ht_bits, Qgot, B, S, chain=None, chain_only=False):
    """(failures, {quantity: largest err/bound}) of one net's forward outputs against fwd_ref.
    sv_bits [5][S][B][RH] and ht_bits [S][B][RH] (HT blocks 0..S-1) are None for the target net.  Steps that
    started from an exact h get the counted bound; the others need ``chain`` (fwd_chain_bound) and get
    CHAIN_FACTOR times the measured floor on top of it, or are skipped when chain is None.  chain_only: count
    the steps inside runs alone (the CPU test's proof that the chain bound by itself tells the mutations)."""
    bad, worst = 0, {}
    tight = ref["tight"]
    live = ~tight if chain_only else (tight | (chain is not None))     # [S+1][B]: the steps that are checked

    def iv(name, bits, val, delta, mask):
        nonlocal bad
        bad += int((~(interval_ok(bits, val, delta) | ~mask)).sum())
        worst[name] = max(worst.get(name, 0.0), interval_ratio(bits, val, delta, mask))

    if sv_bits is not None:
        for q in range(NSV):
            extra = 0.0 if chain is None else CHAIN_FACTOR * chain["sv"][q][:, None, None]
            m = np.broadcast_to(live[:S, :, None], (S, B, RH))
            iv(SV_NAMES[q], sv_bits[q], ref["sv"][q], ref["dsv"][q] + np.where(tight[:S, :, None], 0.0, extra), m)
        # HT block 0 = h0 (exact); block t + 1 = the masked h_t
        if not chain_only:
            bad += int((bf16_val(ht_bits[0]).reshape(B, RH) != ref["sv"][SV_HP, 0]).sum())
        if S > 1:
            extra = 0.0 if chain is None else CHAIN_FACTOR * chain["hm"][:S - 1, None, None]
            m = np.broadcast_to(live[:S - 1, :, None], (S - 1, B, RH))
            iv("HT", ht_bits[1:], ref["hm"][:S - 1], ref["dhm"][:S - 1] + np.where(tight[:S - 1, :, None], 0.0, extra), m)
    Qg = np.asarray(Qgot, F).reshape(S + 1, B, 4)
    bad += int((Qg[:, :, 3].view(np.uint32) != 0).sum())
    bound = ref["dQa"] + ref["dQf"]
    m = np.broadcast_to(live[:, :, None], bound.shape)
    if chain is not None:
        bound = bound + np.where(tight[:, :, None], 0.0, CHAIN_FACTOR * chain["Q"][:, None, None])
    err = np.where(m, np.abs(Qg[:, :, :3].astype(np.float64) - ref["Q"]), 0.0)
    bad += int((err > bound).sum())
    worst["Q"] = ratio(err, bound)
    return bad, worst


# ----------------------------------------------------------------------------- backward
BWD_B = [32, 96]
GQ_STRIDE = 3 * RH + 4


def bwd_inputs(B, S, burn, seed, D="random") -> dict:
    """Hand-built saves (bf16 values): r, z in (0, 1), n in (-1, 1), gh_n and h_prev moderate; dQ random with
    zero rows for t < burn (fourth column NaN: never read); D random, all ones or all zeros."""
    g = np.random.default_rng(seed)
    shp = (S, B, RH)
    sv = np.stack([bf(g.uniform(0.02, 0.98, shp).astype(F)), bf(g.uniform(0.02, 0.98, shp).astype(F)),
                   bf(g.uniform(-0.98, 0.98, shp).astype(F)), bf(g.standard_normal(shp).astype(F)),
                   bf((0.5 * g.standard_normal(shp)).astype(F))])
    dQ = np.full((S, B, 4), np.nan, F)
    dQ[:, :, :3] = g.standard_normal((S, B, 3)) * (g.random((S, B, 3)) < 0.5)
    dQ[:burn, :, :3] = 0.0
    Dv = {"random": (g.random((S, B)) < 0.3), "ones": np.ones((S, B)), "zeros": np.zeros((S, B))}[D]
    return {"sv": sv, "dQ": dQ, "D": np.asarray(Dv, F)}


def quant_hilo_model(x):
    """The kernel's MX-fp8 hi/lo pair of dGh [rows][768] (32-row blocks): dequantised hi and lo."""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=F))
    hi = mx_roundtrip(xt)
    lo = mx_roundtrip(xt - hi)
    return hi.double().numpy(), lo.double().numpy()


def hilo_bound(x):
    """Counted bound on |x - hi - lo| per element: each half is one e4m3 rounding (relative 2^-4 of a normal,
    2^-10 of the block's scale below that) under the block's own scale 2^e <= amax / 224."""
    a = np.abs(np.asarray(x, np.float64))
    blk = a.reshape(a.shape[0], -1, 32)
    res = np.maximum(blk / 16.0, blk.max(-1, keepdims=True) / (224.0 * 1024.0))
    return np.maximum(res / 16.0, res.max(-1, keepdims=True) / (224.0 * 1024.0)).reshape(a.shape)


def bwd_ref(inp, net, B, S, keep_next=False, keep_last=False, keep_zero_early=False, gx_as_gh=False, no_1mr=False,
            swap_blk=False, masked_h=False, gbq_one_tile=False, drop_lo=False):
    """The kernel's definition of the backward in float64, with the counted error of every output propagated
    through the reference's own recurrence.  Returns dGh, dGx [S][B][RG] with deltas, and per backward
    workgroup (16 sequences) gwq [B/16][3][RH], gbq [B/16][3] with the sums of their terms' magnitudes.
    Mutations: keep_next (pkeep from D[t+1]), keep_last (pkeep = 1 - D at t = S-1: without effect, rec starts
    at zero), keep_zero_early (pkeep zero from t = S-2 on), gx_as_gh, no_1mr, swap_blk (fn and fblk traded in
    the saves' address; wrapped into range), masked_h, gbq_one_tile, drop_lo."""
    sv, D = inp["sv"], inp["D"].astype(np.float64)
    dQ = np.nan_to_num(inp["dQ"].astype(np.float64)[:, :, :3])
    if swap_blk:
        src = np.array([(bwd_block(b // LBB, True)[0] * LB + 16 * bwd_block(b // LBB, True)[1] + b % 16) % B for b in range(B)])
        sv = sv[:, :, src]
    W, wq = net["whhT"], net["wq"]
    aW = np.abs(W)
    nwg = B // LBB
    dGh, dGx, eGh, eGx = (np.zeros((S, B, RG)) for _ in range(4))
    gwq, agwq, egwq = (np.zeros((nwg, 3, RH)) for _ in range(3))
    gbq, agbq = np.zeros((nwg, 3)), np.zeros((nwg, 3))
    rec, erec = np.zeros((B, RH)), np.zeros((B, RH))
    for t in range(S - 1, -1, -1):
        r, z, n, gh, hp = sv[:, t]
        if keep_next:
            keep = (1.0 - D[t + 1]) if t < S - 1 else np.zeros(B)
        elif t == S - 1:
            keep = (1.0 - D[t]) if keep_last else np.zeros(B)
        else:
            keep = np.zeros(B) if (keep_zero_early and t >= S - 2) else 1.0 - D[t]
        keep = keep[:, None]
        dh = keep * rec + dQ[t] @ wq
        e_dh = 4 * U * (np.abs(keep * rec) + np.abs(dQ[t]) @ np.abs(wq)) + keep * erec
        h = z * (hp - n) + n
        e_h = 2 * U * (np.abs(z * (hp - n)) + np.abs(n))
        hq = h * (1.0 - D[t])[:, None] if masked_h else h
        for a in range(3):
            term = (dQ[t][:, a:a + 1] * hq).reshape(nwg, LBB, RH)
            gwq[:, a] += term.sum(1)
            agwq[:, a] += np.abs(term).sum(1)
            egwq[:, a] += (np.abs(dQ[t][:, a:a + 1]) * e_h).reshape(nwg, LBB, RH).sum(1)
        dq_wg = dQ[t].reshape(nwg, LBB, 3)
        tile = (np.arange(nwg) % 2 == 0)[:, None] if gbq_one_tile else 1.0
        gbq += dq_wg.sum(1) * tile
        agbq += np.abs(dq_wg).sum(1)
        omn = 1.0 - n * n
        a_n = dh * (1.0 - z) * omn
        e_an = e_dh * np.abs((1.0 - z) * omn) + np.abs(a_n) * (3 * U + U / omn)
        omr = 1.0 if no_1mr else (1.0 - r)
        g0 = a_n * gh * r * omr
        e0 = e_an * np.abs(gh * r * (1.0 - r)) + 4 * U * np.abs(g0)
        dz = dh * (hp - n)
        e_dz = e_dh * np.abs(hp - n) + 2 * U * np.abs(dz)
        g1 = dz * z * (1.0 - z)
        e1 = e_dz * z * (1.0 - z) + 3 * U * np.abs(g1)
        g2 = a_n * r
        e2 = e_an * r + U * np.abs(g2)
        dGh[t], eGh[t] = np.concatenate([g0, g1, g2], 1), np.concatenate([e0, e1, e2], 1)
        dGx[t] = np.concatenate([g0, g1, g2 if gx_as_gh else a_n], 1)
        eGx[t] = np.concatenate([e0, e1, e_an], 1)
        if t > 0:
            nrec = dh * z
            x = dGh[t]
            if drop_lo:
                x = quant_hilo_model(x)[0]
            rec = nrec + x @ W
            qe = hilo_bound(np.abs(dGh[t]) + eGh[t]) + eGh[t]
            erec = e_dh * z + U * np.abs(nrec) + qe @ aW + (2 * RG + 8) * U * (np.abs(nrec) + np.abs(dGh[t]) @ aW)
    return {"dGh": dGh, "dGx": dGx, "eGh": eGh, "eGx": eGx, "gwq": gwq, "agwq": agwq, "egwq": egwq, "gbq": gbq,
            "agbq": agbq}


def bwd_store(ref, B, S):
    """A backward result as the kernel stores it: dGhT / dGxT bits [RG][S*B]; per-workgroup fp32 rows."""
    out = {}
    for k in ("dGh", "dGx"):
        out[k + "T"] = bf16_bits(ref[k].astype(F)).reshape(S * B, RG).T.copy()
    out["gwq"], out["gbq"] = ref["gwq"].astype(F), ref["gbq"].astype(F)
    return out


def check_bwd(got, ref, B, S, gwq0=None, gbq0=None):
    """(failures, {name: err/bound}).  got: dGhT, dGxT bits [RG][S*B]; gwq, gbq either per workgroup
    ([B/16][3][RH], [B/16][3]: the ordered path, gwq0 None) or summed onto the start values gwq0 [3][RH],
    gbq0 [3] (the atomic path)."""
    bad, worst = 0, {}
    for k in ("dGh", "dGx"):
        bits = np.asarray(got[k + "T"], np.uint16).reshape(RG, S * B).T.reshape(S, B, RG)
        ok = interval_ok(bits, ref[k], ref["e" + k[1:]])
        bad += int((~ok).sum())
        worst[k] = interval_ratio(bits, ref[k], ref["e" + k[1:]])
    nwg = B // LBB
    if gwq0 is None:
        wg, wa, we, bg, ba = ref["gwq"], ref["agwq"], ref["egwq"], ref["gbq"], ref["agbq"]
        cw, cb = (S + 8) * U, (S + 10) * U
    else:
        wg, wa, we = gwq0 + ref["gwq"].sum(0), np.abs(gwq0) + ref["agwq"].sum(0), ref["egwq"].sum(0)
        bg, ba = gbq0 + ref["gbq"].sum(0), np.abs(gbq0) + ref["agbq"].sum(0)
        cw, cb = (S + 8 + nwg) * U, (S + 10 + nwg) * U
    ew = np.abs(np.asarray(got["gwq"], np.float64).reshape(wg.shape) - wg)
    eb = np.abs(np.asarray(got["gbq"], np.float64).reshape(bg.shape) - bg)
    bad += int((ew > cw * wa + we).sum()) + int((eb > cb * ba).sum())
    worst["gwq"], worst["gbq"] = ratio(ew, cw * wa + we), ratio(eb, cb * ba)
    return bad, worst


# ----------------------------------------------------------------------------- Q-gradient reduce, fixup
REDUCE_ROWS = [1, 2, 7]


def reduce_inputs(rows, stride, exact, seed):
    """Partial rows [rows][stride]; the padding past 3 RH + 3 is NaN.  Exact: dyadic values of very different
    sizes, whose fp32 sum depends on the order (row 0 large, the rest small: added in index order the small
    ones are lost one by one, in any other order some survive)."""
    g = np.random.default_rng(seed)
    p = np.full((rows, stride), np.nan, F)
    n = 3 * RH + 3
    if exact:
        p[:, :n] = 1.0
        p[0, :n] = 2.0 ** 24 * (1 + np.arange(n) % 3)
    else:
        p[:, :n] = g.standard_normal((rows, n))
    return p


def reduce_ref(p, reverse=False):
    """numpy float32 sum of the rows in index order: [3 RH + 3]."""
    n = 3 * RH + 3
    s = np.zeros(n, F)
    for b in (range(p.shape[0] - 1, -1, -1) if reverse else range(p.shape[0])):
        s = (s + p[b, :n]).astype(F)
    return s


def fixup_ref(ext, dwih, ldx, col=RF):
    """dwhh, dbhh, dbih, and dwih after the launch.  col: the column db_ih is taken from (mutation: RF - 1)."""
    e = ext.reshape(RG, ldx)
    w = dwih.reshape(RG, RFL).copy()
    dbih = w[:, col].copy()
    w[:, col] = 0.0
    return {"dwhh": e[:, :RH].copy(), "dbhh": e[:, RH].copy(), "dbih": dbih, "dwih": w}
