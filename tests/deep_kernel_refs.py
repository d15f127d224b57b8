"""Host references and case builders for the kernels of csrc/deep.hip (no GPU, no torch).

tests/test_gpu_deep_kernels.py compares the kernels with these on the GPU; tests/test_deep_kernel_refs.py
mutates them on the CPU and shows that the same comparisons would notice.  Where the kernel pins every
rounding (trade_rule.h's _rn forms: the env step) the mirror is numpy float32, one operation per rounding;
everything else is float64 with an error bound counted from the kernel's operations (u = 2^-24).
Random draws come from sharetrade.utils.rng (pinned by tests/test_oracle.py)."""
import numpy as np

from sharetrade.utils.rng import philox4x32, u24

U = 2.0 ** -24
F = np.float32
RING_KEYS = ("env", "pos", "budget", "shares", "action", "reward", "budget2", "shares2", "done")
RING_F32 = ("budget", "reward", "budget2")
KEY0, KEY1 = 0x9E3779B9, 0x0BADC0DE


def f32(x) -> float:
    """A hyper-parameter as the kernel receives it."""
    return float(np.float32(x))


# ----------------------------------------------------------------------------- bf16
def bf16_bits(x) -> np.ndarray:
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_val(bits) -> np.ndarray:
    """bf16 bit patterns -> their values (float64)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def bf16_round64(x) -> np.ndarray:
    """float64 -> the nearest bf16 value (ties to even), in one rounding."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.rint(x / q) * q


def interval_ok(got_bits, ref, delta) -> np.ndarray:
    """The stored bf16 lies between rne_bf16(ref - delta) and rne_bf16(ref + delta)."""
    v = bf16_val(got_bits).reshape(np.shape(ref))
    return (bf16_round64(ref - delta) <= v) & (v <= bf16_round64(ref + delta))


def interval_off(got_bits, ref) -> int:
    """Entries whose stored bf16 is not rne_bf16(ref) itself (they needed the interval's slack): the figure
    printed beside an interval check."""
    return int((bf16_val(got_bits).reshape(np.shape(ref)) != bf16_round64(ref)).sum())


def ratio(err, bound) -> float:
    """Largest err / bound (0 / 0 counts as 0, x / 0 as inf)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


# ----------------------------------------------------------------------------- gather
GATHER_SHAPES = [(5, 8), (8, 12), (200, 204), (200, 256), (201, 204), (254, 256)]   # (H, in_p)
GATHER_B = [1, 3, 4, 5, 67]
RINGS = [(7, 1), (7, 5), (64, 64)]          # (cap, size)
SAMPLE_STEPS = [0, 3, 2 ** 32 + 1]
ZERO_N = [0, 1, 3, 4, 5, 1027]
INV_B0 = f32(1.0 / 2000.0)


def price_bank(E: int, T: int, seed: int) -> np.ndarray:
    """[E, T] fp32 prices around 50 (normal range, all distinct enough that a shifted window shows)."""
    g = np.random.default_rng(seed)
    return (50.0 * np.exp(0.05 * g.standard_normal((E, T)))).astype(F)


def gather_env_case(H: int, B: int, seed: int) -> dict:
    """Env-mode inputs: T = H + 4; pos holds 0 and T - H - 1, the last row at T - H - 1 (its pr[H] is the
    bank's final element)."""
    T = H + 4
    g = np.random.default_rng(seed)
    pos = g.integers(0, T - H, B).astype(np.int32)
    pos[0] = 0
    pos[B - 1] = T - H - 1
    if B > 2:
        pos[1] = T - H - 1
    return {"T": T, "prices": price_bank(B, T, seed + 1), "pos": pos,
            "budget": (2000.0 * g.random(B) + 1.0).astype(F), "shares": g.integers(0, 40, B).astype(np.int32)}


def gather_ref(prices, T, H, in_p, feat_mode, inv_b0, e, pos, b, s, nxt=False, shift=True, new_norm=True):
    """Features of rows (e, pos, b, s) in float64 and the fp32 error bound of each column.

    nxt: the x' row (window shifted by one, normalised by the new price pr[H]; b, s are budget2, shares2).
    shift / new_norm = False are the mutations of tests/test_deep_kernel_refs.py.
    Bounds: price columns 4u max(1, |w/last|) (reciprocal, product, subtraction); budget 2u |f|; shares 3u |f|.
    feat_mode 0 does no arithmetic: bound 0."""
    flat = np.asarray(prices, F).reshape(-1)
    e, pos = np.asarray(e, np.int64), np.asarray(pos, np.int64)
    n = e.shape[0]
    base = e * T + pos
    off = 1 if (nxt and shift) else 0
    w = flat[base[:, None] + off + np.arange(H)[None, :]].astype(np.float64)
    last = flat[base + H - 1 + (1 if (nxt and new_norm) else 0)].astype(np.float64)
    ref = np.zeros((n, in_p))
    dl = np.zeros((n, in_p))
    bb, ss = np.asarray(b, F).astype(np.float64), np.asarray(s, np.int64).astype(np.float64)
    if feat_mode:
        rel = w / last[:, None]
        ref[:, :H] = rel - 1.0
        dl[:, :H] = 4 * U * np.maximum(1.0, np.abs(rel))
        ref[:, H] = bb * inv_b0
        dl[:, H] = 2 * U * np.abs(ref[:, H])
        ref[:, H + 1] = ss * last * inv_b0
        dl[:, H + 1] = 3 * U * np.abs(ref[:, H + 1])
    else:
        ref[:, :H] = w
        ref[:, H] = bb
        ref[:, H + 1] = ss
    return ref, dl


def sample_index(B: int, step: int, size: int, key0=KEY0, key1=KEY1, hi_word=True) -> np.ndarray:
    """The replay gather's draw per row: counter (row, step_lo, step_hi, 7), ((c0 << 32) | c1) % size."""
    rows = np.arange(B, dtype=np.uint32)
    c1 = np.full(B, step & 0xFFFFFFFF, np.uint32)
    c2 = np.full(B, ((step >> 32) & 0xFFFFFFFF) if hi_word else 0, np.uint32)
    r0, r1, _, _ = philox4x32(rows, c1, c2, np.full(B, 7, np.uint32), np.full(B, key0, np.uint32),
                              np.full(B, key1, np.uint32))
    return np.array([((int(a) << 32) | int(b)) % max(int(size), 1) for a, b in zip(r0, r1)], dtype=np.int64)


def make_ring(cap: int, size: int, E: int, T: int, H: int, seed: int) -> dict:
    """A ring with ``size`` live records; stale slots hold in-range indices and NaN floats (a read of one
    shows as a wrong value, never as an out-of-range address)."""
    g = np.random.default_rng(seed)
    r = {"env": g.integers(0, E, cap).astype(np.int32), "pos": g.integers(0, T - H, cap).astype(np.int32),
         "budget": (2000.0 * g.random(cap) + 1.0).astype(F), "shares": g.integers(0, 40, cap).astype(np.int32),
         "action": g.integers(0, 3, cap).astype(np.int32), "reward": g.standard_normal(cap).astype(F),
         "budget2": (2000.0 * g.random(cap) + 1.0).astype(F), "shares2": g.integers(0, 40, cap).astype(np.int32),
         "done": g.integers(0, 2, cap).astype(np.int32)}
    r["pos"][0] = T - H - 1          # a live record whose x' ends at the bank row's final element
    r["env"][0] = E - 1
    r["done"][: min(2, size)] = [1, 0][: min(2, size)]
    for k in RING_F32:
        r[k][size:] = np.nan
    # stale slots differ from every live one in their integer fields too, where the range allows
    r["shares"][size:] = 77
    r["shares2"][size:] = 78
    return r


def replay_sample_ref(ring, prices, T, H, in_p, feat_mode, inv_b0, B, step, size, **mut):
    """What the replay gather must produce for B rows: dict with idx, a, r, done and (ref, delta) of X, Xn.
    mut: shift / new_norm (x' mutations), mod (the modulus instead of size), hi_word; key0 / key1."""
    idx = sample_index(B, step, mut.get("mod", size), mut.get("key0", KEY0), mut.get("key1", KEY1),
                       hi_word=mut.get("hi_word", True))
    e, ps = ring["env"][idx], ring["pos"][idx]
    X = gather_ref(prices, T, H, in_p, feat_mode, inv_b0, e, ps, ring["budget"][idx], ring["shares"][idx])
    Xn = gather_ref(prices, T, H, in_p, feat_mode, inv_b0, e, ps, ring["budget2"][idx], ring["shares2"][idx],
                    nxt=True, shift=mut.get("shift", True), new_norm=mut.get("new_norm", True))
    return {"idx": idx, "a": ring["action"][idx].copy(), "r": ring["reward"][idx].copy(),
            "done": ring["done"][idx].astype(F), "X": X, "Xn": Xn}


# ----------------------------------------------------------------------------- env step
ENV_E = [1, 63, 64, 65, 256, 300]
ENV_LDQ = [3, 64]
ENV_EPS = [(0.0, 1.0), (1.0, 1e9), (0.5, 0.25)]
ENV_H, ENV_T = 6, 12
ENV_B0, ENV_S0 = 2000.0, 3


def env_case(E: int, k: int) -> dict:
    """Settings of env case k (varied together): cap in {E, E + 3, 2E + 5} with a starting cursor that makes
    the second launch wrap inside its E slots, compat_env, (eps, inv_ramp), ldq."""
    cap, cur = [(E, E // 2), (E + 3, 1), (2 * E + 5, E // 2 + 3)][k % 3]
    eps, inv_ramp = ENV_EPS[(k // 3 + k) % 3]
    return {"E": E, "T": ENV_T, "H": ENV_H, "cap": cap, "cursor": cur, "compat": (k // 3) % 2, "eps": f32(eps),
            "inv_ramp": f32(inv_ramp), "ldq": ENV_LDQ[k % 2], "n_actions": 3, "b0": ENV_B0, "s0": ENV_S0,
            "step0": [5, 2 ** 32 - 2, 0][k % 3]}


def env_state(E: int, seed: int) -> dict:
    """Env state with envs that cannot afford a buy, envs without a share, and envs at pos = T - H - 1."""
    g = np.random.default_rng(seed)
    T, H = ENV_T, ENV_H
    i = np.arange(E)
    pos = (i % (T - H)).astype(np.int32)
    pos[E - 1] = T - H - 1
    prices = price_bank(E, T, seed + 1)
    budget = (1000.0 + 1000.0 * g.random(E)).astype(F)
    budget[i % 4 == 1] = F(10.0)                       # below every price
    shares = g.integers(1, 9, E).astype(np.int32)
    shares[i % 5 == 2] = 0
    value = np.where(pos > 0, prices[i, np.maximum(pos + H - 1, 0)], F(0)).astype(F)
    return {"prices": prices, "budget": budget, "shares": shares, "value": value, "pos": pos,
            "episodes": (i % 3).astype(np.int32), "last_final": np.full(E, 123.5, F)}


def env_q(E: int, ldq: int, seed: int) -> np.ndarray:
    """Hand-built Q rows with exact ties: row e cycles through every tie pattern of three actions."""
    g = np.random.default_rng(seed)
    q = g.standard_normal((E, ldq)).astype(F)
    pat = [(1, 1, 1), (2, 2, 1), (1, 2, 2), (2, 1, 2), (0, 1, 2), (2, 1, 0), (1, 3, 2), (-1, -1, -2)]
    for e in range(E):
        q[e, :3] = np.array(pat[e % len(pat)], F) * F(0.25 + (e % 7))
    return q


def env_ring0(cap: int) -> dict:
    """The ring before the first launch: in-range indices, NaN floats."""
    r = {k: np.zeros(cap, F if k in RING_F32 else np.int32) for k in RING_KEYS}
    for k in RING_F32:
        r[k][:] = np.nan
    r["shares"][:] = -5
    r["action"][:] = 2
    r["done"][:] = 1
    return r


def env_draws(E: int, step: int, key0=KEY0, key1=KEY1):
    e = np.arange(E, dtype=np.uint32)
    r0, r1, _, _ = philox4x32(e, np.full(E, step & 0xFFFFFFFF, np.uint32), np.full(E, (step >> 32) & 0xFFFFFFFF, np.uint32),
                              np.zeros(E, np.uint32), np.full(E, key0, np.uint32), np.full(E, key1, np.uint32))
    return u24(r0), u24(r1)


def env_mirror(c: dict, st: dict, ring: dict, q: np.ndarray, cursor: int, step: int, *, wrap=True, done_gt=False,
               use_compat=True, last_max=False):
    """One deep_env_step launch in numpy float32, one operation per rounding (trade_rule.h).  Returns the new
    state, the new ring and per-env (action, reward, explore, done, final value).
    Mutations: wrap=False (slot without the modulo), done_gt (done at np > T - H), use_compat=False,
    last_max (ties resolve to the last maximum)."""
    E, T, H, cap = c["E"], c["T"], c["H"], c["cap"]
    e = np.arange(E)
    u1, u2 = env_draws(E, step, c.get("key0", KEY0), c.get("key1", KEY1))
    ps = st["pos"].astype(np.int64)
    thr = np.minimum(F(c["eps"]), ps.astype(F) * F(c["inv_ramp"]))
    exploit = u1 < thr
    qa = q[:, : c["n_actions"]]
    greedy = (qa.shape[1] - 1 - np.argmax(qa[:, ::-1], axis=1)) if last_max else np.argmax(qa, axis=1)
    rnd = np.minimum((u2 * F(3.0)).astype(np.int32), 2)
    a = np.where(exploit, greedy, rnd).astype(np.int32)
    vnew = st["prices"][e, np.minimum(ps + H, T - 1)]   # (the clamp acts only under the done_gt mutation)
    b, s, vprev = st["budget"], st["shares"], st["value"]
    compat = c["compat"] and use_compat
    bd = np.full(E, c["b0"], F) if compat else b
    sd = np.full(E, c["s0"], np.int32) if compat else s
    buy, sell = (a == 0) & (bd >= vnew), (a == 1) & (sd > 0)
    b2 = np.where(buy, bd - vnew, np.where(sell, bd + vnew, bd)).astype(F)
    s2 = np.where(buy, sd + 1, np.where(sell, sd - 1, sd)).astype(np.int32)
    cur = b + s.astype(F) * vprev
    nw = b2 + s2.astype(F) * vnew
    rew = (nw - cur).astype(F)
    npos = ps + 1
    done = (npos > T - H) if done_gt else (npos >= T - H)
    slot = (cursor + e) % cap if wrap else np.minimum(cursor + e, cap - 1)   # (the mutation stays in range)
    ring = {k: v.copy() for k, v in ring.items()}
    for k, v in (("env", e), ("pos", ps), ("budget", b), ("shares", s), ("action", a), ("reward", rew),
                 ("budget2", b2), ("shares2", s2), ("done", done)):
        ring[k][slot] = v
    fin = (b2 + s2.astype(F) * vnew).astype(F)
    new = dict(st)
    new["budget"] = np.where(done, F(c["b0"]), b2).astype(F)
    new["shares"] = np.where(done, c["s0"], s2).astype(np.int32)
    new["value"] = np.where(done, F(0), vnew).astype(F)
    new["pos"] = np.where(done, 0, npos).astype(np.int32)
    new["episodes"] = (st["episodes"] + done).astype(np.int32)
    new["last_final"] = np.where(done, fin, st["last_final"]).astype(F)
    return new, ring, {"a": a, "rew": rew, "explore": ~exploit, "done": done, "fin": fin, "rnd": rnd, "u1": u1, "u2": u2}


# ----------------------------------------------------------------------------- TD
TD_B = [1, 63, 64, 65, 200]
TD_LD = [(3, 3), (4, 4), (64, 3), (64, 1)]     # (ldq, n_actions)
GAMMA_X, COEF_X = 0.5, 0.125                    # the exact case's gamma and coef
GAMMA_R, COEF_R = f32(0.99), f32(2.0 / 200.0)


def td_inputs(B: int, ldq: int, nact: int, exact: bool, seed: int) -> dict:
    """q, qt [B, ldq], r, a, done.  Exact: q in k/4 (|k| <= 8), r in k/4 (|k| <= 4), qt in k/2 (|k| <= 8), so
    with gamma = 1/2 every diff is k/4 with |k| <= 20 and coef * diff (coef = 1/8) is exact in bf16; the loss
    is a sum of k^2 / 16 below 2^24 / 16."""
    g = np.random.default_rng(seed)
    if exact:
        q = (g.integers(-8, 9, (B, ldq)) / 4.0).astype(F)
        qt = (g.integers(-8, 9, (B, ldq)) / 2.0).astype(F)
        r = (g.integers(-4, 5, B) / 4.0).astype(F)
    else:
        q, qt, r = (g.standard_normal(s).astype(F) for s in ((B, ldq), (B, ldq), (B,)))
    done = (np.arange(B) % 3 == 1).astype(F)
    if B > 1:
        done[-1] = 1.0
    a = g.integers(0, nact, B).astype(np.int32)
    return {"q": q, "qt": qt, "r": r, "a": a, "done": done}


def td_ref(q, qt, r, a, done, nact, gamma, coef):
    """float64: dq value per row, its fp32 bound 4u |coef| (|q| + |r| + gamma |max qt|), diff."""
    q, qt, r, done = (np.asarray(x, F).astype(np.float64) for x in (q, qt, r, done))
    mx = qt[:, :nact].max(1)
    qa = q[np.arange(q.shape[0]), a]
    diff = qa - (r + gamma * (1.0 - done) * mx)
    return coef * diff, 4 * U * abs(coef) * (np.abs(qa) + np.abs(r) + gamma * np.abs(mx)), diff


# ----------------------------------------------------------------------------- head
HEAD_SHAPES = [(64, 256), (128, 512), (512, 512), (576, 256)]   # (B, H)
HEAD_NQP = [1, 4, 17]


def head_map(B: int, H: int, L: int):
    """deep_head_kernel's block -> (row block, column block)."""
    nx, ny = H // 256, B // 64
    if ny % 8 == 0:
        xcd, slot = L % 8, L // 8
        return xcd * (ny // 8) + slot // nx, slot % nx
    return L // nx, L % nx


def head_map_rowmajor(B: int, H: int, L: int):
    nx = H // 256
    return L // nx, L % nx


def head_map_half(B: int, H: int, L: int):
    """A botched edit of one branch: the row block of the XCD map with the column block of the row-major one."""
    return head_map(B, H, L)[0], head_map_rowmajor(B, H, L)[1]


def head_inputs(B: int, H: int, nact: int, exact: bool, seed: int):
    """A [B, H] and W [4, H] as bf16-exact fp32.  A holds negatives, -0.0 and +0.0 (all give G = 0).  Exact:
    A in -3..5, W in -4..4 (rows distinct), so g W (g = k/32, |k| <= 20) is exact in bf16 and every dW / gpart
    partial sum is exact in fp32."""
    g = np.random.default_rng(seed)
    if exact:
        A = g.integers(-3, 6, (B, H)).astype(F)
        W = g.integers(-4, 5, (4, H)).astype(F)
    else:
        A = bf16_val(bf16_bits(g.standard_normal((B, H)).astype(F))).astype(F)
        W = bf16_val(bf16_bits(0.1 * g.standard_normal((4, H)).astype(F))).astype(F)
    A[:, 3::17] = F(-0.0)
    A[:, 5::19] = F(0.0)
    W[nact:] = np.nan          # rows the kernel must not read
    return A, W


def head_ref(A, W, a, gv, nact, block_map=head_map, swap_pieces=False, drop_block=None):
    """G, dW increment, gpart from the stored dq values gv [B] (bf16-exact), block by block as the kernel
    walks them.  Returns G bits [B, H] (0xFFFF where no block wrote), dW [4, H] float64, sum|terms| [4, H],
    gpart [B/64, H] float64, sum|G| per block, and the list of (by, bx) visited.
    Mutations: block_map, swap_pieces (the first two 8-column pieces of every row of G trade places),
    drop_block (that row block's contribution to dW is lost)."""
    B, H = A.shape
    nx, ny = H // 256, B // 64
    Gb = np.full((B, H), 0xFFFF, np.uint16)
    dW = np.zeros((4, H))
    dWa = np.zeros((4, H))
    gp = np.full((ny, H), np.nan)
    gpa = np.zeros((ny, H))
    seen = []
    A64, g64 = A.astype(np.float64), np.asarray(gv, np.float64)
    for L in range(nx * ny):
        by, bx = block_map(B, H, L)
        seen.append((by, bx))
        r, cs = slice(64 * by, 64 * by + 64), slice(256 * bx, 256 * bx + 256)
        w = np.nan_to_num(W[:, cs])[a[r]]                                 # [64, 256] row m's W[a_m]
        prod = (F(1) * (g64[r, None] * w).astype(F) + F(0)).astype(F)     # exact product of two bf16; -0 + 0 = +0
        Gv = np.where(A[r, cs] > 0, bf16_val(bf16_bits(prod)), 0.0)
        bitsG = np.where(A[r, cs] > 0, bf16_bits(prod), np.uint16(0))
        if swap_pieces:
            bitsG = bitsG.copy()
            bitsG[:, 0:8], bitsG[:, 8:16] = bitsG[:, 8:16].copy(), bitsG[:, 0:8].copy()
        Gb[r, cs] = bitsG
        gp[by, cs] = Gv.sum(0)
        gpa[by, cs] = np.abs(Gv).sum(0)
        if drop_block is not None and by == drop_block:
            continue
        t = g64[r, None] * A64[r, cs]
        for k in range(nact):
            sel = (a[r] == k)[:, None]
            dW[k, cs] += (t * sel).sum(0)
            dWa[k, cs] += (np.abs(t) * sel).sum(0)
    return Gb, dW, dWa, gp, gpa, seen


def qparts(nqp: int, B: int, nact: int, exact: bool, seed: int):
    """Partial head sums [nqp][B][4] for q and qt and the two biases; entries of actions >= nact are NaN."""
    g = np.random.default_rng(seed)
    if exact:   # q parts in k/4, qt parts in k/2, few nonzero: the sums stay in td_inputs' exact ranges
        qp = (g.integers(-1, 2, (nqp, B, 4)) * (g.random((nqp, B, 4)) < 4.0 / (nqp + 3)) / 4.0).astype(F)
        qpt = (g.integers(-1, 2, (nqp, B, 4)) * (g.random((nqp, B, 4)) < 4.0 / (nqp + 3)) / 2.0).astype(F)
        bq, bqt = np.array([0.25, -0.5, 0.75, 1.0], F), np.array([0.5, -1.0, 1.5, 0.0], F)
    else:
        qp, qpt = (g.standard_normal((nqp, B, 4)).astype(F) for _ in range(2))
        bq, bqt = (g.standard_normal(4).astype(F) for _ in range(2))
    qp[:, :, nact:] = np.nan
    qpt[:, :, nact:] = np.nan
    bq[nact:] = np.nan
    bqt[nact:] = np.nan
    return qp, qpt, bq, bqt


def qparts_sum(qp, bias, nact):
    """numpy float32 sum of the parts in order 0..nqp-1, then plus the bias: [B, nact]."""
    v = np.zeros(qp.shape[1:], F)
    for part in range(qp.shape[0]):
        v = (v + qp[part]).astype(F)
    return (v[:, :nact] + bias[None, :nact]).astype(F)


# ----------------------------------------------------------------------------- qhead
QHEAD_R = [16, 48]
QHEAD_H = [8, 120, 128, 136, 1016, 1024]


def qhead_inputs(R, H, lda, ldw, nact, exact, seed):
    """A [R, lda], W [4, ldw] (bf16-exact fp32; padding and rows >= nact NaN), bias [4].  Exact: integers in
    -8..8 with distinct columns, every partial sum below 2^24."""
    g = np.random.default_rng(seed)
    A = np.full((R, lda), np.nan, F)
    W = np.full((4, ldw), np.nan, F)
    if exact:
        A[:, :H] = g.integers(-8, 9, (R, H))
        W[:nact, :H] = g.integers(-8, 9, (nact, H))
        bias = np.array([3.0, -5.0, 7.0, 11.0], F)
    else:
        A[:, :H] = bf16_val(bf16_bits(g.standard_normal((R, H)).astype(F)))
        W[:nact, :H] = bf16_val(bf16_bits(g.standard_normal((nact, H)).astype(F)))
        bias = g.standard_normal(4).astype(F)
    bias[nact:] = np.nan
    return A, W, bias


def qhead_ref(A, W, bias, H, nact, drop_last_unit=False):
    """Q [R, nact] float64 and its bound (H/2 + 8) u sum|a w| + u |bias|.  drop_last_unit: the mutation."""
    h = H - 8 if drop_last_unit else H
    a, w = A[:, :h].astype(np.float64), W[:nact, :h].astype(np.float64)
    b = bias[:nact].astype(np.float64)
    ref = a @ w.T + b[None, :]
    a, w = A[:, :H].astype(np.float64), W[:nact, :H].astype(np.float64)
    return ref, (H / 2 + 8) * U * (np.abs(a) @ np.abs(w).T) + U * np.abs(b)[None, :]


# ----------------------------------------------------------------------------- row sum, transpose
ROWSUM_N = [1, 255, 256, 257, 1000]
TRANSPOSE_SHAPES = [(8, 8), (64, 64), (72, 56), (136, 200)]


def rowsum_inputs(rows, n, exact, seed):
    g = np.random.default_rng(seed)
    if exact:   # distinct per column: a dropped or doubled column changes the sum
        return ((np.arange(n)[None, :] * 7 + np.arange(rows)[:, None] * 3) % 61 - 30).astype(F)
    return bf16_val(bf16_bits(g.standard_normal((rows, n)).astype(F))).astype(F)


# ----------------------------------------------------------------------------- Adam
LR, B1, B2, EPS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
ADAM_T = [1, 2, 10, 1000]
ADAM_TILE_SHAPES = [(1, 1), (31, 33), (32, 32), (65, 40)]
ADAM_W_SHAPES = [(8, 4), (64, 64), (72, 68), (136, 260)]
ADAM_GT = [(1, 8), (4, 512), (5, 520), (130, 1032)]      # (I, nb); ldg = nb + 8
ADAM_G = [1, 32, 33]
ADAM_GP = [1, 7, 8, 9, 64]                               # np; ldp = I + 4


def adam_state(n: int, seed: int, with_mask: bool = True) -> dict:
    """w, g, m, v (fp32) and a mask holding 0, 0.5 and 1.  m has the sign of g: beta1 m + (1 - beta1) g then
    does not cancel, so m's own roundings (4u of sum|terms|) are 4u of |m'| and fit the 16u of adam_ref's
    bound on w (counted there)."""
    g = np.random.default_rng(seed)
    mask = np.ones(n, F)
    if with_mask:
        mask[g.random(n) < 0.25] = 0.0
        mask[g.random(n) < 0.15] = 0.5
        mask[:3] = [0.5, 0.0, 1.0][:n]
    grad = g.standard_normal(n).astype(F)
    m = np.abs(0.1 * g.standard_normal(n)).astype(F)
    return {"w": (0.1 + 0.05 * g.standard_normal(n)).astype(F), "g": grad, "m": m_like(m, grad),
            "v": (0.01 + 0.1 * g.random(n)).astype(F), "mask": mask}


def m_like(m, g) -> np.ndarray:
    """|m| with the sign of g (+ where g is 0)."""
    return (np.abs(np.asarray(m, F)) * np.where(np.asarray(g, np.float64) < 0, F(-1), F(1))).astype(F)


def adam_ref(w, g, m, v, mask, t, lr=LR, b1=B1, b2=B2, eps=EPS, stale_m=False):
    """One Adam step in float64 from this launch's fp32 inputs.  Returns w', m', v' and their bounds:
    m, v within 4u of sum|terms|; w within u |w'| + lr (2u b2^t / (1 - b2^t) + 2u b1^t / (1 - b1^t) + 16u)
    |mhat| / (sqrt(vhat) + eps) (the fractions: the cancellation in 1 - powf(beta, t); the 16u: m' 3, 1 - pow,
    reciprocal, m c1: 3; v' 4, 1 - pow, reciprocal, v c2: 3, halved by the square root, which adds 1; + eps,
    division, lr: 3 -- 13.5 where m and g have one sign).  Masked elements (mask 0) keep w, m, v.  stale_m: the mutation 'm read after it was written'."""
    w, g, m, v, mask = (np.asarray(x, F).astype(np.float64) for x in (w, g, m, v, mask))
    live = mask != 0
    gk = g * mask
    m1 = b1 * m + (1 - b1) * gk
    if stale_m:
        m1 = b1 * m1 + (1 - b1) * gk
    v1 = b2 * v + (1 - b2) * gk * gk
    c1, c2 = 1 - b1 ** t, 1 - b2 ** t
    step = (m1 / c1) / (np.sqrt(v1 / c2) + eps)
    w1 = w - lr * step
    bm = 4 * U * (np.abs(b1 * m) + np.abs((1 - b1) * gk))
    bv = 4 * U * (np.abs(b2 * v) + (1 - b2) * gk * gk)
    bw = U * np.abs(w1) + lr * (2 * U * b2 ** t / c2 + 2 * U * b1 ** t / c1 + 16 * U) * np.abs(step)
    z = np.zeros_like(w)
    return (np.where(live, w1, w), np.where(live, m1, m), np.where(live, v1, v),
            np.where(live, bw, z), np.where(live, bm, z), np.where(live, bv, z))


def gt_inputs(I, nb, ldg, exact, seed):
    """Layer gradient transposed [I][ldg] as bf16-exact fp32, padding NaN."""
    g = np.random.default_rng(seed)
    x = np.full((I, ldg), np.nan, F)
    if exact:
        x[:, :nb] = ((np.arange(nb)[None, :] * 5 + np.arange(I)[:, None] * 11) % 31 - 15) / 8.0
    else:
        x[:, :nb] = bf16_val(bf16_bits(g.standard_normal((I, nb)).astype(F)))
    return x


def gp_inputs(npart, I, ldp, exact, seed):
    """fp32 partial column sums [np][ldp], padding NaN."""
    g = np.random.default_rng(seed)
    x = np.full((npart, ldp), np.nan, F)
    if exact:
        x[:, :I] = ((np.arange(I)[None, :] * 3 + np.arange(npart)[:, None] * 7) % 29 - 14) / 4.0
    else:
        x[:, :I] = g.standard_normal((npart, I)).astype(F)
    return x


def seg_blocks(kind: str, O: int, I: int) -> int:
    if kind == "w":
        return ((I + 63) // 64) * ((O + 63) // 64)
    return (I + 3) // 4 if kind == "gT" else (I + 31) // 32
