"""csrc/deep.hip against plain references, kernel by kernel, on hand-built tensors.

The `st_*` entry points are driven directly through the ctypes mirrors of sharetrade/trainer/deep.py; no
DeepDQN is involved except in the last section (wiring).  The references and the case lists live in
tests/deep_kernel_refs.py, and tests/test_deep_kernel_refs.py shows on the CPU that these comparisons notice
a mutated kernel.

Every buffer a kernel reads or writes sits in a guard band (tests/guard_band.py): NaN around what is read,
a sentinel around what is only written; after each launch the surroundings are bit-unchanged.  Poison in
index-like fields stays inside the valid range (a wrong read shows as a wrong value, never as an
out-of-range address); the give-away sits in the float fields.

Per arithmetic kernel an exact case (dyadic inputs: every product and partial sum exact, so the result is
independent of summation and atomic order: bit equality) and a random case (error against float64 within a
bound counted from the kernel's operations, u = 2^-24; an interval check where the kernel rounds to bf16).
Where a kernel adds to a value that was there before (loss, statistics, dW), the random case starts it at a
power of two at or below the sum of the added terms' magnitudes (taken from the reference), so that the
roundings of the additions onto it stay inside the stated bound.
"""
import numpy as np
import pytest
import torch

import deep_kernel_refs as R
from guard_band import Band, bits

pytestmark = pytest.mark.gpu

U, F = R.U, np.float32
NAN = float("nan")
INVALID = 1            # hipErrorInvalidValue
BF_SENT = -7776.0      # bf16 sentinel (exact in bf16)
F_SENT = 12345.5
I_SENT = 0x0BADF00D


# ----------------------------------------------------------------------------- plumbing
def _k():
    from sharetrade.trainer import deep

    return deep, deep._bind()


def _sh():
    from sharetrade.ops import native

    return native.stream_handle()


def _band(arr, guard, dtype=None) -> Band:
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return Band(t.numel(), dtype or t.dtype, guard).set(t)


def _out(n, dtype, sentinel) -> Band:
    return Band(n, dtype, sentinel).set(sentinel)


def _np(b: Band) -> np.ndarray:
    return b.cpu().numpy()


def _bfbits(b: Band) -> np.ndarray:
    return bits(b.cpu()).numpy().view(np.uint16)


def _fbits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_f32(got, want) -> bool:
    return bool(np.array_equal(_fbits(got), _fbits(want)))


def _start_below(s):
    """A power of two at or below s (1 where s is 0): the start value of an accumulated output."""
    s = np.asarray(s, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(s > 0, np.exp2(np.floor(np.log2(np.where(s > 0, s, 1.0)))), 1.0)


class Bufs(dict):
    def snap(self):
        return {k: v.snap() for k, v in self.items()}

    def check(self, before, written=()):
        """Everything outside ``written`` is bit-unchanged (guards included); the written ones' guards hold."""
        for k, v in self.items():
            if k in written:
                assert v.guards_intact(), f"{k}: write outside its region"
            else:
                assert v.same(before[k]), f"{k} changed"


def _launch(fn, *args) -> int:
    rc = fn(*args, _sh())
    torch.cuda.synchronize()
    return rc


def _ring_bufs(ring: dict, ctrl) -> Bufs:
    b = Bufs()
    for key in R.RING_KEYS:
        b["rp_" + key] = _band(ring[key], NAN if key in R.RING_F32 else 0)
    b["rp_ctrl"] = _band(np.array(ctrl, np.int64), 0)
    return b


def _ring_struct(deep, b: Bufs, cap: int):
    r = deep._Replay()
    for key in R.RING_KEYS:
        setattr(r, key, b["rp_" + key].ptr())
    r.ctrl, r.cap = b["rp_ctrl"].ptr(), cap
    return r


def _check_features(tag, got_bits, ref, dl, H, fm):
    """X against (ref, delta): feat_mode 0 bit-equal to rne_bf16 of the inputs, feat_mode 1 the interval check;
    columns >= H + 2 are +0 bits."""
    got_bits = got_bits.reshape(ref.shape)
    if fm == 0:
        want = R.bf16_bits(ref.astype(F)).reshape(ref.shape)
        bad = np.argwhere(got_bits != want)
        assert bad.size == 0, (tag, bad[:4].tolist())
        return 0
    ok = R.interval_ok(got_bits, ref, dl)
    assert ok.all(), (tag, np.argwhere(~ok)[:4].tolist())
    assert (got_bits[:, H + 2:] == 0).all(), tag
    return R.interval_off(got_bits, ref)


# ----------------------------------------------------------------------------- 1. gather, env mode
@pytest.mark.parametrize("fm", [0, 1])
@pytest.mark.parametrize("H,in_p", R.GATHER_SHAPES)
def test_gather_env(native_built, H, in_p, fm):
    deep, k = _k()
    off = tot = 0
    for B in R.GATHER_B:
        c = R.gather_env_case(H, B, seed=1000 * H + B)
        T = c["T"]
        b = Bufs(prices=_band(c["prices"], NAN), pos=_band(c["pos"], 0), budget=_band(c["budget"], NAN),
                 shares=_band(c["shares"], 0), X=_out(B * in_p, torch.bfloat16, BF_SENT),
                 Xn=_out(B * in_p, torch.bfloat16, BF_SENT), r=_out(B, torch.float32, F_SENT),
                 a=_out(B, torch.int32, I_SENT), d=_out(B, torch.float32, F_SENT))
        g = deep._Gather()
        g.prices, g.T, g.H, g.in_p, g.feat_mode, g.inv_b0 = b["prices"].ptr(), T, H, in_p, fm, R.INV_B0
        g.mode, g.B = 0, B
        g.pos, g.budget, g.shares = b["pos"].ptr(), b["budget"].ptr(), b["shares"].ptr()
        g.key0, g.key1 = R.KEY0, R.KEY1
        g.X, g.Xn, g.r_out, g.a_out, g.done_out = b["X"].ptr(), b["Xn"].ptr(), b["r"].ptr(), b["a"].ptr(), b["d"].ptr()
        before = b.snap()
        assert _launch(k.st_deep_gather, g) == 0
        b.check(before, written=("X",))
        ref, dl = R.gather_ref(c["prices"], T, H, in_p, fm, R.INV_B0, np.arange(B), c["pos"], c["budget"], c["shares"])
        off += _check_features((H, in_p, B), _bfbits(b["X"]), ref, dl, H, fm)
        tot += B * (H + 2)
    if fm:
        print(f"[meas] gather env H={H} in_p={in_p}: all inside the interval, {off} of {tot} entries off rne_bf16(ref)")


# ----------------------------------------------------------------------------- 2. gather, replay mode
_REPLAY_SHAPES = [(5, 8), (201, 204), (254, 256)]
_REPLAY_B = [(1, None), (5, None), (67, None), (16, 16), (16, 24), (48, 48), (48, 56)]   # (B, ldxt)
_CURSOR = {(7, 1): 3, (7, 5): 7, (64, 64): 96}   # rp.ctrl[0] != rp.ctrl[1]; as a modulus it still stays in the band


def _gather_replay_struct(deep, b, T, H, in_p, fm, B, cap, ldxt, z0, z1):
    g = deep._Gather()
    g.prices, g.T, g.H, g.in_p, g.feat_mode, g.inv_b0 = b["prices"].ptr(), T, H, in_p, fm, R.INV_B0
    g.mode, g.B = 1, B
    g.rp = _ring_struct(deep, b, cap)
    g.key0, g.key1, g.step = R.KEY0, R.KEY1, b["step"].ptr()
    g.X, g.Xn, g.r_out, g.a_out, g.done_out = b["X"].ptr(), b["Xn"].ptr(), b["r"].ptr(), b["a"].ptr(), b["d"].ptr()
    g.zero0, g.zero0_n = (b["z0"].ptr() if "z0" in b else None), z0
    g.zero1, g.zero1_n = (b["z1"].ptr() if "z1" in b else None), z1
    if ldxt is not None:
        g.XT, g.ldxt = b["XT"].ptr(), ldxt
    return g


def _replay_bufs(ring, ctrl, prices, step, B, in_p, ldxt, z0, z1, null0) -> Bufs:
    b = _ring_bufs(ring, ctrl)
    b["prices"] = _band(prices, NAN)
    b["step"] = _band(np.array([step], np.int64), 0)
    for key in ("X", "Xn"):
        b[key] = _out(B * in_p, torch.bfloat16, BF_SENT)
    b["r"], b["a"], b["d"] = _out(B, torch.float32, F_SENT), _out(B, torch.int32, I_SENT), _out(B, torch.float32, F_SENT)
    if ldxt is not None:
        b["XT"] = _out(in_p * ldxt, torch.bfloat16, BF_SENT)
    # the zeroed spans: n floats, then 5 more of the same buffer that must stay
    if not (z0 == 0 and null0):
        b["z0"] = _out(z0 + 5, torch.float32, F_SENT)
    if not (z1 == 0 and not null0):
        b["z1"] = _out(z1 + 5, torch.float32, F_SENT)
    return b


@pytest.mark.parametrize("step", R.SAMPLE_STEPS)
@pytest.mark.parametrize("cap,size", R.RINGS)
def test_gather_replay(native_built, cap, size, step):
    deep, k = _k()
    E, n, off, tot = 3, 0, 0, 0
    for H, in_p in _REPLAY_SHAPES:
        T = H + 4
        prices = R.price_bank(E, T, seed=H)
        ring = R.make_ring(cap, size, E, T, H, seed=100 * cap + size + H)
        for fm in (0, 1):
            for B, ldxt in _REPLAY_B:
                z0, z1 = R.ZERO_N[n % 6], R.ZERO_N[(n // 6 + n + 1) % 6]
                null0 = n % 2 == 0
                n += 1
                b = _replay_bufs(ring, [_CURSOR[(cap, size)], size], prices, step, B, in_p, ldxt, z0, z1, null0)
                g = _gather_replay_struct(deep, b, T, H, in_p, fm, B, cap, ldxt, z0, z1)
                before = b.snap()
                tag = (H, in_p, fm, B, ldxt, z0, z1)
                assert _launch(k.st_deep_gather, g) == 0, tag
                b.check(before, written=("X", "Xn", "r", "a", "d", "XT", "z0", "z1"))
                ref = R.replay_sample_ref(ring, prices, T, H, in_p, fm, R.INV_B0, B, step, size)
                assert (ref["idx"] < size).all()
                assert np.array_equal(_np(b["a"]), ref["a"]), tag
                assert _same_f32(_np(b["r"]), ref["r"]), tag
                assert _same_f32(_np(b["d"]), ref["done"]), tag
                xb = _bfbits(b["X"])
                off += _check_features(tag, xb, *ref["X"], H, fm) + _check_features(tag, _bfbits(b["Xn"]), *ref["Xn"], H, fm)
                tot += 2 * fm * B * (H + 2)
                if ldxt is not None:
                    xt = _bfbits(b["XT"]).reshape(in_p, ldxt)
                    assert np.array_equal(xt[:, :B], xb.reshape(B, in_p).T), tag
                    assert (R.bf16_val(xt[:, B:]) == BF_SENT).all(), tag      # columns B..ldxt are untouched
                for key, zn in (("z0", z0), ("z1", z1)):
                    if key in b:
                        z = _np(b[key])
                        assert (_fbits(z[:zn]) == 0).all() and (z[zn:] == F(F_SENT)).all(), (tag, key)
    print(f"[meas] gather replay cap={cap} size={size} step={step}: all inside the interval, {off} of {tot} entries off rne_bf16(ref)")


def test_gather_rejections(native_built):
    deep, k = _k()
    H, in_p, B, cap, size = 5, 8, 16, 7, 5
    T, E = H + 4, 3
    prices = R.price_bank(E, T, seed=1)
    ring = R.make_ring(cap, size, E, T, H, seed=2)

    def rejected(mode=1, in_p=in_p, H=H, B=B, ldxt=None, xt=False, z0_off=0, alloc_p=256):
        b = _replay_bufs(ring, [7, size], prices, 0, 64, alloc_p, 64 if xt else None, 8, 0, True)
        b["pos"], b["budget"], b["shares"] = (_band(np.zeros(64, np.int32), 0), _band(np.full(64, 5.0, F), NAN),
                                              _band(np.zeros(64, np.int32), 0))
        g = _gather_replay_struct(deep, b, T, H, in_p, 1, B, cap, ldxt if xt else None, 8, 0)
        g.mode = mode
        g.pos, g.budget, g.shares = b["pos"].ptr(), b["budget"].ptr(), b["shares"].ptr()
        g.zero0 = b["z0"].ptr() + z0_off
        before = b.snap()
        rc = _launch(k.st_deep_gather, g)
        if rc != 0:
            b.check(before)
        return rc == INVALID

    assert rejected(in_p=260, alloc_p=260), "in_p > 256"
    assert rejected(in_p=10), "in_p % 4"
    assert rejected(in_p=4), "H + 2 > in_p"
    assert rejected(mode=0, xt=True, ldxt=16), "XT in env mode"
    assert rejected(B=8, xt=True, ldxt=16), "XT with B % 16"
    assert rejected(B=32, xt=True, ldxt=16), "ldxt < B"
    assert rejected(B=16, xt=True, ldxt=20), "ldxt % 8"
    assert rejected(z0_off=4), "zero0 not 16-byte aligned"
    assert not rejected(xt=True, ldxt=16)      # the same buffers with valid arguments run


# ----------------------------------------------------------------------------- 3. env step
_ENV_STATE_KEYS = ("budget", "shares", "value", "pos", "episodes", "last_final")


@pytest.mark.parametrize("E", R.ENV_E)
def test_env_step(native_built, E):
    deep, k = _k()
    worst = 0.0
    for case in range(6):
        c = R.env_case(E, case)
        st = R.env_state(E, seed=10 * E + case)
        q = R.env_q(E, c["ldq"], seed=E + case)
        ring = R.env_ring0(c["cap"])
        cursor, step = c["cursor"], c["step0"]
        b = _ring_bufs(ring, [cursor, min(cursor, c["cap"])])
        b["prices"], b["q"] = _band(st["prices"], NAN), _band(q, NAN)
        for key in _ENV_STATE_KEYS:
            b[key] = _band(st[key], NAN if st[key].dtype == F else 0)
        b["ctrl"] = _band(np.array([step, 0], np.int64), 0x5A5A5A5A)
        b["stats"] = _band(np.zeros(4, F), NAN)
        p = deep._Env()
        p.prices, p.T, p.H, p.E = b["prices"].ptr(), c["T"], c["H"], E
        p.compat_env, p.s0, p.n_actions = c["compat"], c["s0"], c["n_actions"]
        p.b0, p.eps, p.inv_ramp = c["b0"], c["eps"], c["inv_ramp"]
        p.budget, p.shares, p.value, p.pos = b["budget"].ptr(), b["shares"].ptr(), b["value"].ptr(), b["pos"].ptr()
        p.episodes, p.last_final = b["episodes"].ptr(), b["last_final"].ptr()
        p.q, p.ldq, p.key0, p.key1 = b["q"].ptr(), c["ldq"], R.KEY0, R.KEY1
        p.ctrl, p.rp, p.stats = b["ctrl"].ptr(), _ring_struct(deep, b, c["cap"]), b["stats"].ptr()
        patterns, draws = [], []
        for launch in range(3):
            tag = (E, case, launch)
            new, ring2, info = R.env_mirror(c, st, ring, q, cursor, step)
            rew64, fin64 = info["rew"].astype(np.float64), info["fin"].astype(np.float64)[info["done"]]
            s0 = np.array([float(_start_below(np.abs(rew64).sum())), 5.0, 7.0, -float(_start_below(np.abs(fin64).sum()))])
            b["stats"].set(torch.from_numpy(s0.astype(F)))
            before = b.snap()
            assert _launch(k.st_deep_env_step, p) == 0
            b.check(before, written=_ENV_STATE_KEYS + ("ctrl", "stats", "rp_ctrl") + tuple("rp_" + x for x in R.RING_KEYS))
            for key in _ENV_STATE_KEYS:
                got = _np(b[key])
                assert (_same_f32(got, new[key]) if new[key].dtype == F else np.array_equal(got, new[key])), (tag, key)
            for key in R.RING_KEYS:       # written slots hold the record, every other slot is untouched
                got = _np(b["rp_" + key])
                assert (_same_f32(got, ring2[key]) if key in R.RING_F32 else np.array_equal(got, ring2[key])), (tag, key)
            assert _np(b["rp_ctrl"]).tolist() == [cursor + E, min(cursor + E, c["cap"])], tag
            assert _np(b["ctrl"]).tolist() == [step + 1, 0], tag
            stats = _np(b["stats"]).astype(np.float64)
            assert stats[1] == 5.0 + info["explore"].sum() and stats[2] == 7.0 + info["done"].sum(), (tag, stats)
            for i, terms in ((0, rew64), (3, fin64)):
                bound = (E + 4) * U * np.abs(terms).sum()
                err = abs(stats[i] - (s0[i] + terms.sum()))
                worst = max(worst, R.ratio(err, bound))
                assert err <= bound, (tag, i, err, bound)
            patterns.append(info["a"].tobytes())
            draws.append(info["u1"].tobytes() + info["u2"].tobytes())
            st, ring, cursor, step = new, ring2, cursor + E, step + 1
        # the step counter matters: three launches, three different draws (and, with enough envs that explore,
        # three different action patterns)
        assert len(set(draws)) == 3
        if E >= 63 and c["eps"] < 1.0:
            assert len(set(patterns)) == 3, (E, case)
    print(f"[meas] env_step E={E}: stats[0], stats[3] max err/bound = {worst:.4f}")


# ----------------------------------------------------------------------------- 4. TD
def _td_bufs(inp, B, ldq, loss0, t0) -> Bufs:
    b = Bufs(q=_band(inp["q"], NAN), qt=_band(inp["qt"], NAN), r=_band(inp["r"], NAN), a=_band(inp["a"], 0),
             done=_band(inp["done"], NAN), dq=_out(B * ldq, torch.bfloat16, BF_SENT),
             dqT=_out(ldq * B, torch.bfloat16, BF_SENT), loss=_band(np.array([loss0], F), NAN))
    if t0 is not None:
        b["t"] = _band(np.array([t0], np.int64), 0x5A5A5A5A)
    return b


def _td_fill(td, b, B, ldq, nact, gamma, coef):
    td.q, td.qt, td.r, td.a, td.done = b["q"].ptr(), b["qt"].ptr(), b["r"].ptr(), b["a"].ptr(), b["done"].ptr()
    td.dq, td.dqT, td.loss = b["dq"].ptr(), b["dqT"].ptr(), b["loss"].ptr()
    td.B, td.ldq, td.n_actions, td.gamma, td.coef = B, ldq, nact, gamma, coef
    td.t = b["t"].ptr() if "t" in b else None


def _td_params(inp, nact, exact):
    """gamma, coef and the start of the loss (exact: dyadic; random: a power of two at or below sum diff^2)."""
    if exact:
        return R.GAMMA_X, R.COEF_X, 3.5
    _, _, diff = R.td_ref(inp["q"], inp["qt"], inp["r"], inp["a"], inp["done"], nact, R.GAMMA_R, R.COEF_R)
    return R.GAMMA_R, R.COEF_R, float(_start_below((diff * diff).sum()))


def _check_td(tag, b, inp, B, ldq, nact, gamma, coef, loss0, t0, exact) -> float:
    """dq, dqT, loss, t of one TD launch against td_ref; returns the loss's err/bound."""
    dqv, dl, diff = R.td_ref(inp["q"], inp["qt"], inp["r"], inp["a"], inp["done"], nact, gamma, coef)
    dq, dqT = _bfbits(b["dq"]).reshape(B, ldq), _bfbits(b["dqT"]).reshape(ldq, B)
    sent = R.bf16_bits(np.array([BF_SENT], F))[0]
    rows = np.arange(B)
    taken = dq[rows, inp["a"]]
    assert R.interval_ok(taken, dqv, dl).all(), tag
    other = dq[:, :nact].copy()
    other[rows, inp["a"]] = 0
    assert (other == 0).all(), tag                       # +0 beside the taken action
    assert (dq[:, nact:] == sent).all() and (dqT[nact:] == sent).all(), tag
    assert np.array_equal(dqT[:nact], dq[:, :nact].T), tag
    want = loss0 + (diff * diff).sum()
    got = float(_np(b["loss"])[0])
    if exact:
        assert np.array_equal(taken, R.bf16_bits(dqv.astype(F))), tag
        assert got == want, (tag, got, want)
        rt = 0.0
    else:
        bound = (B + 4) * U * (diff * diff).sum()
        rt = R.ratio(abs(got - want), bound)
        assert abs(got - want) <= bound, (tag, got, want, bound)
    if t0 is not None:
        assert int(_np(b["t"])[0]) == t0 + 1, tag
    return rt


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("ldq,nact", R.TD_LD)
@pytest.mark.parametrize("B", R.TD_B)
def test_td(native_built, B, ldq, nact, exact):
    deep, k = _k()
    inp = R.td_inputs(B, ldq, nact, exact, seed=1000 * B + 10 * ldq + nact)
    gamma, coef, loss0 = _td_params(inp, nact, exact)
    worst = 0.0
    for t0 in (41, None):
        b = _td_bufs(inp, B, ldq, loss0, t0)
        td = deep._TD()
        _td_fill(td, b, B, ldq, nact, gamma, coef)
        before = b.snap()
        assert _launch(k.st_deep_td, td) == 0
        b.check(before, written=("dq", "dqT", "loss", "t"))
        worst = max(worst, _check_td((B, ldq, nact, t0), b, inp, B, ldq, nact, gamma, coef, loss0, t0, exact))
    if not exact:
        print(f"[meas] td B={B} ldq={ldq} nact={nact}: loss max err/bound = {worst:.4f}")


# ----------------------------------------------------------------------------- 5. head
def _head_case(deep, k, B, H, nact, exact, ldgp, nqp, seed):
    """One st_deep_head launch, checked against the references; returns (dW, gpart) err/bound."""
    ldq = 64 if nact == 3 else 4
    tag = (B, H, nact, exact, ldgp, nqp)
    inp = R.td_inputs(B, ldq, nact, exact, seed)
    A, W = R.head_inputs(B, H, nact, exact, seed + 1)
    qf = nqp is not None
    if qf:
        qp, qpt, bq, bqt = R.qparts(nqp, B, nact, exact, seed + 2)
        eff = dict(inp)
        eff["q"], eff["qt"] = np.full((B, ldq), F_SENT, F), np.full((B, ldq), F_SENT, F)
        eff["q"][:, :nact], eff["qt"][:, :nact] = R.qparts_sum(qp, bq, nact), R.qparts_sum(qpt, bqt, nact)
        inp = dict(inp, q=np.full((B, ldq), F_SENT, F), qt=np.full((B, ldq), F_SENT, F))
    else:
        eff = inp
    gamma, coef, loss0 = _td_params(eff, nact, exact)
    b = _td_bufs(inp, B, ldq, loss0, 41)
    b["A"], b["W"] = _band(A, NAN, torch.bfloat16), _band(W, NAN, torch.bfloat16)
    b["G"], b["GT"] = _out(B * H, torch.bfloat16, BF_SENT), _out(H * B, torch.bfloat16, BF_SENT)
    # the dW the launch adds to: known only after g is; a first guess here, replaced below for the random case
    dqv, _, _ = R.td_ref(eff["q"], eff["qt"], eff["r"], eff["a"], eff["done"], nact, gamma, coef)
    g_guess = R.bf16_round64(dqv)
    _, _, dWa, _, _, _ = R.head_ref(A, W, eff["a"], g_guess, nact)
    n_i, a_i = np.arange(H)[None, :], np.arange(4)[:, None]
    if exact:
        dW0 = (((n_i + 3 * a_i) % 9 - 4) / 32.0).astype(F)
    else:
        dW0 = (np.where((n_i + a_i) % 2 == 0, 0.5, -0.25) * _start_below(dWa)).astype(F)
    b["dW"] = _band(dW0, NAN)
    if ldgp is not None:
        b["gpart"] = _out((B // 64) * ldgp, torch.float32, F_SENT)
    if qf:
        b["qp"], b["qpt"], b["bq"], b["bqt"] = _band(qp, NAN), _band(qpt, NAN), _band(bq, NAN), _band(bqt, NAN)
    hd = deep._Head()
    _td_fill(hd.td, b, B, ldq, nact, gamma, coef)
    hd.A, hd.W, hd.G, hd.GT, hd.dW, hd.H = b["A"].ptr(), b["W"].ptr(), b["G"].ptr(), b["GT"].ptr(), b["dW"].ptr(), H
    if ldgp is not None:
        hd.gpart, hd.ldgp = b["gpart"].ptr(), ldgp
    if qf:
        hd.qp, hd.qpt, hd.nqp, hd.bq, hd.bqt = b["qp"].ptr(), b["qpt"].ptr(), nqp, b["bq"].ptr(), b["bqt"].ptr()
    before = b.snap()
    assert _launch(k.st_deep_head, hd) == 0, tag
    b.check(before, written=("dq", "dqT", "loss", "t", "G", "GT", "dW", "gpart") + (("q", "qt") if qf else ()))
    if qf:   # Q values: fixed-order fp32 sums, bit for bit; the padding columns stay
        assert _same_f32(_np(b["q"]).reshape(B, ldq), eff["q"]), tag
        assert _same_f32(_np(b["qt"]).reshape(B, ldq), eff["qt"]), tag
    _check_td(tag, b, eff, B, ldq, nact, gamma, coef, loss0, 41, exact)
    if not qf:   # the same TD outputs as st_deep_td, bit for bit
        b2 = _td_bufs(inp, B, ldq, loss0, 41)
        td = deep._TD()
        _td_fill(td, b2, B, ldq, nact, gamma, coef)
        assert _launch(k.st_deep_td, td) == 0
        # the loss: both kernels add one wave sum per 64 rows with an atomic; with more than one row block the
        # order of the atomics is free, so the random case is bit-equal only at B = 64 (both within the bound)
        for key in ("dq", "dqT", "t") + (("loss",) if exact or B == 64 else ()):
            assert torch.equal(b[key].snap(), b2[key].snap()), (tag, key)
        _check_td(tag, b2, inp, B, ldq, nact, gamma, coef, loss0, 41, exact)
    # G, GT, dW, gpart from the dq the kernel stored
    dq = _bfbits(b["dq"]).reshape(B, ldq)
    gv = R.bf16_val(dq[np.arange(B), eff["a"]])
    Gb, dW, dWa, gp, gpa, seen = R.head_ref(A, W, eff["a"], gv, nact)
    assert sorted(seen) == [(y, x) for y in range(B // 64) for x in range(H // 256)]
    G = _bfbits(b["G"]).reshape(B, H)
    bad = np.argwhere(G != Gb)
    assert bad.size == 0, (tag, bad[:4].tolist())
    assert np.array_equal(_bfbits(b["GT"]).reshape(H, B), G.T), tag
    got = _np(b["dW"]).reshape(4, H)
    assert _same_f32(got[nact:], dW0[nact:]), tag
    want = dW0[:nact].astype(np.float64) + dW[:nact]
    rw = rg = 0.0
    if exact:
        assert _same_f32(got[:nact], want.astype(F)), tag
        assert (want.astype(F).astype(np.float64) == want).all()
    else:
        bound = (B + 8) * U * dWa[:nact]
        err = np.abs(got[:nact].astype(np.float64) - want)
        rw = R.ratio(err, bound)
        assert (err <= bound).all(), (tag, rw)
    if ldgp is not None:
        gpg = _np(b["gpart"]).reshape(B // 64, ldgp)
        assert (gpg[:, H:] == F(F_SENT)).all(), tag
        if exact:
            assert _same_f32(gpg[:, :H], gp.astype(F)), tag
        else:
            err = np.abs(gpg[:, :H].astype(np.float64) - gp)
            rg = R.ratio(err, 72 * U * gpa)
            assert (err <= 72 * U * gpa).all(), (tag, rg)
    return rw, rg


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("B,H", R.HEAD_SHAPES)
def test_head(native_built, B, H, exact):
    deep, k = _k()
    rw = rg = 0.0
    n = 0
    for nact in (1, 3, 4):
        for ldgp in (None, H, H + 64):
            for nqp in [None] + R.HEAD_NQP:
                n += 1
                w, g = _head_case(deep, k, B, H, nact, exact, ldgp, nqp, seed=100 * B + H + n)
                rw, rg = max(rw, w), max(rg, g)
    if not exact:
        print(f"[meas] head B={B} H={H}: dW max err/bound = {rw:.4f}, gpart max err/bound = {rg:.4f}")


def test_head_rejections(native_built):
    deep, k = _k()
    B, H, ldq, nact = 64, 256, 4, 3
    inp = R.td_inputs(B, ldq, nact, True, 5)
    A, W = R.head_inputs(B, H, nact, True, 6)
    qp, qpt, bq, bqt = R.qparts(1, B, nact, True, 7)

    def rejected(B=B, H=H, nact=nact, ldq=ldq, ldgp=None, qf=(), nqp=1):
        b = _td_bufs(inp, 64, 4, 3.5, 41)
        b["A"], b["W"] = _band(A, NAN, torch.bfloat16), _band(W, NAN, torch.bfloat16)
        b["G"], b["GT"] = _out(64 * 256, torch.bfloat16, BF_SENT), _out(64 * 256, torch.bfloat16, BF_SENT)
        b["dW"], b["gpart"] = _band(np.ones((4, 256), F), NAN), _out(256, torch.float32, F_SENT)
        b["qp"], b["qpt"], b["bq"], b["bqt"] = _band(qp, NAN), _band(qpt, NAN), _band(bq, NAN), _band(bqt, NAN)
        hd = deep._Head()
        _td_fill(hd.td, b, B, ldq, nact, 0.5, 0.125)
        hd.A, hd.W, hd.G, hd.GT, hd.dW, hd.H = b["A"].ptr(), b["W"].ptr(), b["G"].ptr(), b["GT"].ptr(), b["dW"].ptr(), H
        if ldgp is not None:
            hd.gpart, hd.ldgp = b["gpart"].ptr(), ldgp
        for key in qf:
            setattr(hd, key, b[key].ptr())
        hd.nqp = nqp
        before = b.snap()
        rc = _launch(k.st_deep_head, hd)
        if rc != 0:
            b.check(before)
        return rc == INVALID

    assert rejected(B=32), "B % 64"
    assert rejected(H=128), "H % 256"
    assert rejected(nact=0) and rejected(nact=5), "n_actions"
    assert rejected(nact=3, ldq=2), "n_actions > ldq"
    assert rejected(ldgp=192), "ldgp < H"
    assert rejected(qf=("qp", "bq", "bqt")), "qp without qpt"
    assert rejected(qf=("qp", "qpt", "bqt")), "qp without bq"
    assert rejected(qf=("qp", "qpt", "bq", "bqt"), nqp=0), "nqp 0"
    assert not rejected(ldgp=256, qf=("qp", "qpt", "bq", "bqt"))


# ----------------------------------------------------------------------------- 6. qhead
def _qhead_launch(deep, k, b, R_, H, lda, ldw, ldq, nact, null=None):
    p = deep._QHead()
    p.A, p.W, p.bias, p.Q = (None if null == key else b[key].ptr() for key in ("A", "W", "bias", "Q"))
    p.R, p.H, p.lda, p.ldw, p.ldq, p.nact = R_, H, lda, ldw, ldq, nact
    return _launch(k.st_qhead, p)


@pytest.mark.parametrize("H", R.QHEAD_H)
@pytest.mark.parametrize("rows", R.QHEAD_R)
def test_qhead(native_built, rows, H):
    deep, k = _k()
    worst, n = 0.0, 0
    for lda in (H, H + 8):
        for ldw in (H, H + 8):
            for nact in (1, 3, 4):
                for ldq in (nact, 64):
                    for exact in (True, False):
                        n += 1
                        tag = (rows, H, lda, ldw, nact, ldq, exact)
                        A, W, bias = R.qhead_inputs(rows, H, lda, ldw, nact, exact, seed=H + n)
                        b = Bufs(A=_band(A, NAN, torch.bfloat16), W=_band(W, NAN, torch.bfloat16), bias=_band(bias, NAN),
                                 Q=_out(rows * ldq, torch.float32, F_SENT))
                        before = b.snap()
                        assert _qhead_launch(deep, k, b, rows, H, lda, ldw, ldq, nact) == 0, tag
                        b.check(before, written=("Q",))
                        Q = _np(b["Q"]).reshape(rows, ldq)
                        assert (Q[:, nact:] == F(F_SENT)).all(), tag
                        ref, bound = R.qhead_ref(A, W, bias, H, nact)
                        if exact:
                            assert _same_f32(Q[:, :nact], ref.astype(F)), tag
                        else:
                            err = np.abs(Q[:, :nact].astype(np.float64) - ref)
                            worst = max(worst, R.ratio(err, bound))
                            assert (err <= bound).all(), (tag, R.ratio(err, bound))
    print(f"[meas] qhead R={rows} H={H}: max err/bound = {worst:.4f}")


def test_qhead_rejections(native_built):
    deep, k = _k()
    A, W, bias = R.qhead_inputs(16, 1032, 1040, 1040, 4, True, 3)
    b = Bufs(A=_band(A, NAN, torch.bfloat16), W=_band(W, NAN, torch.bfloat16), bias=_band(bias, NAN),
             Q=_out(16 * 64, torch.float32, F_SENT))
    ok = dict(R_=16, H=128, lda=136, ldw=136, ldq=4, nact=3)
    bad = [dict(R_=8), dict(R_=0), dict(H=12), dict(H=1032, lda=1040, ldw=1040), dict(nact=0), dict(nact=5, ldq=8),
           dict(lda=120), dict(ldw=120), dict(ldq=2), dict(null="A"), dict(null="W"), dict(null="bias"), dict(null="Q")]
    for kw in bad:
        before = b.snap()
        assert _qhead_launch(deep, k, b, **dict(ok, **kw)) == INVALID, kw
        b.check(before)
    assert _qhead_launch(deep, k, b, **ok) == 0


# ----------------------------------------------------------------------------- 7. row sum, transpose
@pytest.mark.parametrize("n", R.ROWSUM_N)
@pytest.mark.parametrize("rows", [1, 3])
def test_row_sum(native_built, rows, n):
    deep, k = _k()
    ld = n + 3
    for exact in (True, False):
        x = np.full((rows, ld), np.nan, F)
        x[:, :n] = R.rowsum_inputs(rows, n, exact, seed=n + rows)
        b = Bufs(X=_band(x, NAN, torch.bfloat16), out=_out(rows, torch.float32, F_SENT))
        before = b.snap()
        assert _launch(k.st_row_sum_bf16, b["X"].ptr(), ld, rows, n, b["out"].ptr()) == 0
        b.check(before, written=("out",))
        got = _np(b["out"])
        x64 = x[:, :n].astype(np.float64)
        if exact:
            assert _same_f32(got, x64.sum(1).astype(F)), (rows, n)
        else:
            err, bound = np.abs(got.astype(np.float64) - x64.sum(1)), (n / 256 + 12) * U * np.abs(x64).sum(1)
            print(f"[meas] row_sum rows={rows} n={n}: max err/bound = {R.ratio(err, bound):.4f}")
            assert (err <= bound).all()


@pytest.mark.parametrize("rows,cols", R.TRANSPOSE_SHAPES)
def test_transpose(native_built, rows, cols):
    deep, k = _k()
    ldi, ldo = cols + 8, rows + 16
    g = np.random.default_rng(rows * cols)
    x = R.bf16_val(R.bf16_bits(g.standard_normal((rows, ldi)).astype(F))).astype(F)
    x[:, cols:] = np.nan
    b = Bufs(X=_band(x, NAN, torch.bfloat16), out=_out(cols * ldo, torch.bfloat16, BF_SENT))
    before = b.snap()
    assert _launch(k.st_transpose_bf16, b["X"].ptr(), ldi, b["out"].ptr(), ldo, rows, cols) == 0
    b.check(before, written=("out",))
    out = _bfbits(b["out"]).reshape(cols, ldo)
    assert np.array_equal(out[:, :rows], R.bf16_bits(x[:, :cols]).reshape(rows, cols).T)
    assert (R.bf16_val(out[:, rows:]) == BF_SENT).all()
    for kw in (dict(rows=rows + 4), dict(cols=cols + 4), dict(ldi=ldi + 4), dict(ldo=ldo + 4)):
        a = dict(dict(rows=rows, cols=cols, ldi=ldi, ldo=ldo), **kw)
        before = b.snap()
        assert _launch(k.st_transpose_bf16, b["X"].ptr(), a["ldi"], b["out"].ptr(), a["ldo"], a["rows"], a["cols"]) == INVALID
        b.check(before)


# ----------------------------------------------------------------------------- 8. Adam
def _adam_bufs(st, O, I, wb=True, wbT=True, mask=True) -> Bufs:
    b = Bufs(w=_band(st["w"], NAN), g=_band(st["g"], NAN), m=_band(st["m"], NAN), v=_band(st["v"], NAN))
    if mask:
        b["mask"] = _band(st["mask"], NAN)
    if wb:
        b["wb"] = _out(O * I, torch.bfloat16, BF_SENT)
    if wbT:
        b["wbT"] = _out(O * I, torch.bfloat16, BF_SENT)
    return b


def _check_adam(tag, b, before_st, O, I, t, grads_only=False):
    """w, m, v, wb, wbT after one launch against adam_ref of this launch's own fp32 inputs (before_st: numpy
    w, g, m, v, mask as the update read them).  Returns the largest err/bound of (w, m, v)."""
    w, m, v = _np(b["w"]), _np(b["m"]), _np(b["v"])
    if grads_only:
        for key, got in (("w", w), ("m", m), ("v", v)):
            assert _same_f32(got, before_st[key]), (tag, key)
        return 0.0
    w1, m1, v1, bw, bm, bv = R.adam_ref(before_st["w"], before_st["g"], before_st["m"], before_st["v"], before_st["mask"], t)
    keep = before_st["mask"] == 0
    worst = 0.0
    for key, got, ref, bound in (("w", w, w1, bw), ("m", m, m1, bm), ("v", v, v1, bv)):
        assert np.array_equal(_fbits(got)[keep], _fbits(before_st[key])[keep]), (tag, key, "masked element moved")
        err = np.abs(got.astype(np.float64) - ref)
        rt = R.ratio(err, bound)
        worst = max(worst, rt)
        assert (err <= bound).all(), (tag, key, rt)
    if (~keep).any():
        assert not np.array_equal(_fbits(w)[~keep], _fbits(before_st["w"])[~keep]), tag
    if "wb" in b:
        wb = _bfbits(b["wb"])
        assert np.array_equal(wb, R.bf16_bits(w)), (tag, "wb")
        if "wbT" in b:
            assert np.array_equal(_bfbits(b["wbT"]).reshape(I, O), wb.reshape(O, I).T), (tag, "wbT")
    return worst


def _st_of(b: Bufs, n: int) -> dict:
    st = {key: _np(b[key]) for key in ("w", "g", "m", "v")}
    st["mask"] = _np(b["mask"]) if "mask" in b else np.ones(n, F)
    return st


def _adam_tile(deep, k, b, tband, O, I):
    p = deep._Adam()
    p.w, p.g, p.m, p.v = b["w"].ptr(), b["g"].ptr(), b["m"].ptr(), b["v"].ptr()
    p.mask = b["mask"].ptr() if "mask" in b else None
    p.wb, p.wbT = b["wb"].ptr(), (b["wbT"].ptr() if "wbT" in b else None)
    p.t, p.O, p.I = tband.ptr(), O, I
    p.lr, p.beta1, p.beta2, p.eps = R.LR, R.B1, R.B2, R.EPS
    return _launch(k.st_adam_tile, p)


@pytest.mark.parametrize("O,I", R.ADAM_TILE_SHAPES)
def test_adam_tile(native_built, O, I):
    deep, k = _k()
    worst = 0.0
    for mask in (True, False):
        for wbT in (True, False):
            for t in R.ADAM_T:
                st = R.adam_state(O * I, seed=O * I + t)
                b = _adam_bufs(st, O, I, wbT=wbT, mask=mask)
                tb = _band(np.array([t], np.int64), 0)
                before, st0 = b.snap(), _st_of(b, O * I)
                assert _adam_tile(deep, k, b, tb, O, I) == 0
                b.check(before, written=("w", "m", "v", "wb", "wbT"))
                worst = max(worst, _check_adam((O, I, mask, wbT, t), b, st0, O, I, t))
    # a trajectory: four consecutive launches, each checked from its own inputs
    st = R.adam_state(O * I, seed=O + I)
    b = _adam_bufs(st, O, I)
    for t in (1, 2, 3, 4):
        tb = _band(np.array([t], np.int64), 0)
        st0 = _st_of(b, O * I)
        assert _adam_tile(deep, k, b, tb, O, I) == 0
        worst = max(worst, _check_adam((O, I, "trajectory", t), b, st0, O, I, t))
    print(f"[meas] adam_tile O={O} I={I}: max err/bound = {worst:.4f}")


class Seg:
    """One segment of an st_adam_multi launch and its expectations.  kind: 'w' (weights [O][I]), 'gT' (bias,
    gradient = row sums of gT [I][ldg] over nb), 'g' (bias, gradient given), 'gP' (bias, gradient = sum of np
    partial rows [np][ldp])."""

    def __init__(self, kind, O, I, seed, exact=False, nb=0, npart=0, mask=True, wb=True):
        self.kind, self.O, self.I, self.nb, self.npart, self.exact = kind, O, I, nb, npart, exact
        self.ldg, self.ldp = nb + 8, I + 4
        n = O * I
        st = R.adam_state(n, seed, with_mask=mask)
        if kind == "gT":
            self.src = R.gt_inputs(I, nb, self.ldg, exact, seed + 1)
            gsum = self.src[:, :nb].astype(np.float64).sum(1)
        if kind == "gP":
            self.src = R.gp_inputs(npart, I, self.ldp, exact, seed + 1)
            gsum = self.src[:, :I].astype(np.float64).sum(0)
        if kind in ("gT", "gP"):
            st["g"] = np.full(n, F_SENT, F)     # written by the launch
            st["m"] = R.m_like(st["m"], gsum)   # (the sign of the gradient the launch will reduce)
        self.b = _adam_bufs(st, O, I, wb=wb, wbT=(kind == "w"), mask=mask)
        if kind == "gT":
            self.b["gT"] = _band(self.src, NAN, torch.bfloat16)
        if kind == "gP":
            self.b["gP"] = _band(self.src, NAN)

    def fill(self, s, blocks=None):
        b = self.b
        s.w, s.g, s.m, s.v = b["w"].ptr(), b["g"].ptr(), b["m"].ptr(), b["v"].ptr()
        s.mask = b["mask"].ptr() if "mask" in b else None
        s.wb = b["wb"].ptr() if "wb" in b else None
        s.wbT = b["wbT"].ptr() if "wbT" in b else None
        s.gT = b["gT"].ptr() if "gT" in b else None
        s.gP = b["gP"].ptr() if "gP" in b else None
        s.O, s.I, s.ldg, s.nb, s.bias = self.O, self.I, self.ldg if self.kind == "gT" else 0, self.nb, int(self.kind != "w")
        s.np, s.ldp = self.npart, self.ldp if self.kind == "gP" else 0
        s.blocks = R.seg_blocks(self.kind, self.O, self.I) if blocks is None else blocks

    def written(self, grads_only):
        if grads_only:
            return ("g",)
        return ("w", "m", "v", "wb", "wbT") + (("g",) if self.kind in ("gT", "gP") else ())

    def check(self, tag, st0, t, grads_only=False):
        """Returns (Adam err/bound, bias-gradient err/bound)."""
        rg = 0.0
        if self.kind in ("gT", "gP"):
            got = _np(self.b["g"])
            if self.kind == "gT":
                x = self.src[:, :self.nb].astype(np.float64)
                ref, sa, cnt = x.sum(1), np.abs(x).sum(1), self.nb / 512 + 16
            else:
                x = self.src[:, :self.I].astype(np.float64)
                ref, sa, cnt = x.sum(0), np.abs(x).sum(0), self.npart / 8 + 8
            if self.exact:
                assert _same_f32(got, ref.astype(F)), (tag, "bias gradient")
                assert len(set(ref.tolist())) > 1 or self.I == 1, (tag, "degenerate pattern")
            else:
                err = np.abs(got.astype(np.float64) - ref)
                rg = R.ratio(err, cnt * U * sa)
                assert (err <= cnt * U * sa).all(), (tag, "bias gradient", rg)
            st0 = dict(st0, g=got)       # the update read the gradient it just reduced
        return _check_adam(tag, self.b, st0, self.O, self.I, t, grads_only), rg


def _adam_multi(deep, k, segs, t, grads_only=False, nseg=None, total=None, blocks=None):
    """One st_adam_multi launch over ``segs`` with full band checks; returns (rc, worst Adam, worst gradient)."""
    am = deep._AdamMulti()
    for i, sg in enumerate(segs):
        sg.fill(am.seg[i], blocks=blocks if i == 0 else None)
    tb = _band(np.array([t], np.int64), 0)
    am.nseg, am.t = (len(segs) if nseg is None else nseg), tb.ptr()
    am.total = sum(am.seg[i].blocks for i in range(len(segs))) if total is None else total
    am.lr, am.beta1, am.beta2, am.eps, am.grads_only = R.LR, R.B1, R.B2, R.EPS, int(grads_only)
    before = [sg.b.snap() for sg in segs]
    st0 = [_st_of(sg.b, sg.O * sg.I) for sg in segs]
    rc = _launch(k.st_adam_multi, am)
    ra = rg = 0.0
    for i, sg in enumerate(segs):
        sg.b.check(before[i], written=sg.written(grads_only) if rc == 0 else ())
        if rc == 0:
            a, g = sg.check((i, sg.kind, sg.O, sg.I, t), st0[i], t, grads_only)
            ra, rg = max(ra, a), max(rg, g)
    return rc, ra, rg


def _single_segments(exact):
    n = 0
    for O, I in R.ADAM_W_SHAPES:
        for mask in (True, False):
            n += 1
            yield Seg("w", O, I, seed=n, mask=mask)
    for I, nb in R.ADAM_GT:
        for wb in (True, False):
            n += 1
            yield Seg("gT", 1, I, seed=n, exact=exact, nb=nb, wb=wb, mask=wb)
    for I in R.ADAM_G:
        for wb in (True, False):
            n += 1
            yield Seg("g", 1, I, seed=n, wb=wb, mask=not wb)
    for i, npart in enumerate(R.ADAM_GP):
        n += 1
        yield Seg("gP", 1, (1, 33, 70, 32, 5)[i], seed=n, exact=exact, npart=npart, wb=bool(i % 2), mask=bool(i % 2))


@pytest.mark.parametrize("t", R.ADAM_T)
def test_adam_multi_single_segment(native_built, t):
    """Every segment shape as a launch of its own (nseg = 1), bias gradients random and exact."""
    deep, k = _k()
    ra = rg = 0.0
    for exact in (False, True):
        for sg in _single_segments(exact):
            rc, a, g = _adam_multi(deep, k, [sg], t)
            assert rc == 0, (sg.kind, sg.O, sg.I)
            ra, rg = max(ra, a), max(rg, g)
    print(f"[meas] adam_multi single segments t={t}: Adam max err/bound = {ra:.4f}, bias gradient max err/bound = {rg:.4f}")


def _mixed_segments():
    """16 segments whose kinds walk w g w T w P g T g P T P w w g g: every ordered pair of different kinds is
    a boundary once, and two same-kind boundaries."""
    w = iter([(8, 4), (64, 64), (72, 68), (136, 260), (8, 4), (72, 68)])
    g = iter([1, 32, 33, 1, 33])
    T = iter(R.ADAM_GT[:1] + R.ADAM_GT[2:])
    P = iter([(1, 5), (9, 33), (64, 40)])
    out = []
    for i, kind in enumerate("wgwTwPgTgPTPwwgg"):
        if kind == "w":
            O, I = next(w)
            out.append(Seg("w", O, I, seed=50 + i, mask=bool(i % 2)))
        elif kind == "g":
            out.append(Seg("g", 1, next(g), seed=50 + i, wb=bool(i % 2)))
        elif kind == "T":
            I, nb = next(T)
            out.append(Seg("gT", 1, I, seed=50 + i, nb=nb))
        else:
            npart, I = next(P)
            out.append(Seg("gP", 1, I, seed=50 + i, npart=npart, wb=False))
    return out


def test_adam_multi_mixed(native_built):
    deep, k = _k()
    segs = _mixed_segments()
    assert len(segs) == deep.ADAM_MAX_SEG
    ra = rg = 0.0
    for t in (1, 2, 3, 4, 1000):      # a trajectory, then a late step on the same state
        rc, a, g = _adam_multi(deep, k, segs, t)
        assert rc == 0
        ra, rg = max(ra, a), max(rg, g)
    print(f"[meas] adam_multi 16 segments: Adam max err/bound = {ra:.4f}, bias gradient max err/bound = {rg:.4f}")


def test_adam_multi_grads_only(native_built):
    deep, k = _k()
    segs = [Seg("gT", 1, 5, seed=1, nb=520), Seg("gP", 1, 33, seed=2, npart=9), Seg("gT", 1, 130, seed=3, nb=1032, exact=True),
            Seg("gP", 1, 70, seed=4, npart=64, exact=True)]
    rc, _, rg = _adam_multi(deep, k, segs, 3, grads_only=True)
    assert rc == 0
    print(f"[meas] adam_multi grads_only: bias gradient max err/bound = {rg:.4f}")


def test_adam_multi_rejections(native_built):
    deep, k = _k()

    def rc(segs, **kw):
        return _adam_multi(deep, k, segs, 2, **kw)[0]

    w = lambda O=64, I=64: Seg("w", O, I, seed=1)   # noqa: E731
    assert rc([w()], nseg=0) == INVALID and rc([w()], nseg=17) == INVALID, "nseg"
    assert rc([w()], blocks=2) == INVALID and rc([Seg("gT", 1, 5, seed=1, nb=8)], blocks=1) == INVALID, "blocks"
    assert rc([w(), w()], total=3) == INVALID, "total"
    assert rc([w(64, 66)]) == INVALID and rc([w(68, 64)]) == INVALID, "I % 4, O % 8"
    sg = Seg("gT", 1, 4, seed=1, nb=16)
    sg.nb = 12
    assert rc([sg]) == INVALID, "nb % 8"
    sg = Seg("gT", 1, 4, seed=1, nb=16)
    sg.ldg = 20
    assert rc([sg]) == INVALID, "ldg % 8"
    sg = Seg("gP", 1, 5, seed=1, npart=3)
    sg.npart = 0
    assert rc([sg]) == INVALID, "np < 1"
    sg = Seg("gP", 1, 5, seed=1, npart=3)
    sg.ldp = 4
    assert rc([sg]) == INVALID, "ldp < I"
    assert rc([w()], grads_only=True) == INVALID and rc([Seg("g", 1, 5, seed=1)], grads_only=True) == INVALID, "grads_only"
    assert rc([w(), Seg("gT", 1, 4, seed=1, nb=16)]) == 0


# ----------------------------------------------------------------------------- 9. wiring through DeepDQN
def test_deep_dqn_wiring(native_built):
    """The Python side fills the structs the way the mirrors assume: three act steps reproduce the env mirror
    (fed d.Qe, the previous state and the step counter) and one update's replay sample reproduces the gather
    mirror (fed the ring and the value t_ctr had before the call)."""
    from sharetrade.config import preset_config
    from sharetrade.data.prices import random_walk
    from sharetrade.env.trading import FEATURES
    from sharetrade.trainer.deep import DeepDQN
    from sharetrade.utils import rng

    cfg = preset_config("flagship")
    cfg.model.hidden = [128, 128]
    cfg.agent.epsilon, cfg.agent.ramp = 0.5, 2.0
    E = B = 128
    cap = 3 * E + 5
    prices = random_walk(400, 50.0, 0.02, 4, n_series=E).astype(F)
    d = DeepDQN(cfg, torch.device("cuda", 0), envs=E, batch=B, replay_capacity=cap, prices=torch.from_numpy(prices))
    key0, key1 = (int(x) for x in rng.key_for(d.seed, 0))
    c = {"E": E, "T": prices.shape[1], "H": cfg.model.history, "cap": cap, "compat": int(cfg.env.compat_decisions),
         "eps": R.f32(cfg.agent.epsilon), "inv_ramp": R.f32(1 / cfg.agent.ramp), "n_actions": cfg.model.n_actions,
         "b0": R.f32(cfg.env.budget), "s0": int(cfg.env.shares), "key0": key0, "key1": key1}

    def state():
        st = {key: getattr(d, key).cpu().numpy() for key in _ENV_STATE_KEYS}
        st["prices"] = prices
        return st

    def ring():
        return {key: d.rp[key].cpu().numpy() for key in R.RING_KEYS}

    for step in range(3):
        st, rg = state(), ring()
        d.act_step()
        torch.cuda.synchronize()
        new, ring2, _ = R.env_mirror(c, st, rg, d.Qe.cpu().numpy(), step * E, step)
        got, gring = state(), ring()
        for key in _ENV_STATE_KEYS:
            # last_final starts as NaN: compare bits
            assert (_same_f32(got[key], new[key]) if new[key].dtype == F else np.array_equal(got[key], new[key])), (step, key)
        for key in R.RING_KEYS:
            assert (_same_f32(gring[key], ring2[key]) if key in R.RING_F32 else np.array_equal(gring[key], ring2[key])), (step, key)
        assert d.rp_ctrl.tolist() == [(step + 1) * E, min((step + 1) * E, cap)] and d.env_ctrl.tolist() == [step + 1, 0]
    t0, rg = int(d.t_ctr), ring()
    size = int(d.rp_ctrl[1])
    d.update_step()
    torch.cuda.synchronize()
    assert int(d.t_ctr) == t0 + 1
    fm = FEATURES[cfg.env.features]
    ref = R.replay_sample_ref(rg, prices, c["T"], c["H"], d.in_p, fm, R.f32(1.0 / cfg.env.budget), B, t0, size,
                              key0=key0, key1=key1)
    assert np.array_equal(d.a_b.cpu().numpy(), ref["a"])
    assert _same_f32(d.r_b.cpu().numpy(), ref["r"]) and _same_f32(d.d_b.cpu().numpy(), ref["done"])
    for name, t in (("X", d.X), ("Xn", d.Xn)):
        _check_features(name, bits(t.cpu()).numpy().view(np.uint16), *ref[name], c["H"], fm)
