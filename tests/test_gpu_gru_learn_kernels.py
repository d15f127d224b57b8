"""csrc/gru_learn.hip against plain references, kernel by kernel, on hand-built tensors.

The `st_gru_*` entry points are driven directly through the ctypes mirrors of sharetrade/ops/gru.py; no
RecurrentDQN and no actor is involved.  The references, the case lists and the comparisons (``check_*``) live
in tests/gru_learn_refs.py, and tests/test_gru_learn_refs.py shows on the CPU that these comparisons notice a
mutated kernel.  Packed weights come from the project's own st_gru_pack on hand-built fp32 masters; the
references multiply with what unpack_whh / unpack_whhT read back from the packed fragments.

Every buffer a kernel reads sits in a NaN guard band (tests/guard_band.py), every buffer it only writes in a
sentinel band; after each launch everything outside the written regions is bit-unchanged.  No case can
produce an out-of-range address: ring fills stay at or below the ring's capacity and actions in 0..2.

No bound here was set from what the kernels return: each is counted from the kernel's operations
(u = 2^-24), or, for forward steps inside un-reset runs, four times the flip noise measured on the reference
(gru_learn_refs.fwd_chain_bound).  Figures: profiles/gru_learn_refs.md."""
import numpy as np
import pytest
import torch

import gru_learn_refs as R
from guard_band import bits
from test_gpu_deep_kernels import Bufs, _band, _bfbits, _fbits, _launch, _np, _out, _same_f32

pytestmark = pytest.mark.gpu

U, F = R.U, np.float32
NAN = float("nan")
INVALID = 1            # hipErrorInvalidValue
BF_SENT, F_SENT, I_SENT = -7776.0, 12345.5, 0x0BADF00D
BF_NAN = 0x7FC0        # int16 bands of bf16 data
FP8_NAN = 0x7F7F7F7F   # int32 bands of e4m3 bytes
RH, RG, RF, RFL = R.RH, R.RG, R.RF, R.RFL


def _k():
    from sharetrade.ops import gru as G

    return G, G.lib()


def _i16(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.uint16).view(np.int16)


# ----------------------------------------------------------------------------- packed weights
_PACKED = {}


def _packed(seed: int, heavy: bool = False) -> dict:
    """Masters of ``seed`` packed by st_gru_pack into guard bands, and the net the references multiply with
    (W_hh read back from the fragments).  Cached per module: packing has its own exactness test."""
    if (seed, heavy) in _PACKED:
        return _PACKED[(seed, heavy)]
    G, k = _k()
    m = R.masters(seed, heavy)
    nfr = G.RW * 3 * 2 * 2 * 64
    src = {n: torch.from_numpy(v).cuda() for n, v in m.items()}
    b = Bufs(whh8=_out(nfr * 8, torch.int32, FP8_NAN), whhs=_out(nfr, torch.int32, 0xFF),
             wih=_out(G.RW * 6 * 64 * 8, torch.int16, BF_NAN), bias4=_out(4 * RH, torch.float32, NAN),
             wq=_out(4 * RH, torch.float32, NAN), whhT8=_out(nfr * 8, torch.int32, FP8_NAN),
             whhTs=_out(nfr, torch.int32, 0xFF))
    p = G.PackArgs()
    p.w_hh, p.w_ih, p.b_ih, p.b_hh, p.w_q, p.b_q = (src[n].data_ptr() for n in ("w_hh", "w_ih", "b_ih", "b_hh", "w_q", "b_q"))
    for n in b:
        setattr(p, n, b[n].ptr())
    assert _launch(k.st_gru_pack, p) == 0
    for n in b:
        assert b[n].guards_intact(), n
    net = R.net_from(m, G.unpack_whh(b["whh8"].v, b["whhs"].v, unscale=False).numpy(),
                     G.unpack_whhT(b["whhT8"].v, b["whhTs"].v).numpy(), _np(b["bias4"]))
    host = R.net_from(m)
    assert np.array_equal(net["whh"], host["whh"]) and np.array_equal(net["whhT"], host["whhT"])
    # the pre-scaled biases: a sum and a product in fp32 (the references use the packed values themselves)
    mag = np.abs(m["b_ih"].astype(np.float64)) + np.abs(m["b_hh"])
    lim = 4 * U * abs(R.GS_N) * np.stack([mag[:RH], mag[RH:2 * RH], mag[2 * RH:], mag[2 * RH:]])
    assert (np.abs(net["bias4"] - host["bias4"]) <= lim).all()
    wq = _np(b["wq"]).reshape(4, RH)
    assert _same_f32(wq[:3], m["w_q"]) and _same_f32(wq[3, :3], m["b_q"]) and (_fbits(wq[3, 3:]) == 0).all()
    out = {"m": m, "b": b, "net": net, "w_q": _band(m["w_q"], NAN)}
    _PACKED[(seed, heavy)] = out
    return out


# ----------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("S", R.GATHER_S)
def test_gather(native_built, S):
    G, k = _k()
    cap = R.GATHER_CAP
    ring = R.gather_ring(S, cap, seed=S)
    rb = Bufs(rx=_band(_i16(ring["rx"]), BF_NAN), rh0=_band(_i16(ring["rh0"]), BF_NAN), ra=_band(ring["ra"], 0),
              rr=_band(ring["rr"], NAN), rd=_band(ring["rd"], 0))
    n = 0
    for B in R.GATHER_B:
        for fill in R.GATHER_FILL:
            for step in R.GATHER_STEPS:
                n += 1
                tag = (S, B, fill, step)
                b = Bufs(rb)
                b["rctrl"] = _band(np.array([fill + 7, fill], np.int64), 0)    # cursor != fill
                b["step"] = _band(np.array([step], np.int64), 0)
                b["X"] = _out((S + 1) * B * RFL, torch.bfloat16, BF_SENT)
                b["H0"] = _out(B * RH, torch.float32, F_SENT)
                b["A"], b["R"], b["D"] = (_out(S * B, torch.int32, I_SENT), _out(S * B, torch.float32, F_SENT),
                                          _out(S * B, torch.float32, F_SENT))
                g = G.GatherArgs()
                g.rx, g.ra, g.rr, g.rd, g.rh0 = (b[x].ptr() for x in ("rx", "ra", "rr", "rd", "rh0"))
                g.rctrl, g.cap, g.S, g.B, g.key0, g.key1, g.step = b["rctrl"].ptr(), cap, S, B, R.KEY0, R.KEY1, b["step"].ptr()
                g.X, g.H0, g.A, g.R, g.D = (b[x].ptr() for x in ("X", "H0", "A", "R", "D"))
                before = b.snap()
                assert _launch(k.st_gru_gather, g) == 0, tag
                b.check(before, written=("X", "H0", "A", "R", "D"))
                ref = R.gather_ref(ring, S, B, step, fill)
                assert (ref["idx"] < max(fill, 1)).all()
                X = _bfbits(b["X"]).reshape((S + 1) * B, RFL)
                got = {"X": X, "H0": _fbits(_np(b["H0"])), "A": _np(b["A"]), "R": _np(b["R"]), "D": _np(b["D"])}
                assert R.check_gather(got, ref) == 0, tag
                assert (X[:, RF] == 0x3F80).all() and (X[:, RF + 1:] == 0).all(), tag
                t, bb = np.meshgrid(np.arange(S + 1), np.arange(B), indexing="ij")
                assert np.array_equal(X[R.row_tb(t, bb, B), :RF], ring["rx"][ref["idx"][bb], t]), tag   # time-major
    # bad S: nothing is launched
    for bad in (0, 65):
        g.S = bad
        before = b.snap()
        assert _launch(k.st_gru_gather, g) == INVALID
        b.check(before)
    print(f"[meas] gather S={S}: {n} launches bit-equal")


# ----------------------------------------------------------------------------- 2. TD
def _td_launch(G, k, inp, B, S, burn, gamma, coef, loss0):
    b = Bufs(Q=_band(inp["Q"], NAN), Qt=_band(inp["Qt"], NAN), A=_band(inp["A"], 0), R=_band(inp["R"], NAN),
             D=_band(inp["D"], NAN), dQ=_out(S * B * 4, torch.float32, F_SENT), loss=_band(np.array([loss0], F), NAN))
    p = G.TDArgs()
    p.Q, p.Qt, p.A, p.R, p.D, p.dQ, p.loss = (b[x].ptr() for x in ("Q", "Qt", "A", "R", "D", "dQ", "loss"))
    p.B, p.S, p.burn, p.gamma, p.coef = B, S, burn, gamma, coef
    before = b.snap()
    assert _launch(k.st_gru_td, p) == 0
    b.check(before, written=("dQ", "loss"))
    return _np(b["dQ"]), float(_np(b["loss"])[0])


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("S", R.TD_S)
@pytest.mark.parametrize("B", R.TD_B)
def test_td(native_built, B, S, exact):
    G, k = _k()
    inp = R.td_inputs(B, S, exact, seed=100 * B + S)
    wd = wl = 0.0
    for burn in R.td_burns(S):
        gamma = R.TD_GAMMA_X if exact else R.TD_GAMMA_R
        coef = R.TD_COEF_X if exact else float(F(2.0 / (B * (S - burn))))
        sq = R.td_ref(inp, B, S, burn, gamma, coef)[2]
        loss0 = 3.5 if exact else float(R.start_below(sq.sum()))
        dq, loss = _td_launch(G, k, inp, B, S, burn, gamma, coef, loss0)
        bad, r1, r2 = R.check_td(dq, loss, loss0, inp, B, S, burn, gamma, coef, exact)
        print(f"[meas] td B={B} S={S} burn={burn} {'exact' if exact else 'random'}: dQ err/bound {r1:.4f} loss err/bound {r2:.4f}")
        assert bad == 0, (B, S, burn)
        d = dq.reshape(S * B, 4)
        assert (_fbits(d[:burn * B]) == 0).all() and (_fbits(d[:, 3]) == 0).all()
        wd, wl = max(wd, r1), max(wl, r2)


# ----------------------------------------------------------------------------- 3. forward
def _fwd_launch(G, k, inp, on, tg, B, S, pad=8):
    """One st_gru_seq_fwd launch on banded buffers.  Returns (rc, sv bits [5][S][B][RH], HT bits [S][B][RH], Q,
    Qt); X's columns >= RF are NaN (the unroll reads RF columns), HT has ``pad`` spare columns and 64 spare
    rows that must keep the sentinel, like its blocks >= S."""
    X = np.full(((S + 1) * B, RFL), BF_NAN, np.uint16)
    X[:, :RF] = R.bf16_bits(inp["x"].astype(F)).reshape((S + 1) * B, RF)
    ldht = (S + 1) * B + pad
    b = Bufs(X=_band(_i16(X), BF_NAN), H0=_band(inp["h0"].astype(F), NAN), D=_band(inp["D"], NAN),
             Q=_out((S + 1) * B * 4, torch.float32, F_SENT), Qt=_out((S + 1) * B * 4, torch.float32, F_SENT),
             HT=_out((RH + 64) * ldht, torch.bfloat16, BF_SENT), sv=_out(R.sv_size(S, B) // 2, torch.int32, I_SENT))
    f = G.SeqFwdArgs()
    for w, pk in ((f.on, on), (f.tg, tg)):
        G.set_netw(w, {n: band.v for n, band in pk["b"].items()})
    f.X, f.H0, f.D, f.Q, f.Qt, f.HT, f.ldht, f.sv, f.B, f.S = (b["X"].ptr(), b["H0"].ptr(), b["D"].ptr(), b["Q"].ptr(),
                                                                 b["Qt"].ptr(), b["HT"].ptr(), ldht, b["sv"].ptr(), B, S)
    before = b.snap()
    wsnap = [{n: band.snap() for n, band in pk["b"].items()} for pk in (on, tg)]
    rc = _launch(k.st_gru_seq_fwd, f)
    for pk, sn in zip((on, tg), wsnap):
        for n, band in pk["b"].items():
            assert band.same(sn[n]), n
    if rc != 0:
        b.check(before)
        return rc, None, None, None, None
    b.check(before, written=("Q", "Qt", "HT", "sv"))
    HT = _bfbits(b["HT"]).reshape(RH + 64, ldht)
    sent = R.bf16_bits(np.array([BF_SENT], F))[0]
    assert (HT[RH:] == sent).all() and (HT[:, S * B:] == sent).all(), "HT written outside blocks 0..S-1 of rows 0..RH-1"
    blk, bb = np.meshgrid(np.arange(S), np.arange(B), indexing="ij")
    ht = HT[:RH, R.ht_col(blk, bb, B)].transpose(1, 2, 0)
    sv = R.sv_unpack(bits(b["sv"].cpu()).numpy().view(np.uint16), S, B)
    return rc, sv, ht, _np(b["Q"]), _np(b["Qt"])


def _fwd_case(B, S, pattern, chain=False):
    G, k = _k()
    on, tg = _packed(11), _packed(12)
    inp = R.fwd_inputs(B, S, pattern, seed=10 * B + S)
    rc, sv, ht, Q, Qt = _fwd_launch(G, k, inp, on, tg, B, S)
    assert rc == 0
    worst = {}
    for name, pk, args in (("online", on, (sv, ht, Q)), ("target", tg, (None, None, Qt))):
        ref = R.fwd_ref(inp, pk["net"], B, S)
        ch = R.fwd_chain_bound(inp, pk["net"], B, S) if chain else None
        if ch is not None and name == "online":
            print("[meas] flip-noise floor (max over steps) r, z, n, gh_n, h_prev:",
                  " ".join(f"{v:.3g}" for v in ch["sv"].max(1)), f"HT {ch['hm'].max():.3g} Q {ch['Q'].max():.3g}")
        bad, w = R.check_fwd(ref, *args, B, S, ch)
        print(f"[meas] fwd {name} B={B} S={S} D={pattern}{' chain' if chain else ''}: tight steps "
              f"{int(ref['tight'].sum())} of {ref['tight'].size}; err/bound " + " ".join(f"{n} {v:.4f}" for n, v in w.items()))
        assert bad == 0, (name, B, S, pattern, bad)
        worst[name] = w
    return worst


@pytest.mark.parametrize("S", R.FWD_S_RESET)
@pytest.mark.parametrize("B", R.FWD_B)
def test_forward_every_step_reset(native_built, B, S):
    """D all ones: every step starts from h = 0 (step 0 from an H0 on the MX-fp8 grid), so every step of both
    nets is an independent step with counted bounds."""
    _fwd_case(B, S, "ones")


@pytest.mark.parametrize("B,S", [(32, 9), (96, 64)])
def test_forward_mixed_resets(native_built, B, S):
    """Resets between runs of 1..4 steps: the steps right after a reset get the counted bounds."""
    _fwd_case(B, S, "mixed")


def test_forward_chains(native_built):
    """Steps inside un-reset runs: CHAIN_FACTOR times the flip noise of the reference on top of the counted
    bound."""
    _fwd_case(*R.FWD_CHAIN, "mixed", chain=True)


def test_forward_rejections(native_built):
    G, k = _k()
    on, tg = _packed(11), _packed(12)
    inp = R.fwd_inputs(96, 1, "ones", seed=1)
    for B, S in ((48, 1), (32, 0), (32, 65)):
        # (the buffers are those of B = 96, S = 1; the arguments are refused before any launch)
        X = np.full((2 * 96, RFL), BF_NAN, np.uint16)
        b = Bufs(X=_band(_i16(X), BF_NAN), H0=_band(inp["h0"].astype(F), NAN), D=_band(inp["D"], NAN),
                 Q=_out(2 * 96 * 4, torch.float32, F_SENT), HT=_out((RH + 64) * 2 * 96, torch.bfloat16, BF_SENT),
                 sv=_out(R.sv_size(1, 96) // 2, torch.int32, I_SENT))
        f = G.SeqFwdArgs()
        for w, pk in ((f.on, on), (f.tg, tg)):
            G.set_netw(w, {n: band.v for n, band in pk["b"].items()})
        f.X, f.H0, f.D, f.Q, f.Qt, f.HT, f.ldht, f.sv, f.B, f.S = (b["X"].ptr(), b["H0"].ptr(), b["D"].ptr(), b["Q"].ptr(),
                                                                     b["Q"].ptr(), b["HT"].ptr(), 2 * 96, b["sv"].ptr(), B, S)
        before = b.snap()
        assert _launch(k.st_gru_seq_fwd, f) == INVALID, (B, S)
        b.check(before)


# ----------------------------------------------------------------------------- 4. backward
def _bwd_bufs(inp, pk, B, S):
    sv = R.sv_pack(inp["sv"], S, B)
    return Bufs(sv=_band(_i16(sv), BF_NAN), dQ=_band(inp["dQ"], NAN), D=_band(inp["D"], NAN),
                dGxT=_out(RG * S * B, torch.bfloat16, BF_SENT), dGhT=_out(RG * S * B, torch.bfloat16, BF_SENT))


def _bwd_args(G, b, pk, B, S, stride):
    p = G.SeqBwdArgs()
    p.sv, p.dQ, p.D, p.wq = b["sv"].ptr(), b["dQ"].ptr(), b["D"].ptr(), pk["w_q"].ptr()
    p.whhT8, p.whhTs = pk["b"]["whhT8"].ptr(), pk["b"]["whhTs"].ptr()
    p.dGxT, p.dGhT, p.B, p.S, p.gq_stride = b["dGxT"].ptr(), b["dGhT"].ptr(), B, S, stride
    return p


def _bwd_case(B, S, burn, D, seed=None):
    """Both Q-head paths of one case; returns the err/bound figures."""
    G, k = _k()
    pk = _packed(21, heavy=True)
    inp = R.bwd_inputs(B, S, burn, seed=(B + S) if seed is None else seed, D=D)
    ref = R.bwd_ref(inp, pk["net"], B, S)
    nwg = B // R.LBB
    assert nwg == B // int(k.st_gru_seq_bwd_rows())
    out = {}
    # atomics onto start values
    sgn = np.where((np.arange(RH)[None, :] + np.arange(3)[:, None]) % 2 == 0, 0.5, -0.25)
    gwq0 = (sgn * R.start_below(ref["agwq"].sum(0))).astype(F)
    gbq0 = (np.array([0.5, -0.25, 0.5]) * R.start_below(ref["agbq"].sum(0))).astype(F)
    b = _bwd_bufs(inp, pk, B, S)
    b["gwq"], b["gbq"] = _band(gwq0, NAN), _band(gbq0, NAN)
    p = _bwd_args(G, b, pk, B, S, 0)
    p.gwq, p.gbq = b["gwq"].ptr(), b["gbq"].ptr()
    before, wsn, qsn = b.snap(), {n: v.snap() for n, v in pk["b"].items()}, pk["w_q"].snap()
    assert _launch(k.st_gru_seq_bwd, p) == 0
    b.check(before, written=("dGxT", "dGhT", "gwq", "gbq"))
    assert all(v.same(wsn[n]) for n, v in pk["b"].items()) and pk["w_q"].same(qsn)
    got = {"dGhT": _bfbits(b["dGhT"]), "dGxT": _bfbits(b["dGxT"]), "gwq": _np(b["gwq"]), "gbq": _np(b["gbq"])}
    bad, w = R.check_bwd(got, ref, B, S, gwq0.astype(np.float64), gbq0.astype(np.float64))
    print(f"[meas] bwd B={B} S={S} burn={burn} D={D} atomic: err/bound " + " ".join(f"{n} {v:.4f}" for n, v in w.items()))
    assert bad == 0, (B, S, burn, D, "atomic", bad)
    out["atomic"] = w
    # one zeroed row per workgroup, then the ordered reduce
    stride = R.GQ_STRIDE
    part0 = np.zeros((nwg, stride), F)
    part0[:, 3 * RH + 3:] = F_SENT
    b2 = _bwd_bufs(inp, pk, B, S)
    b2["part"] = _band(part0, NAN)
    p = _bwd_args(G, b2, pk, B, S, stride)
    p.gwq, p.gbq = b2["part"].ptr(), b2["part"].ptr() + 3 * RH * 4
    before = b2.snap()
    assert _launch(k.st_gru_seq_bwd, p) == 0
    b2.check(before, written=("dGxT", "dGhT", "part"))
    part = _np(b2["part"]).reshape(nwg, stride)
    assert (part[:, 3 * RH + 3:] == F(F_SENT)).all()
    for key in ("dGhT", "dGxT"):      # the same arithmetic on either path
        assert np.array_equal(_bfbits(b2[key]), got[key]), key
    got2 = dict(got, gwq=part[:, :3 * RH].reshape(nwg, 3, RH), gbq=part[:, 3 * RH:3 * RH + 3])
    bad, w = R.check_bwd(got2, ref, B, S)
    print(f"[meas] bwd B={B} S={S} burn={burn} D={D} ordered: err/bound gwq {w['gwq']:.4f} gbq {w['gbq']:.4f}")
    assert bad == 0, (B, S, burn, D, "ordered", bad)
    b2["gwq"], b2["gbq"] = _out(3 * RH, torch.float32, F_SENT), _out(3, torch.float32, F_SENT)
    before = b2.snap()
    assert _launch(k.st_gru_qgrad_reduce, b2["part"].ptr(), nwg, stride, b2["gwq"].ptr(), b2["gbq"].ptr()) == 0
    b2.check(before, written=("gwq", "gbq"))
    want = R.reduce_ref(part)
    assert _same_f32(_np(b2["gwq"]), want[:3 * RH]) and _same_f32(_np(b2["gbq"]), want[3 * RH:])
    out["ordered"] = w
    return out


@pytest.mark.parametrize("B", R.BWD_B)
def test_backward_single_step(native_built, B):
    """S = 1: no recurrent product."""
    _bwd_case(B, 1, 0, "random")


@pytest.mark.parametrize("S", [2, 24, 64])
@pytest.mark.parametrize("B", R.BWD_B)
def test_backward_independent_steps(native_built, B, S):
    """keep = 0 everywhere (D all ones): every step is independent."""
    _bwd_case(B, S, min(4, S - 1), "ones")


@pytest.mark.parametrize("B", R.BWD_B)
def test_backward_one_recurrent_product(native_built, B):
    """keep = 1, S = 2, dQ zero at t = 0: the outputs of t = 0 are the recurrent product alone, bounded by
    the hi/lo MX-fp8 representation of dGh."""
    _bwd_case(B, 2, 1, "zeros")


@pytest.mark.parametrize("S,burn", [(4, 1), (24, 4), (64, 4)])
@pytest.mark.parametrize("B", R.BWD_B)
def test_backward_chains(native_built, B, S, burn):
    _bwd_case(B, S, burn, "random")


def test_backward_rejections(native_built):
    G, k = _k()
    pk = _packed(21, heavy=True)
    inp = R.bwd_inputs(96, 1, 0, seed=1)
    b = _bwd_bufs(inp, pk, 96, 1)
    b["part"] = _band(np.zeros((6, R.GQ_STRIDE), F), NAN)
    for B, S, stride in ((32, 1, -1), (32, 1, 1), (32, 1, 770), (48, 1, 0), (32, 0, 0), (32, 65, 0)):
        p = _bwd_args(G, b, pk, B, S, stride)
        p.gwq, p.gbq = b["part"].ptr(), b["part"].ptr() + 3 * RH * 4
        before = b.snap()
        assert _launch(k.st_gru_seq_bwd, p) == INVALID, (B, S, stride)
        b.check(before)
    b["gwq"], b["gbq"] = _out(3 * RH, torch.float32, F_SENT), _out(3, torch.float32, F_SENT)
    ok = dict(part=b["part"].ptr(), rows=6, stride=R.GQ_STRIDE, gwq=b["gwq"].ptr(), gbq=b["gbq"].ptr())
    for kw in (dict(part=None), dict(gwq=None), dict(gbq=None), dict(rows=0), dict(stride=3 * RH + 2)):
        a = dict(ok, **kw)
        before = b.snap()
        assert _launch(k.st_gru_qgrad_reduce, a["part"], a["rows"], a["stride"], a["gwq"], a["gbq"]) == INVALID, kw
        b.check(before)


# ----------------------------------------------------------------------------- 5. Q-gradient reduce, fixup
@pytest.mark.parametrize("rows", R.REDUCE_ROWS)
def test_qgrad_reduce(native_built, rows):
    G, k = _k()
    for exact in (True, False):
        for stride in (R.GQ_STRIDE, R.GQ_STRIDE + 5):
            part = R.reduce_inputs(rows, stride, exact, seed=rows + stride)
            b = Bufs(part=_band(part, NAN), gwq=_out(3 * RH, torch.float32, F_SENT), gbq=_out(3, torch.float32, F_SENT))
            before = b.snap()
            assert _launch(k.st_gru_qgrad_reduce, b["part"].ptr(), rows, stride, b["gwq"].ptr(), b["gbq"].ptr()) == 0
            b.check(before, written=("gwq", "gbq"))
            want = R.reduce_ref(part)       # the fp32 sum in row order: bit-equal, exact or not
            assert _same_f32(_np(b["gwq"]), want[:3 * RH]) and _same_f32(_np(b["gbq"]), want[3 * RH:]), (rows, exact, stride)
            if exact and rows >= 3:
                assert not _same_f32(_np(b["gwq"]), R.reduce_ref(part, reverse=True)[:3 * RH])


@pytest.mark.parametrize("ldx", [RH + 64, RH + 72])
def test_grad_fixup(native_built, ldx):
    G, k = _k()
    g = np.random.default_rng(ldx)
    ext, dwih = g.standard_normal((RG, ldx)).astype(F), g.standard_normal((RG, RFL)).astype(F)
    b = Bufs(ext=_band(ext, NAN), dwih=_band(dwih, NAN), dwhh=_out(RG * RH, torch.float32, F_SENT),
             dbhh=_out(RG, torch.float32, F_SENT), dbih=_out(RG, torch.float32, F_SENT))
    before = b.snap()
    assert _launch(k.st_gru_grad_fixup, b["ext"].ptr(), ldx, b["dwhh"].ptr(), b["dbhh"].ptr(), b["dwih"].ptr(),
                   b["dbih"].ptr()) == 0
    b.check(before, written=("dwhh", "dbhh", "dwih", "dbih"))
    ref = R.fixup_ref(ext, dwih, ldx)
    for key in ("dwhh", "dbhh", "dbih", "dwih"):
        assert _same_f32(_np(b[key]), ref[key].reshape(-1)), key
    assert (_fbits(_np(b["dwih"]).reshape(RG, RFL)[:, RF]) == 0).all()
