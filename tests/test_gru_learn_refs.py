"""The references of tests/gru_learn_refs.py would notice a wrong kernel (CPU only).

As tests/test_deep_kernel_refs.py does for the deep learner: each check applies one mutation to the expected
values or to an index map, stores the result the way the kernel would (fp32 / bf16, in the kernel's layout),
and runs the very comparison tests/test_gpu_gru_learn_kernels.py uses (the ``check_*`` functions of the refs
module) over the committed case lists.  It must fail on at least one case; every mutation prints its count of
failing entries and its err / bound.  The layout maps are checked for being bijections, the hand-written
backward against torch autograd of the forward, and the torch model of the backward's fp8 hi/lo pair against
its counted bound."""
import itertools

import numpy as np
import pytest
import torch

import gru_learn_refs as R

U, F = R.U, np.float32


def _bits(x):
    return R.bf16_bits(np.asarray(x, np.float64).astype(F)).reshape(np.shape(x))


# ----------------------------------------------------------------------------- layout maps
@pytest.mark.parametrize("B,S", [(32, 1), (96, 3)])
def test_layout_maps_are_bijections(B, S):
    n = R.sv_size(S, B)
    t, b, u, q = np.meshgrid(np.arange(S), np.arange(B), np.arange(R.RH), np.arange(R.NSV), indexing="ij")
    idx = R.sv_index(t, b, u, q, B).ravel()
    assert idx.min() == 0 and idx.max() == n - 1 and np.unique(idx).size == n == t.size
    back = R.sv_coords(idx, B)
    for got, want in zip(back, (t, b, u, q)):
        assert np.array_equal(got, want.ravel())
    for pair in itertools.combinations(R._ORDER, 2):
        assert not np.array_equal(R.sv_index(t, b, u, q, B, swap=pair).ravel(), idx), pair
    # HT columns, X / Q / dQ rows, dGxT / dGhT columns
    blk, bb = np.meshgrid(np.arange(S + 1), np.arange(B), indexing="ij")
    assert np.array_equal(np.sort(R.ht_col(blk, bb, B).ravel()), np.arange((S + 1) * B))
    assert np.array_equal(np.sort(R.row_tb(blk, bb, B).ravel()), np.arange((S + 1) * B))
    assert not np.array_equal(R.row_tb(blk, bb, B), bb * (S + 1) + blk) or S == 0
    # the backward's workgroups cover every (forward block, tile) once; the swapped map differs
    ids = [R.bwd_block(i) for i in range(B // R.LBB)]
    assert sorted(ids) == [(f, n) for f in range(B // R.LB) for n in range(2)]
    assert [R.bwd_block(i, True) for i in range(B // R.LBB)] != ids
    # the saves round-trip through pack / unpack
    g = np.random.default_rng(0)
    q5 = R.bf(g.standard_normal((R.NSV, S, B, R.RH)).astype(F))
    assert np.array_equal(R.sv_unpack(R.sv_pack(q5, S, B), S, B), _bits(q5))


# ----------------------------------------------------------------------------- gather
def _gather_cases():
    for S in R.GATHER_S:
        ring = R.gather_ring(S, 64, seed=S)       # (a small ring here: the fills stay below it)
        for B in R.GATHER_B:
            for size in (0, 1, 5, 61):
                for step in R.GATHER_STEPS:
                    yield ring, S, B, step, size


def test_gather_mutations_are_caught():
    cases = list(_gather_cases())
    for name, mut, applies in (("low word as the index", dict(low_word=True), lambda S, size: size == 61),
                               ("second pass dropped", dict(one_pass=True), lambda S, size: S >= 24),
                               ("column RF not set", dict(ones_col=False), lambda S, size: True),
                               ("A / R / D at lane < S - 1", dict(short_ard=True), lambda S, size: True)):
        n = []
        for ring, S, B, step, size in cases:
            ref = R.gather_ref(ring, S, B, step, size)
            assert R.check_gather(ref, ref) == 0
            if applies(S, size):
                n.append(R.check_gather(R.gather_ref(ring, S, B, step, size, **mut), ref))
        print(f"[mutation] gather, {name}: differing entries per case min {min(n)} max {max(n)}")
        assert max(n) > 0 and (min(n) > 0 or name.startswith("low word"))
    # a step counter above 2^32 draws differently from its low word
    assert not np.array_equal(R.seq_index(32, 2 ** 32 + 1, 61), R.seq_index(32, 1, 61))


# ----------------------------------------------------------------------------- TD
def _td_cases(exact):
    for B in R.TD_B:
        for S in R.TD_S:
            inp = R.td_inputs(B, S, exact, seed=100 * B + S)
            for burn in R.td_burns(S):
                gamma = R.TD_GAMMA_X if exact else R.TD_GAMMA_R
                coef = R.TD_COEF_X if exact else float(F(2.0 / (B * (S - burn))))
                yield inp, B, S, burn, gamma, coef


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_td_mutations_are_caught(exact):
    cases = list(_td_cases(exact))
    if exact:   # the assumptions of the exact case: ties of two and three, every value exact in fp32
        inp = cases[0][0]
        q = inp["Q"][:, :3]
        assert ((q[:, 0] == q[:, 1]) & (q[:, 1] == q[:, 2])).any() and ((q[:, 0] == q[:, 1]) & (q[:, 1] != q[:, 2])).any()
    for name, mut in (("none", {}), ("argmax on the target net", dict(target_argmax=True)),
                      ("last index wins a tie", dict(last_tie=True)), ("(1 - D) dropped", dict(no_done=True)),
                      ("burn mask one late", dict(burn_off=1)), ("burn mask one early", dict(burn_off=-1)),
                      ("coef on masked rows", dict(coef_masked=True))):
        if name == "last index wins a tie" and not exact:
            continue          # random values have no ties
        n, rt = [], 0.0
        for inp, B, S, burn, gamma, coef in cases:
            dQ, _, sq, _ = R.td_ref(inp, B, S, burn, gamma, coef, **mut)
            bad, r1, r2 = R.check_td(dQ.astype(F), F(3.5 + sq.sum()) if exact else F(sq.sum()), 3.5 if exact else 0.0,
                                     inp, B, S, burn, gamma, coef, exact)
            n.append(bad)
            rt = max(rt, r1, r2)
        print(f"[mutation] td {'exact' if exact else 'random'}, {name}: failing entries per case min {min(n)} max {max(n)}, "
              f"err/bound {rt:.3g}")
        assert (max(n) == 0) if name == "none" else (max(n) > 0), name


# ----------------------------------------------------------------------------- forward
_NETS = {}


def _nets():
    if not _NETS:
        _NETS["on"], _NETS["tg"] = R.net_from(R.masters(11)), R.net_from(R.masters(12))
    return _NETS["on"], _NETS["tg"]


def _fwd_store(ref, B, S, swap=None):
    """A forward result as the kernel stores it, read back the way the GPU test reads it."""
    sv = R.sv_unpack(R.sv_pack(ref["sv"], S, B, swap), S, B)
    ht = np.concatenate([_bits(ref["sv"][R.SV_HP, :1]), _bits(ref["hm"][:S - 1])])
    Q = np.zeros((S + 1, B, 4), F)
    Q[:, :, :3] = ref["Q"]
    return sv, ht, Q


_FWD_MUT = (("none", {}, None, False), ("keep before the Q head", dict(keep_first=True), None, False),
            ("x_t and x_t+1 swapped", dict(swap_x=True), None, False), ("gh_n left pre-scaled", dict(gh_scaled=True), None, False),
            ("h_prev saved after the update", dict(hp_after=True), None, False),
            ("tiles n = 0 / 1 swapped in sv", {}, ("m", "n"), False), ("target net with online W_ih", {}, None, True))


def _fwd_mutations(cases, chain_of, chain_only=False):
    """Run every forward mutation over ``cases`` [(B, S, pattern)]; chain_of(inp, net) -> chain bound or None."""
    on, tg = _nets()
    table = {}
    for B, S, pattern in cases:
        inp = R.fwd_inputs(B, S, pattern, seed=10 * B + S)
        ref_on, ref_tg = R.fwd_ref(inp, on, B, S), R.fwd_ref(inp, tg, B, S)
        ch_on, ch_tg = chain_of(inp, on, B, S), chain_of(inp, tg, B, S)
        for name, mut, swap, tgmut in _FWD_MUT:
            if tgmut:
                got = R.fwd_ref(inp, tg, B, S, wih=on["wih"])
                bad, w = R.check_fwd(ref_tg, None, None, _fwd_store(got, B, S)[2], B, S, ch_tg, chain_only)
            else:
                sv, ht, Q = _fwd_store(R.fwd_ref(inp, on, B, S, **mut), B, S, swap)
                bad, w = R.check_fwd(ref_on, sv, ht, Q, B, S, ch_on, chain_only)
            table.setdefault(name, []).append((bad, max(w.values())))
    return table


def _report(kind, table):
    for name, rows in table.items():
        n, rt = [r[0] for r in rows], max(r[1] for r in rows)
        print(f"[mutation] {kind}, {name}: failing entries per case min {min(n)} max {max(n)}, err/bound {rt:.3g}")
        assert (max(n) == 0) if name == "none" else (max(n) > 0), (kind, name)


def test_forward_mutations_are_caught_reset_cases():
    cases = [(32, S, "ones") for S in R.FWD_S_RESET if S <= 24] + [(32, 9, "mixed")]
    _report("forward, reset steps", _fwd_mutations(cases, lambda *a: None))


def test_forward_mutations_are_caught_under_the_chain_bound():
    """The measured flip-noise floor times CHAIN_FACTOR still tells every mutation on the steps inside runs
    alone (chain_only: the steps that start from an exact h are left out of the count)."""
    B, S = 32, 64
    floors = {}

    def chain_of(inp, net, B, S):
        ch = R.fwd_chain_bound(inp, net, B, S)
        floors.setdefault("sv", ch["sv"].max(1)), floors.setdefault("hm", ch["hm"].max()), floors.setdefault("Q", ch["Q"].max())
        return ch

    _report("forward, chains", _fwd_mutations([(B, S, "mixed")], chain_of, chain_only=True))
    print("[meas] flip-noise floor (max over steps) r, z, n, gh_n, h_prev:", " ".join(f"{v:.3g}" for v in floors["sv"]),
          f"HT {floors['hm']:.3g} Q {floors['Q']:.3g}")


# ----------------------------------------------------------------------------- backward
def _bnet():
    if "bw" not in _NETS:
        _NETS["bw"] = R.net_from(R.masters(21, heavy=True))
    return _NETS["bw"]


BWD_CASES = [(32, 1, 0, "random"), (96, 1, 0, "random"), (32, 2, 0, "ones"), (32, 24, 4, "ones"), (32, 2, 1, "zeros"),
             (96, 2, 1, "zeros"), (32, 4, 1, "random"), (96, 24, 4, "random")]
_BWD_MUT = (("none", {}), ("pkeep from D[t + 1]", dict(keep_next=True)), ("pkeep zero from t = S-2 on", dict(keep_zero_early=True)),
            ("dGx's n rows equal to dGh's", dict(gx_as_gh=True)), ("1 - r dropped", dict(no_1mr=True)),
            ("fn and fblk swapped", dict(swap_blk=True)), ("W_q gradient from the masked h", dict(masked_h=True)),
            ("gbq over one tile only", dict(gbq_one_tile=True)), ("lo half dropped", dict(drop_lo=True)))


def test_backward_mutations_are_caught():
    net = _bnet()
    table = {}
    for B, S, burn, D in BWD_CASES:
        inp = R.bwd_inputs(B, S, burn, seed=B + S, D=D)
        ref = R.bwd_ref(inp, net, B, S)
        for name, mut in _BWD_MUT:
            got = R.bwd_store(R.bwd_ref(inp, net, B, S, **mut), B, S)
            bad, w = R.check_bwd(got, ref, B, S)
            table.setdefault(name, []).append((bad, max(w.values())))
        # pkeep = 1 - D at t = S-1 changes nothing: the recurrent gradient it multiplies starts at zero
        same = R.bwd_store(R.bwd_ref(inp, net, B, S, keep_last=True), B, S)
        assert all(np.array_equal(same[k], R.bwd_store(ref, B, S)[k]) for k in same)
    _report("backward", table)
    print("[mutation] backward, pkeep not zero at t = S-1: an equivalent mutant (rec is zero there), output bit-identical")


def test_quant_hilo_model_stays_inside_the_counted_bound():
    """The torch model of quant_hilo (mx_exp, float8_e4m3fn, residual) on the dGh of the S = 2 case: hi + lo
    is within the counted bound everywhere, hi alone is not."""
    net = _bnet()
    inp = R.bwd_inputs(32, 2, 1, seed=34, D="zeros")
    x = R.bwd_ref(inp, net, 32, 2)["dGh"][1]
    hi, lo = R.quant_hilo_model(x)
    bound = R.hilo_bound(x)
    e2, e1 = np.abs(x.astype(F).astype(np.float64) - hi - lo), np.abs(x - hi)
    print(f"[meas] quant_hilo model: hi + lo err/bound {R.ratio(e2, bound):.3g}, hi alone err/bound {R.ratio(e1, bound):.3g}")
    assert (e2 <= bound).all() and (e1 > bound).any()
    # subnormal floor: a block with one large and many tiny values
    y = np.full((1, 768), 1e-7)
    y[0, ::32] = 3.0
    hi, lo = R.quant_hilo_model(y)
    assert (np.abs(y.astype(F).astype(np.float64) - hi - lo) <= R.hilo_bound(y)).all()


def test_reference_backward_equals_autograd_of_reference_forward():
    """B = 32, S = 5 with resets: the hand-written backward (fed the forward's own un-rounded saves) gives
    the gradients torch autograd gives for the same forward in float64, to 1e-10."""
    B, S = 32, 5
    net = _bnet()
    g = np.random.default_rng(3)
    x = torch.from_numpy(g.standard_normal((S, B, R.RF)))
    D = torch.from_numpy((g.random((S, B)) < 0.3).astype(np.float64))
    dQ = g.standard_normal((S, B, 3))
    Wi = torch.from_numpy(g.standard_normal((R.RG, R.RF)) * 0.2)
    W = torch.from_numpy(net["whhT"]).clone().requires_grad_(True)
    wq = torch.from_numpy(net["wq"]).clone().requires_grad_(True)
    bq = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    bh = torch.from_numpy(g.standard_normal(R.RG) * 0.2)
    h = torch.from_numpy(0.5 * g.standard_normal((B, R.RH)))
    sv = np.zeros((R.NSV, S, B, R.RH))
    gxs, ghs, loss = [], [], 0.0
    for t in range(S):
        gx = (x[t] @ Wi.t()).requires_grad_(True)
        gh = h @ W.t() + bh
        gh.retain_grad(), gx.retain_grad()
        gxs.append(gx), ghs.append(gh)
        r = torch.sigmoid(gx[:, :256] + gh[:, :256])
        z = torch.sigmoid(gx[:, 256:512] + gh[:, 256:512])
        n = torch.tanh(gx[:, 512:] + r * gh[:, 512:])
        for q, v in ((0, r), (1, z), (2, n), (3, gh[:, 512:]), (4, h)):
            sv[q, t] = v.detach().numpy()
        h = z * (h - n) + n
        loss = loss + ((h @ wq.t() + bq) * torch.from_numpy(dQ[t])).sum()
        h = h * (1 - D[t])[:, None]
    loss.backward()
    dq4 = np.zeros((S, B, 4), np.float64)
    dq4[:, :, :3] = dQ
    ref = R.bwd_ref({"sv": sv, "dQ": dq4, "D": D.numpy()}, net, B, S)
    for t in range(S):
        assert np.abs(ref["dGh"][t] - ghs[t].grad.numpy()).max() < 1e-10, t
        assert np.abs(ref["dGx"][t] - gxs[t].grad.numpy()).max() < 1e-10, t
    assert np.abs(ref["gwq"].sum(0) - wq.grad.numpy()).max() < 1e-10
    assert np.abs(ref["gbq"].sum(0) - bq.grad.numpy()).max() < 1e-10


# ----------------------------------------------------------------------------- reduce, fixup
def test_reduce_and_fixup_mutations_are_caught():
    for rows in R.REDUCE_ROWS:
        p = R.reduce_inputs(rows, R.GQ_STRIDE, True, rows)
        # (two rows commute: the order of the sum shows from three rows on)
        assert (rows < 3) == np.array_equal(R.reduce_ref(p), R.reduce_ref(p, reverse=True)), rows
    g = np.random.default_rng(1)
    ext, dwih = g.standard_normal((R.RG, R.RH + 64)).astype(F), g.standard_normal((R.RG, R.RFL)).astype(F)
    ref, got = R.fixup_ref(ext, dwih, R.RH + 64), R.fixup_ref(ext, dwih, R.RH + 64, col=R.RF - 1)
    n = sum(int((ref[k].view(np.uint32) != got[k].view(np.uint32)).sum()) for k in ref)
    print(f"[mutation] fixup, db_ih from column RF-1: differing entries {n}")
    assert n > 0
