"""tests/f32b_refs.py on the CPU: the exactness precondition of every exact case, the loader pair and the form every
case must select, coverage of the shape lists, the unmutated models through the ``check_*`` functions (0 differences
on every committed case) and one mutation at a time (> 0 differences each), the env rule against the torch oracle,
and the Gaussian bounds against the reference's own rounding."""
import numpy as np
import pytest
import torch

import f32b_refs as fr
from f32b_refs import F


# ----------------------------------------------------------------------------- preconditions and coverage
def test_gemm_cases_exact_and_covering():
    cases = fr.gemm_cases()
    ex = [c for c in cases if c.exact]
    assert all(c.notes["bits"] < fr.LIMIT_BITS for c in ex)
    # the loader the strides force is the loader the case is listed under, and all nine pairs occur
    assert all((c.A.mode(), c.B.mode()) == (c.am, c.bm) for c in cases)
    assert {(c.am, c.bm) for c in ex} == {(a, b) for a in range(3) for b in range(3)}
    assert {(c.am, c.bm) for c in cases if not c.exact} == {(a, b) for a in range(3) for b in range(3)}
    for mode in range(3):   # every listed M / N / K with every loader mode of the operand it belongs to
        assert {c.M for c in ex if c.am == mode} >= set(fr._MS), mode
        assert {c.N for c in ex if c.bm == mode} >= set(fr._NS), mode
        assert {c.K for c in ex if c.am == mode} >= set(fr._KS) and {c.K for c in ex if c.bm == mode} >= set(fr._KS)
    for epi in range(4):    # every tail with every epilogue
        tails = set().union(*(fr.gemm_tails(c) for c in ex if c.epi == epi))
        assert tails == {"row", "col", "k", "f4"}, (epi, tails)
    for epi in (fr.F32B_ATOMIC, fr.F32B_PARTIAL):
        assert {c.splits for c in ex if c.epi == epi} >= {1, 2, 3, 5}
    st = [c for c in ex if c.epi == fr.F32B_STORE]
    assert {(c.bias is not None, c.relu) for c in st} == {(a, b) for a in (False, True) for b in (False, True)}
    for c in st:
        if c.bias is not None and c.relu:   # the bias leaves outputs on both sides of the relu
            v = c.A.get() @ c.B.get().T + c.bias.astype(np.float64)
            assert (v < 0).any() and (v > 0).any(), c.name
    for c in ex:
        if c.epi == fr.F32B_MASK and c.M * c.N >= 7:
            assert set(fr.bits32(c.aux.get().astype(F)).ravel().tolist()) == set(fr.bits32(fr.ACT_PALETTE).tolist())
    # the split count shrinks: K = 40, 3 requested, 2 run -- and the Python side's count agrees with the launcher's
    assert fr.split_rule(40, 3) == (32, 2)
    for c in ex:
        kc, nz = fr.split_rule(c.K, c.splits)
        assert kc % 32 == 0 and nz <= c.splits and nz == -(-c.K // (-(-(-(-c.K // c.splits)) // 32) * 32))
    assert any(fr.split_rule(c.K, c.splits)[1] < c.splits for c in ex if c.epi == fr.F32B_PARTIAL)


def test_other_cases_exact_and_forms():
    for c in fr.fwd2_cases():
        if c.exact:
            assert max(c.notes["bits_h"], c.notes["bits_q"]) < fr.LIMIT_BITS, (c.name, c.notes)
    f2 = fr.fwd2_cases()
    assert {c.M for c in f2} >= {1, 63, 65, 130} and {c.K for c in f2} >= {4, 36, 100, 208}
    assert {c.N1 for c in f2} >= {1, 3, 64, 65, 200, 256} and {c.nout for c in f2} == {1, 2, 3}
    assert {(c.b1 is None, c.b2 is None, c.relu_out) for c in f2} >= {(True, True, False), (False, False, True)}
    assert {c.b1 is None for c in f2} == {c.b2 is None for c in f2} == {c.relu_out for c in f2} == {False, True}
    cs = fr.colsum_cases()
    assert {c.N for c in cs if c.vec} >= {4, 16, 200, 256} and {c.E for c in cs if c.vec} >= {1, 5, 127, 128, 129, 1000}
    fb = [c for c in cs if not fr.colsum_form(c, det=True)]
    assert {c.N for c in fb} >= {3, 203, 260, 520} and {c.E for c in fb} >= {1, 255, 256, 257, 600}
    assert any(c.D.sr % 4 for c in fb if c.N % 4 == 0) and any(c.D.off % 4 for c in fb) and any(c.out_off for c in fb)
    ss = fr.splitsum_cases()
    assert {c.splits for c in ss if not c.one} >= {1, 2, 15, 16, 17, 63, 64, 65, 130}
    assert {c.n for c in ss if not c.one} >= {4, 60, 64, 68, 160} and all(c.zstride > c.n for c in ss)
    one = [c for c in ss if c.one]
    assert {c.n for c in one} >= {1, 3, 203} and any(c.zstride % 4 and c.n % 4 == 0 for c in one)
    assert any(c.part_off for c in one) and any(c.out_off for c in one)
    for c in fr.batch_cases():
        if c.k["stat"]:
            assert c.k["dyadic"] and fr.stat_bits(c) < 53.0, c.name


def test_batch_coverage():
    """Every situation the env and TD launches must handle occurs in some committed case."""
    tot = {}
    for c in fr.batch_cases():
        for k, v in fr.batch_coverage(c).items():
            tot[k] = tot.get(k, 0) + v
    assert all(v > 0 for v in tot.values()), tot
    assert {"qs_pzero", "qs_nzero", "qs_neg", "qs_pos", "clip_hi", "clip_lo", "cur_not_positive"} <= set(tot)
    cs = fr.batch_cases()
    ks = [c.k for c in cs]
    assert {c.E for c in cs} == {1, 255, 257, 1025} and {c.H for c in cs} == {5, 201}
    for key, vals in (("feat_mode", {0, 1}), ("compat_env", {0, 1}), ("reward_mode", {0, 1, 2}), ("ramp_global", {0, 1}),
                      ("target_compat", {0, 1}), ("double_dqn", {0, 1}), ("output_relu", {0, 1}), ("use_qt", {False, True}),
                      ("stat", {False, True}), ("actions_out", {False, True}), ("rewards_out", {False, True})):
        assert {k[key] for k in ks} == vals, key
    assert any(k["env_offset"] for k in ks) and any(k["step"] >= 2 ** 32 for k in ks)
    assert any(k["reward_scale"] != 1.0 for k in ks) and any(k["reward_scale"] == 1.0 for k in ks)
    assert any(k["td_clip"] > 0 for k in ks) and any(k["td_clip"] == 0 for k in ks)
    assert any(c.E == 1025 and c.k["stat"] for c in cs)   # a last TD block with one live thread, statistics on


def test_env_rule_matches_oracle():
    """The model's trade and reward are the torch oracle's (sharetrade/env/trading.py env_transition), bit for bit."""
    from sharetrade.env.trading import env_transition

    for c in fr.batch_cases():
        ev = fr.env_model(c)
        st, k = c.state, c.k
        e = np.arange(c.E)
        vnew = torch.from_numpy(c.prices[e, st["pos"] + c.H])
        b2, s2, r = env_transition(torch.from_numpy(ev["s_act"]), torch.from_numpy(st["budget"]),
                                   torch.from_numpy(st["shares"]), torch.from_numpy(st["value"]), vnew,
                                   bool(k["compat_env"]), k["b0"], k["s0"], relative=k["reward_mode"] >= 1,
                                   growth=k["reward_mode"] == 2)
        assert fr.check_bits(b2.numpy(), ev["s_b2"].astype(F)) == 0, c.name
        assert np.array_equal(s2.numpy(), ev["s_s2"]), c.name
        assert fr.check_bits(r.numpy(), ev["s_rew"].astype(F)) == 0, c.name


# ----------------------------------------------------------------------------- the models through check_*
def _gemm_diffs(mut=None, only=None):
    """Differences of the stored C plus the loads issued outside an operand (a loaded row r == R feeds no stored
    output; it is an over-read and nothing else)."""
    fr.OUTSIDE[0] = 0
    d = sum(fr.check_gemm(c, fr.gemm_model(c, mut))[0] for c in fr.gemm_cases() if only is None or only(c))
    return d + fr.OUTSIDE[0]


def _fwd2_diffs(mut=None):
    return sum(fr.check_fwd2(c, *fr.fwd2_model(c, mut))[0] for c in fr.fwd2_cases())


def _colsum_diffs(mut=None):
    d = 0
    for c in fr.colsum_cases():
        for det in (False, True):
            out, part, nb = fr.colsum_model(c, det, mut)
            d += fr.check_colsum(c, det, out, part if det else None, nb if det else None)
    return d


def _splitsum_diffs(mut=None):
    return sum(fr.check_splitsum(c, fr.splitsum_model(c.part, c.splits, c.zstride, c.n, c.one, c.part_off, mut))[0]
               for c in fr.splitsum_cases())


def _gather_diffs(mut=None):
    return sum(fr.check_gather(c, *(x.astype(F) for x in fr.gather_model(c, mut))) for c in fr.batch_cases())


def _env_diffs(mut=None):
    return sum(fr.check_env(c, fr.env_outputs(c, mut)) for c in fr.batch_cases())


def _td_diffs(mut=None):
    return sum(fr.check_td(c, fr.td_outputs(c, mut)) for c in fr.batch_cases())


def _sync_diffs(mut=None):
    d = 0
    for n, every, c0 in fr.SYNC_CASES:
        p, t = np.arange(n, dtype=F) + 1, -np.arange(n, dtype=F) - 1
        d += fr.check_sync(p, t, every, c0, fr.sync_model(p, t, every, c0, mut))
    return d


FAMILY = {}
for _m in fr.MUTATIONS[:11]:
    FAMILY[_m] = _gemm_diffs
for _m in fr.MUTATIONS[11:14]:
    FAMILY[_m] = _fwd2_diffs
FAMILY.update(colsum_last_group=_colsum_diffs, colsum_det_adds=_colsum_diffs, splitsum_tail16=_splitsum_diffs,
              splitsum1_n_for_zstride=_splitsum_diffs, xn_not_shifted=_gather_diffs, no_bias_col=_gather_diffs,
              tie_last=_env_diffs, u2_exploit=_env_diffs, no_env_offset=_env_diffs, step_hi_ignored=_env_diffs,
              td_reset_late=_td_diffs, loss_from_clipped=_td_diffs, ddqn_target_argmax=_td_diffs,
              scale_stored_reward=_td_diffs, sync_plus_one=_sync_diffs)


def test_models_unmutated():
    for fn in (_gemm_diffs, _fwd2_diffs, _colsum_diffs, _splitsum_diffs, _gather_diffs, _env_diffs, _td_diffs,
               _sync_diffs):
        assert fn() == 0, fn.__name__


@pytest.mark.parametrize("mut", fr.MUTATIONS)
def test_mutation_caught(mut):
    assert set(FAMILY) == set(fr.MUTATIONS)
    d = FAMILY[mut](mut)
    print(f"[mut] {mut}: {d} differences")
    assert d > 0, mut


def test_loader_mutations_show_where_expected():
    """The float4 tails are caught by the cases that have them (not by an accident elsewhere)."""
    assert _gemm_diffs("kf_ktail_dropped", lambda c: c.exact and c.K % 4 == 0) == 0
    assert _gemm_diffs("kf_ktail_dropped", lambda c: c.exact and c.K % 4 and fr.LD_KF in (c.am, c.bm)) > 0
    assert _gemm_diffs("rf_rtail_dropped", lambda c: c.exact and fr.LD_RF not in (c.am, c.bm)) == 0
    assert _gemm_diffs("kchunk_unrounded", lambda c: c.name == "shrink-40-partial3") > 0


def test_partial_then_splitsum_equals_atomic_model():
    """PARTIAL tiles added by the split-sum equal the ATOMIC result on a zeroed C (dense C, the engine's use)."""
    for M, N, K, sp, am, bm, seed in fr.small_split_cases():
        p = fr.make_gemm("p", M, N, K, am, bm, fr.F32B_PARTIAL, sp, seed=seed, dense=True)
        a = fr.make_gemm("a", M, N, K, am, bm, fr.F32B_ATOMIC, sp, seed=seed, dense=True)
        a.C.put(np.zeros((M, N)))
        assert np.array_equal(p.A.flat, a.A.flat, equal_nan=True) and np.array_equal(p.B.flat, a.B.flat, equal_nan=True)
        _, nz = fr.split_rule(K, sp)
        n = M * N
        tot = fr.splitsum_model(fr.gemm_model(p), nz, p.zstride, n, one=bool(n % 4))
        assert fr.check_bits(tot.astype(F), fr.gemm_model(a)[:n]) == 0


# ----------------------------------------------------------------------------- the bounds are neither vacuous nor tight
def test_gaussian_bounds_sane():
    """The float64 reference rounded once to fp32 lies well inside the bound (a correct kernel can pass), and the
    bound is a small fraction of the magnitude it scales with (a wrong element cannot)."""
    for c in fr.gemm_cases():
        if not c.exact:
            ref, bound, mask = fr.gemm_ref(c)
            d, ratio = fr.check_bound(ref.astype(F), ref, bound, mask)
            assert d == 0 and ratio < 0.5, (c.name, ratio)
            mag = np.abs(c.A.get()) @ np.abs(c.B.get().T)
            assert bound[mask].max() < 2.0 ** -15 * mag.max(), c.name
    for c in fr.fwd2_cases():
        if not c.exact:
            h, q, bh, bq = fr.fwd2_ref(c)
            d, r1, r2 = fr.check_fwd2(c, np.r_[h.astype(F).reshape(-1), np.full(8, np.nan, F)], q.astype(F))
            assert d == 0 and r1 < 0.5 and r2 < 0.5, (c.name, r1, r2)
            assert bh.max() < 2.0 ** -14 * np.abs(h).max() * c.K and bq.max() < 2.0 ** -12 * np.abs(q).max() * c.N1
    for c in fr.colsum_cases():
        if not c.exact:
            for det in (False, True):
                ref, bound = fr.colsum_ref(c, det)
                assert (np.abs(ref.astype(F) - ref) < 0.5 * bound).all() and bound.max() < 2.0 ** -12 * c.E
    for c in fr.splitsum_cases():
        if not c.exact:
            ref = fr.splitsum_dense(c).sum(0)
            d, ratio = fr.check_splitsum(c, ref.astype(F))
            assert d == 0 and ratio < 0.5


def test_optim_reference_and_bounds():
    """The float64 optimizer reference: masked entries keep everything, bounds are positive where live, and one fp32
    rounding of the reference lies inside them."""
    g = np.random.default_rng(5)
    P = 257
    w, s1, s2 = (0.1 + 0.05 * g.standard_normal(P)).astype(F), (0.1 + g.random(P)).astype(F), g.random(P).astype(F)
    mask = g.choice(np.array([0.0, 1.0, 0.5, 2.0], F), P)
    grad = g.standard_normal(P).astype(F)
    for kind in (0, 1, 2):
        w2, a, b, bw, b1, b2 = fr.optim_ref(kind, w, mask, s1, s2, grad, 3, 0.37)
        dead = mask == 0
        assert np.array_equal(w2[dead], w[dead].astype(np.float64)) and np.array_equal(a[dead], s1[dead])
        assert (bw[~dead] > 0).all() and (np.abs(w2.astype(F) - w2) <= bw)[~dead].all()
        assert (w2 != w)[~dead].any() and bw.max() < 1e-6
