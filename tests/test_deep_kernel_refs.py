"""The references of tests/deep_kernel_refs.py would notice a wrong kernel (CPU only).

Each check applies one mutation to the expected values or to the index map, stores the mutated result the
way the kernel would (fp32 / bf16), and runs the comparison tests/test_gpu_deep_kernels.py uses on the GPU
over the committed case lists: it must fail on at least one case.  The exact cases' patterns are checked for
degeneracy (a pattern whose column sums are all equal lets columns trade places unseen), and the
assumptions the GPU tests make about the mirrors (exactness in bf16, three different action patterns) are
checked here, where a failure costs no GPU time.  Every mutation prints its err/bound or its count of
differing entries."""
import numpy as np
import pytest

import deep_kernel_refs as R

U, F = R.U, np.float32


def _stored(ref):
    """A float64 result as the kernel would store it in bf16."""
    return R.bf16_bits(np.asarray(ref, np.float64).astype(F)).reshape(np.shape(ref))


def _replay_cases():
    for cap, size in R.RINGS:
        for step in R.SAMPLE_STEPS:
            for H, in_p in ((5, 8), (201, 204)):
                T, E = H + 4, 3
                prices = R.price_bank(E, T, seed=H)
                ring = R.make_ring(cap, size, E, T, H, seed=100 * cap + size + H)
                for fm in (0, 1):
                    for B in (1, 5, 67):
                        yield dict(ring=ring, prices=prices, T=T, H=H, in_p=in_p, feat_mode=fm, inv_b0=R.INV_B0, B=B,
                                   step=step, size=size), cap


def _replay_mismatch(case, **mut) -> int:
    """Entries at which the GPU test's comparisons fail when the kernel computes the mutated sample."""
    ref, got = R.replay_sample_ref(**case), R.replay_sample_ref(**case, **mut)
    bad = int((got["a"] != ref["a"]).sum())
    for key in ("r", "done"):
        bad += int((got[key].view(np.uint32) != ref[key].view(np.uint32)).sum())
    for key in ("X", "Xn"):
        stored = _stored(got[key][0])
        if case["feat_mode"]:
            bad += int((~R.interval_ok(stored, *ref[key])).sum())
        else:
            bad += int((stored != _stored(ref[key][0])).sum())
    return bad


# ----------------------------------------------------------------------------- bf16 helpers
def test_bf16_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-3, 255.5, 0.0], F)   # ties to even, both ways
    import torch

    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    assert np.array_equal(R.bf16_round64(x.astype(np.float64)), R.bf16_val(want))
    g = np.random.default_rng(0)
    y = g.standard_normal(4096) * 10.0 ** g.integers(-3, 4, 4096)
    assert np.array_equal(R.bf16_round64(y), R.bf16_val(R.bf16_bits(R.bf16_round64(y).astype(F))))   # bf16 values
    assert (np.abs(R.bf16_round64(y) - y) <= np.abs(y) * 2.0 ** -8).all()
    # a value next to a rounding boundary neither hides an error nor fails wrongly
    ref, d = 1.00390625 - 1e-9, 4 * U
    assert R.interval_ok(R.bf16_bits(np.array([1.0], F)), ref, d) and R.interval_ok(R.bf16_bits(np.array([1.0078125], F)), ref, d)
    assert not R.interval_ok(R.bf16_bits(np.array([1.015625], F)), ref, d)


# ----------------------------------------------------------------------------- gather
def test_gather_mutations_are_caught():
    cases = list(_replay_cases())
    assert all(_replay_mismatch(c) == 0 for c, _ in cases)
    for name, mut, only in (("x' window not shifted", dict(shift=False), None),
                            ("x' normalised by last", dict(new_norm=False), 1)):
        n = [_replay_mismatch(c, **mut) for c, _ in cases if only is None or c["feat_mode"] == only]
        print(f"[mutation] gather, {name}: differing entries per case min {min(n)} max {max(n)}")
        assert min(n) > 0
    n = {(cap, c["size"]): _replay_mismatch(c, mod=cap) for c, cap in cases if c["B"] == 67}
    print(f"[mutation] gather, index % cap: differing entries by ring {n}")
    assert n[(7, 1)] > 0 and n[(7, 5)] > 0 and n[(64, 64)] == 0
    for step in R.SAMPLE_STEPS:
        n = sum(_replay_mismatch(c, hi_word=False) for c, _ in cases if c["step"] == step and c["size"] > 1)
        print(f"[mutation] gather, counter high word dropped, step {step}: {n} differing entries")
        assert (n > 0) == (step >> 32 != 0)


def test_gather_env_cases_reach_the_bank_end():
    for H, in_p in R.GATHER_SHAPES:
        for B in R.GATHER_B:
            c = R.gather_env_case(H, B, seed=1000 * H + B)
            assert c["pos"].min() == 0 or B == 1
            assert c["pos"][B - 1] == c["T"] - H - 1 and (B - 1) * c["T"] + c["pos"][B - 1] + H == B * c["T"] - 1
            assert c["pos"].max() + H < c["T"] and H + 2 <= in_p <= 256


# ----------------------------------------------------------------------------- env step
def _env_run(E, case, **mut):
    c = R.env_case(E, case)
    st, q, ring = R.env_state(E, seed=10 * E + case), R.env_q(E, c["ldq"], seed=E + case), R.env_ring0(c["cap"])
    cursor, step, out, infos = c["cursor"], c["step0"], [], []
    for _ in range(3):
        st, ring, info = R.env_mirror(c, st, ring, q, cursor, step, **mut)
        out.append(b"".join(st[k].tobytes() for k in ("budget", "shares", "value", "pos", "episodes", "last_final")) +
                   b"".join(ring[k].tobytes() for k in R.RING_KEYS))
        infos.append(info)
        cursor, step = cursor + E, step + 1
    return c, out, infos


def test_env_cases_cover_their_edges():
    seen = set()
    for E in R.ENV_E:
        for case in range(6):
            c, _, infos = _env_run(E, case)
            seen.add((case % 3, c["compat"], c["eps"]))
            # the second launch wraps inside its E slots (E = 1 has one slot per launch)
            start = (c["cursor"] + E) % c["cap"]
            assert E == 1 or start + E > c["cap"], (E, case)
            assert len({i["u1"].tobytes() + i["u2"].tobytes() for i in infos}) == 3
            if E >= 63 and c["eps"] < 1.0:
                assert len({i["a"].tobytes() for i in infos}) == 3, (E, case)
            st = R.env_state(E, seed=10 * E + case)
            if E >= 63:
                price = st["prices"][np.arange(E), st["pos"] + c["H"]]
                assert (st["budget"] < price).any() and (st["shares"] == 0).any()
                assert (st["pos"] == c["T"] - c["H"] - 1).sum() > 1
                assert any(i["done"].any() for i in infos) and not all(i["done"].all() for i in infos)
                a0 = infos[0]
                assert a0["explore"].any() or c["eps"] == 1.0
            assert c["step0"] + 3 < 2 ** 63
    assert len({x[:2] for x in seen}) == 6 and len({x[1:] for x in seen}) == 6   # every cap and every eps with both compat_env
    # the Q rows hold ties, and the first maximum is not the last one there
    q = R.env_q(64, 3, 0)
    assert ((q[:, 0] == q[:, 1]) & (q[:, 0] >= q[:, 2])).any() and ((q[:, 1] == q[:, 2]) & (q[:, 1] > q[:, 0])).any()


@pytest.mark.parametrize("name,mut", [("slot without the wrap", dict(wrap=False)), ("done at np > T - H", dict(done_gt=True)),
                                      ("compat_env ignored", dict(use_compat=False)),
                                      ("ties to the last maximum", dict(last_max=True))])
def test_env_mutations_are_caught(name, mut):
    caught = 0
    for E in R.ENV_E:
        for case in range(6):
            _, good, _ = _env_run(E, case)
            _, bad, _ = _env_run(E, case, **mut)
            caught += good != bad
    print(f"[mutation] env step, {name}: {caught} of {6 * len(R.ENV_E)} cases differ")
    assert caught > 0


# ----------------------------------------------------------------------------- TD / head
def test_td_exact_case_is_exact():
    for B in R.TD_B:
        for ldq, nact in R.TD_LD:
            inp = R.td_inputs(B, ldq, nact, True, seed=1000 * B + 10 * ldq + nact)
            dq, _, diff = R.td_ref(inp["q"], inp["qt"], inp["r"], inp["a"], inp["done"], nact, R.GAMMA_X, R.COEF_X)
            assert np.array_equal(R.bf16_round64(dq), dq) and (np.abs(diff * 4) <= 20).all()
            assert set(inp["done"].tolist()) == ({0.0, 1.0} if B > 1 else {0.0})
            loss = 3.5 + (diff * diff).sum()
            assert float(F(loss)) == loss


def _head_setup(B, H, nact, exact, seed=7):
    ldq = 4
    inp = R.td_inputs(B, ldq, nact, exact, seed)
    A, W = R.head_inputs(B, H, nact, exact, seed + 1)
    gamma, coef = (R.GAMMA_X, R.COEF_X) if exact else (R.GAMMA_R, R.COEF_R)
    dq, _, _ = R.td_ref(inp["q"], inp["qt"], inp["r"], inp["a"], inp["done"], nact, gamma, coef)
    return A, W, inp["a"], R.bf16_round64(dq)


def test_head_exact_case_is_exact_and_not_degenerate():
    for B, H in R.HEAD_SHAPES:
        for nact in (1, 3, 4):
            A, W, a, gv = _head_setup(B, H, nact, True)
            Gb, dW, _, gp, _, seen = R.head_ref(A, W, a, gv, nact)
            assert sorted(seen) == [(y, x) for y in range(B // 64) for x in range(H // 256)]      # the map is a bijection
            live = A > 0
            assert (live.sum(0) > 0).any() and ((A == 0) & np.signbit(A)).any() and ((A == 0) & ~np.signbit(A)).any()
            prod = gv[:, None] * np.nan_to_num(W)[a]
            assert np.array_equal(R.bf16_round64(prod), prod)                       # g W exact in bf16
            start = (((np.arange(H)[None, :] + 3 * np.arange(4)[:, None]) % 9 - 4) / 32.0)
            tot = start[:nact] + dW[:nact]
            assert np.array_equal(tot.astype(F).astype(np.float64), tot) and np.abs(tot).max() * 32 < 2 ** 24
            assert np.array_equal(gp.astype(F).astype(np.float64), gp)
            # distinct columns get distinct sums (most of them: the values are small integers)
            for k in range(nact):
                assert len(set(dW[k].tolist())) > H // 8, (B, H, nact, k)
            assert len(set(gp[0].tolist())) > H // 16
            # with qp: the exact parts' sums stay exact as well
            for nqp in R.HEAD_NQP:
                qp, qpt, bq, bqt = R.qparts(nqp, B, nact, True, 3)
                q, qt = R.qparts_sum(qp, bq, nact).astype(np.float64), R.qparts_sum(qpt, bqt, nact).astype(np.float64)
                assert (np.abs(q * 4) <= 21).all() and (np.abs(qt * 2) <= 20).all() and (q * 4 == np.rint(q * 4)).all()
                assert len(set(q[:, 0].tolist())) > 1


def _head_compare(B, H, nact, exact, **mut):
    """(G entries differing, dW err/bound, gpart rows differing) of a mutated head against the true one."""
    A, W, a, gv = _head_setup(B, H, nact, exact)
    Gb, dW, dWa, gp, gpa, _ = R.head_ref(A, W, a, gv, nact)
    Gm, dWm, _, gpm, _, _ = R.head_ref(A, W, a, gv, nact, **mut)
    bound = (B + 8) * U * dWa[:nact]
    err = np.abs(dWm[:nact].astype(F).astype(np.float64) - dW[:nact])
    rows = int((~(np.abs(np.nan_to_num(gpm, nan=1e30) - gp) <= 72 * U * gpa)).any(1).sum())
    return int((Gm != Gb).sum()), R.ratio(err, bound) if not exact else float((dWm[:nact] != dW[:nact]).sum()), rows


def test_head_mutations_are_caught():
    B, H = 512, 512
    assert [R.head_map(B, H, L) for L in range(16)] != [R.head_map_rowmajor(B, H, L) for L in range(16)]
    # replacing one bijective map by another is no defect: the outputs are the same, as they must be
    assert _head_compare(B, H, 3, True, block_map=R.head_map_rowmajor) == (0, 0.0, 0)
    # a map that takes the row block from one and the column block from the other leaves blocks out
    g, w, r = _head_compare(B, H, 3, True, block_map=R.head_map_half)
    print(f"[mutation] head, half of the XCD map replaced at (512, 512): {g} G entries, {int(w)} dW entries, {r} gpart rows differ")
    assert g > 0 and w > 0 and r > 0
    for B, H in R.HEAD_SHAPES:
        g, _, _ = _head_compare(B, H, 3, True, swap_pieces=True)
        print(f"[mutation] head, two 8-column pieces swapped at ({B}, {H}): {g} G entries differ")
        assert g > 0
        _, w, _ = _head_compare(B, H, 3, True, drop_block=B // 64 - 1)
        _, rw, _ = _head_compare(B, H, 3, False, drop_block=B // 64 - 1)
        print(f"[mutation] head, last row block dropped from dW at ({B}, {H}): {int(w)} exact entries differ, random err/bound {rw:.3g}")
        assert w > 0 and rw > 1


# ----------------------------------------------------------------------------- qhead
@pytest.mark.parametrize("H", [136, 1016])
def test_qhead_dropped_unit_is_caught(H):
    for exact in (True, False):
        A, W, bias = R.qhead_inputs(16, H, H + 8, H + 8, 3, exact, seed=H)
        ref, bound = R.qhead_ref(A, W, bias, H, 3)
        bad, _ = R.qhead_ref(A, W, bias, H, 3, drop_last_unit=True)
        if exact:
            assert np.array_equal(ref.astype(F).astype(np.float64), ref) and np.abs(A[:, :H]).sum(1).max() * 8 < 2 ** 24
            n = int((bad.astype(F) != ref.astype(F)).sum())
            print(f"[mutation] qhead, last 16-byte unit dropped at H={H}: {n} of {ref.size} exact entries differ")
            assert n > ref.size // 2
            assert len(set(ref[:, 0].tolist())) > 8      # rows get distinct sums
        else:
            rt = R.ratio(np.abs(bad.astype(F).astype(np.float64) - ref), bound)
            print(f"[mutation] qhead, last 16-byte unit dropped at H={H}: random err/bound {rt:.3g}")
            assert rt > 1


# ----------------------------------------------------------------------------- row sum, bias gradients
def test_exact_sum_patterns_are_not_degenerate():
    for n in R.ROWSUM_N:
        x = R.rowsum_inputs(3, n, True, 0).astype(np.float64)
        assert np.array_equal(R.bf16_round64(x), x)
        assert len(set(x.sum(1).tolist())) == 3                  # rows differ
        assert n < 61 or len(set(x[0, :61].tolist())) == 61      # columns differ
    for I, nb in R.ADAM_GT:
        x = R.gt_inputs(I, nb, nb + 8, True, 0)[:, :nb].astype(np.float64)
        assert np.array_equal(R.bf16_round64(x), x) and np.isnan(R.gt_inputs(I, nb, nb + 8, True, 0)[:, nb:]).all()
        assert I == 1 or len(set(x.sum(1).tolist())) > 1
        assert len(set(x[0, :8].tolist())) == 8                  # the 8 elements of a 16-byte unit differ
    for npart in R.ADAM_GP:
        for I in (1, 33, 70, 32, 5):
            x = R.gp_inputs(npart, I, I + 4, True, 0)[:, :I].astype(np.float64)
            assert I == 1 or len(set(x.sum(0).tolist())) > 1


# ----------------------------------------------------------------------------- Adam
def _adam_worst(t, got):
    st = R.adam_state(4096, seed=t)
    ref = R.adam_ref(st["w"], st["g"], st["m"], st["v"], st["mask"], t)
    out = got(st)
    return max(R.ratio(np.abs(np.asarray(out[i]).astype(F).astype(np.float64) - ref[i]), ref[3 + i]) for i in range(3))


def test_adam_reference_is_self_consistent():
    """The true update, stored as fp32, passes its own bounds; masked elements stay; m and g share a sign."""
    for t in R.ADAM_T:
        st = R.adam_state(4096, seed=t)
        assert set(st["mask"].tolist()) == {0.0, 0.5, 1.0} and (st["m"] * st["g"] >= 0).all()
        assert _adam_worst(t, lambda s: R.adam_ref(s["w"], s["g"], s["m"], s["v"], s["mask"], t)) < 1
        w1, m1, v1, bw, _, _ = R.adam_ref(st["w"], st["g"], st["m"], st["v"], st["mask"], t)
        keep = st["mask"] == 0
        assert np.array_equal(w1[keep], st["w"][keep].astype(np.float64)) and (bw[keep] == 0).all()
        assert (np.abs(w1 - st["w"])[~keep] > 100 * bw[~keep]).all()      # the bound is far below the update itself


def test_adam_mutations_are_caught():
    for t in R.ADAM_T:
        r1 = _adam_worst(t, lambda s: R.adam_ref(s["w"], s["g"], s["m"], s["v"], s["mask"], t + 1))
        r2 = _adam_worst(t, lambda s: R.adam_ref(s["w"], s["g"], s["m"], s["v"], s["mask"], t, b1=R.B2, b2=R.B1))
        r3 = _adam_worst(t, lambda s: R.adam_ref(s["w"], s["g"], s["m"], s["v"], s["mask"], t, stale_m=True))
        print(f"[mutation] Adam at t={t}: t + 1 err/bound {r1:.3g}; betas swapped {r2:.3g}; m read after its write {r3:.3g}")
        assert r1 > 1 and r2 > 1 and r3 > 1
    # t + 1 at t = 1 is the case the old t = 1 formula check could not see
    assert _adam_worst(1, lambda s: R.adam_ref(s["w"], s["g"], s["m"], s["v"], s["mask"], 2)) > 100
