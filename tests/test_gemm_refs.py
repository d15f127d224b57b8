"""The references of tests/gemm_refs.py would notice a wrong GEMM kernel (CPU only).

As tests/test_gru_learn_refs.py does for the GRU learner: a numpy model of the kernels' tiling (block origin m0 / n0,
the waves' rows and columns, K-tiles and split ranges, the xcd_remap and grouped tile-order maps) must equal the
float64 reference on every committed case through the very ``check_*`` functions tests/test_gpu_gemm_refs.py uses,
and each mutation of the model must make them report more than 0 on at least one case.  The exactness precondition
of the integer operands is asserted for every case, and the two index maps are checked for being bijections."""
import numpy as np
import pytest

import gemm_refs as R

CASES = R.exact_cases()
GAUSS = [c for t in R.TILES for c in R.gauss_cases(t)]


def _any(c, f):
    return any(f(p) for p in c["probs"])


def _total(c, gots, refs):
    return sum(sum(R.check_problem(g, r).values()) for g, r in zip(gots, refs))


def test_case_names_are_unique_and_cover_every_tile():
    names = [c["name"] for c in CASES + GAUSS]
    assert len(set(names)) == len(names)
    assert {c["tile"] for c in CASES} == set(R.TILES) == {c["tile"] for c in GAUSS}
    # every gemm_body tile meets every epilogue, split-K 2 and 4 with one K-tile per split among them
    for t in R.BODY_TILES:
        mine = [p for c in CASES if c["tile"] == t and c["kind"] == "nt" for p in c["probs"]]
        assert {p["epi"] for p in mine} == {R.EPI_BF16, R.EPI_RELU_GRAD, R.EPI_F32}
        assert {(p["K"] // 64, p["splitk"]) for p in mine if p["splitk"] > 1} >= {(2, 2), (4, 2), (4, 4)}
        assert {p["nq"] for p in mine} == {0, 1, 2, 3, 4}
        kts = {p["K"] // 64 for p in mine if p["splitk"] == 1}
        S = R.TILES[t].S
        assert kts >= {1, 2, 3, 5, 7} and (S == 2 or kts >= {1, S - 2, S - 1, S, S + 1})
    for t in R.BIG_TILES:
        mine = [p for c in CASES if c["tile"] == t for p in c["probs"]]
        assert {p["K"] // 64 for p in mine} == {1, 2, 3, 6, 7}
        assert {(p["M"] // 256, p["N"] // 256) for p in mine if p["K"] == 64} >= {(1, 1), (3, 5), (9, 2), (10, 2)}
    # grouped launches: remainders 1, 3, 4, 7 of the workgroup count mod 8, 4 problems of different shapes each
    assert {R.blocks(c) % 8 for c in R.BATCHED_CASES} >= {1, 3, 4, 7}
    for c in R.BATCHED_CASES:
        assert len(c["probs"]) == 4 and len({(p["M"], p["N"], p["K"]) for p in c["probs"]}) == 4
    assert {tuple(p["epi"] for p in c["probs"]) for c in R.DUAL_CASES} == {(1, 2), (2, 2), (0, 2)}


def test_cases_have_several_tiles_each_way():
    """At least 2 tiles along M and along N with M != N, unless the problem is named as a small one."""
    for c in CASES + GAUSS:
        g = R.TILES[c["tile"]]
        for p in c["probs"]:
            assert p["M"] % g.BM == 0 and p["N"] % g.BN == 0 and p["K"] % R.GBK == 0 and p["K"] <= 4096, c["name"]
            if not p["small"]:
                assert p["M"] // g.BM >= 2 and p["N"] // g.BN >= 2 and p["M"] != p["N"], c["name"]
    assert all(not p["small"] for c in CASES if c["kind"] == "nt" and "-g1x1" not in c["name"] for p in c["probs"])


def test_index_maps_are_bijections():
    counts = sorted({R.blocks(c) for c in CASES + GAUSS})
    assert {n % 8 for n in counts} >= {0, 1, 3, 4, 7}
    for n in counts:
        assert sorted(R.xcd_remap(b, n) for b in range(n)) == list(range(n)), n
        if n % 8 and n > 1:
            assert sorted(R.xcd_remap(b, n, remainder=False) for b in range(n)) != list(range(n)), n
    grids = {(p["M"] // 256, p["N"] // 256) for c in CASES if c["tile"] in (7, 8) for p in c["probs"]}
    assert grids >= {(1, 1), (3, 5), (9, 2), (10, 2)}
    for ntm, ntn in sorted(grids):
        want = sorted((a, b) for a in range(ntm) for b in range(ntn))
        assert sorted(R.pp_tile(i, ntm, ntn) for i in range(ntm * ntn)) == want, (ntm, ntn)
        if ntm % 8 and ntm * ntn > 1:
            assert sorted(R.pp_tile(i, ntm, ntn, ragged=False) for i in range(ntm * ntn)) != want, (ntm, ntn)


def test_bf16_rne_pins_ties_to_even():
    x = np.array([257.0, 259.0, 258.0, 514.0, 518.0, 1.00390625, 1.01171875, -257.0, 0.0, 2.0 ** -133, 2.0 ** -134])
    want = np.array([256.0, 260.0, 258.0, 512.0, 520.0, 1.0, 1.015625, -256.0, 0.0, 2.0 ** -133, 0.0])
    assert np.array_equal(R.bf16_val(R.bf16_rne(x)), want)
    assert np.array_equal(R.bf16_val(R.bf16_trunc(np.array([259.0, -259.0, 511.0]))), [258.0, -258.0, 510.0])
    bits = np.arange(0x7F80, dtype=np.uint16)                 # every non-negative finite bf16 round-trips
    assert np.array_equal(R.bf16_rne(R.bf16_val(bits)), bits)
    assert R.check_bf16(np.array([0x8000], np.uint16), np.array([0], np.uint16)) == 0
    assert R.check_bf16(np.array([0x7FC0], np.uint16), np.array([0], np.uint16)) == 1
    assert R.check_f32(np.array([-0.0, np.nan], np.float32), np.array([0.0, 1.0])) == 1


def test_exactness_precondition_and_real_rounding():
    """Every exact case satisfies the precondition; the bf16 outputs really round (ties included) and the masks
    really hold every special value."""
    ties = rounded = 0
    for c in CASES:
        g = R.TILES[c["tile"]]
        inputs = R.case_inputs(c)
        for p, inp, r in zip(c["probs"], inputs, R.case_refs(c, inputs)):
            assert not p["gauss"]
            R.assert_exact(p, inp, g)
            for k, v in r.items():
                assert not np.isnan(R.bf16_val(v) if v.dtype == np.uint16 else v).any(), (c["name"], k)
            if p["epi"] == R.EPI_BF16:
                x = r["x"]
                rounded += int((R.bf16_val(r["out"]) != x).sum())
                ax = np.abs(x)
                ties += int((((ax > 256) & (ax < 512) & (ax % 2 == 1)) | ((ax > 512) & (ax < 1024) & (ax % 4 == 2))).sum())
            if p["epi"] == R.EPI_RELU_GRAD:
                assert set(np.unique(inp["act"])) == set(R.ACT_PALETTE.tolist())
                for (m, n), b in R.ACT_KNOWN.items():
                    assert inp["act"][m, n] == b and bool(r["out"][m, n] & 0x7FFF) <= (b in (0x0001, 0x7F80, 0x3F80))
            if p["nq"]:
                assert not r["qpart"][:, :, p["nq"]:].any() and r["qpart"][:, :, :p["nq"]].any()
    print(f"[exact] {len(CASES)} cases: {rounded} bf16 outputs are not their own pre-rounding value, {ties} exact ties")
    assert rounded > 10000 and ties > 1000


def test_model_equals_reference_on_every_case():
    for c in CASES:
        inputs = R.case_inputs(c)
        refs = R.case_refs(c, inputs)
        n = [R.check_problem(g, r) for g, r in zip(R.model_launch(c, inputs), refs)]
        assert all(v == 0 for d in n for v in d.values()), (c["name"], n)
        for p, d in zip(c["probs"], n):
            assert set(d) == {"out"} | {k for k, on in (("outT", p["outT"]), ("colpart", p["colpart"]),
                                                        ("qpart", p["nq"])) if on}


APPLIES = {
    "drop_last_ktile": lambda c: True,
    "swap_kchunks": lambda c: True,
    "bias_local": lambda c: _any(c, lambda p: p["bias"]),
    "alpha_after_bias": lambda c: _any(c, lambda p: p["bias"] and p["alpha"] != 1.0),
    "bias_every_split": lambda c: _any(c, lambda p: p["bias"] and p["splitk"] > 1),
    "accumulate_ignores_prior": lambda c: _any(c, lambda p: p["accumulate"]),
    "bf16_trunc": lambda c: _any(c, lambda p: p["epi"] != R.EPI_F32),
    "mask_ge": lambda c: _any(c, lambda p: p["epi"] == R.EPI_RELU_GRAD),
    "mask_untransposed": lambda c: _any(c, lambda p: p["epi"] == R.EPI_RELU_GRAD),
    "outT_in_tile": lambda c: _any(c, lambda p: p["outT"]),
    "colpart_unrounded": lambda c: _any(c, lambda p: p["colpart"]),
    "colpart_row": lambda c: _any(c, lambda p: p["colpart"]),
    "qpart_unrounded": lambda c: _any(c, lambda p: p["nq"]),
    "qpart_part": lambda c: _any(c, lambda p: p["nq"]),
    "qpart_col_nq": lambda c: _any(c, lambda p: 0 < p["nq"] < 4),
    "batch_bias0": lambda c: c["kind"] == "batched" and c["probs"][0]["bias"] and c["probs"][1]["bias"],
    "pp_gm8": lambda c: c["tile"] in (7, 8),
    "xcd_no_remainder": lambda c: R.blocks(c) % 8 != 0,
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutation_is_caught(mut):
    """One mutation of the model, over an evenly spread subset (fewer than 48) of the cases it applies to: the GPU test's own
    comparison reports it.  Prints differing entries and how many of the cases noticed."""
    cases = [c for c in CASES if APPLIES[mut](c)]
    assert cases, mut
    cases = cases[::max(1, len(cases) // 24)]
    counts = []
    for c in cases:
        inputs = R.case_inputs(c)
        counts.append(_total(c, R.model_launch(c, inputs, mut), R.case_refs(c, inputs)))
    print(f"[mutation] {mut}: {sum(counts)} differing entries, caught by {sum(n > 0 for n in counts)} of "
          f"{len(counts)} cases")
    assert max(counts) > 0


def test_gauss_check_accepts_fp32_sums_and_refuses_a_dropped_term():
    """The Gaussian bound: an fp32 left-to-right sum lies inside it, a result with one k-term dropped does not."""
    for c in GAUSS[:4]:
        (p,), (inp,) = c["probs"], R.case_inputs(c)
        (ref,) = R.case_refs(c, [inp])
        bound = R.gauss_bound(p, inp)
        A, B = R.bf16_val(inp["A"]).astype(np.float32), R.bf16_val(inp["B"]).astype(np.float32)
        acc = np.zeros((p["M"], p["N"]), np.float32)
        for k in range(p["K"]):
            acc += A[:, k:k + 1] * B[None, :, k]
        for drop in (False, True):
            a = acc - (A[:, :1] * B[None, :, 0] if drop else 0)
            v = np.float32(p["alpha"]) * a + inp["bias"].astype(np.float32)[None, :]
            got = {"out": v if p["epi"] == R.EPI_F32 else R.bf16_rne(v.astype(np.float64))}
            bad, ratio = R.check_gauss(p, got, ref, bound)
            print(f"[gauss] {c['name']} {'one k-term dropped' if drop else 'fp32 sum'}: outside {bad}, err/bound {ratio:.3g}")
            assert (bad > 0 and ratio > 1) if drop else (bad == 0 and ratio <= 1)
