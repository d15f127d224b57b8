"""The kernels of the batched exact-fp32 step (csrc/mlp_f32_mfma.hip) and the mode-2 optimizer pass
(csrc/mlp_f32.hip), one entry point at a time, against the float64 references of tests/f32b_refs.py.

The ``st_f32b_*`` entry points and ``st_f32_grad_optim`` are called through the ctypes mirrors of
sharetrade/ops/mlp_f32.py, not through the engine.  Every operand and output is a (strided) region inside a NaN-filled
guard band (tests/guard_band.py): after each launch the guards and row gaps are bit-unchanged, every in-range output
is written (a left-over NaN differs from the reference), the inputs are unchanged; a refused launch returns
hipErrorInvalidValue and leaves every buffer bit-unchanged.  Exact cases are compared bit for bit, Gaussian cases per
element within the bounds derived in tests/f32b_refs.py; the scalar env / TD rule is bit-equal on every case."""
import ctypes as C

import numpy as np
import pytest
import torch

import f32b_refs as fr
from f32b_refs import F
from guard_band import Band

pytestmark = pytest.mark.gpu

INVALID = 1   # hipErrorInvalidValue
NAN = float("nan")
# Adam goes through powf, whose device error is measured, not assumed: the largest |w' - ref64| over the Adam cases
# below, in units of B_adam (the derived bound of every other operation, tests/f32b_refs.py), was measured on an
# MI355X (profiles/f32b_refs.md): 3.53 (SGD and AdaGrad, which have no powf, reach 0.92 of their own bounds).  The test
# asserts 4 x that, 14.12, because powf's error varies with t and beta and the test samples few values of them.
ADAM_MEASURED = 3.53
ADAM_MARGIN = 4.0


@pytest.fixture(scope="module")
def lib(native_built):
    from sharetrade.ops import mlp_f32

    L = mlp_f32._bind_batched()
    return L, native_built, mlp_f32


def fband(flat, guard=NAN):
    flat = np.ascontiguousarray(flat, dtype=F)
    return Band(flat.size, torch.float32, guard).set(torch.from_numpy(flat.copy()))


def iband(v, dtype=torch.int32, guard=0x5A5A5A5):
    t = torch.as_tensor(np.ascontiguousarray(v)).to(dtype)
    return Band(t.numel(), dtype, guard).set(t)


def np_of(b: Band):
    return b.cpu().numpy()


def intact(bands, snaps, written=()):
    """Guards of everything intact; everything outside ``written`` bit-unchanged."""
    for k, b in bands.items():
        assert b.guards_intact(), f"{k}: write outside its region"
        if k not in written:
            assert b.same(snaps[k]), f"{k} changed"


def snap_all(bands):
    return {k: b.snap() for k, b in bands.items()}


# ----------------------------------------------------------------------------- st_f32b_gemm
def _gemm_setup(mlp, c):
    bands = dict(A=fband(c.A.flat), B=fband(c.B.flat), C=fband(c.C.flat))
    if c.bias is not None:
        bands["bias"] = fband(c.bias)
    if c.aux is not None:
        bands["aux"] = fband(c.aux.flat)
    g = mlp.GemmF32()
    g.A, g.B, g.C = bands["A"].ptr() + 4 * c.A.off, bands["B"].ptr() + 4 * c.B.off, bands["C"].ptr() + 4 * c.C.off
    g.bias = bands["bias"].ptr() if c.bias is not None else None
    g.aux = bands["aux"].ptr() + 4 * c.aux.off if c.aux is not None else None
    g.M, g.N, g.K = c.M, c.N, c.K
    g.am, g.ak, g.bn, g.bk, g.ldc = c.A.sr, c.A.sc, c.B.sr, c.B.sc, c.C.sr
    g.ldaux = c.aux.sr if c.aux is not None else 0
    g.epi, g.relu, g.kchunk, g.zstride = c.epi, int(c.relu), 0, c.zstride
    return g, bands


def _run_gemm(lib, c):
    L, native, mlp = lib
    g, bands = _gemm_setup(mlp, c)
    # the loader pair this launch selects, by the launcher's rule on the real pointers: the one the case is listed for
    assert (fr.ld_mode(g.A, g.am, g.ak), fr.ld_mode(g.B, g.bn, g.bk)) == (c.am, c.bm), c.name
    snaps = snap_all(bands)
    rc = L.st_f32b_gemm(C.byref(g), c.splits, native.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0, (c.name, rc)
    intact(bands, snaps, written=("C",))
    got = np_of(bands["C"])
    d, ratio = fr.check_gemm(c, got)
    assert d == 0, (c.name, d, ratio)
    if c.epi == fr.F32B_PARTIAL:
        # the partial tiles the kernel wrote = the count the Python side computes (F32BatchedStep.grad)
        kchunk = -(-(-(-c.K // c.splits)) // 32) * 32
        tiles = got[:c.splits * c.zstride] if got.size >= c.splits * c.zstride else np.r_[
            got, np.full(c.splits * c.zstride - got.size, np.nan, F)]
        wrote = [z for z in range(c.splits) if not np.isnan(tiles[z * c.zstride:(z + 1) * c.zstride]).all()]
        assert wrote == list(range(-(-c.K // kchunk))), (c.name, wrote)
    return ratio, bands


@pytest.mark.parametrize("am", range(3), ids=fr.LD_NAMES)
@pytest.mark.parametrize("bm", range(3), ids=fr.LD_NAMES)
def test_gemm_loader_pair(lib, am, bm):
    """Every committed GEMM case of one (A loader, B loader) pair: all four epilogues, every K, the row / column / k /
    float4 tails, split-K counts 1, 2, 3, 5 (and K = 40 with 3 requested, where 2 run); exact cases bit for bit
    (signed zeros included), the Gaussian case within gamma(K + c) sum |terms| + u |ref| per element."""
    cases = [c for c in fr.gemm_cases() if (c.am, c.bm) == (am, bm)]
    assert {c.epi for c in cases if c.exact} == {0, 1, 2, 3} and any(not c.exact for c in cases)
    for c in cases:
        ratio, _ = _run_gemm(lib, c)
        if not c.exact:
            print(f"[meas] gemm {c.name}: max err/bound = {ratio:.4f}")


def test_gemm_partial_splitsum_equals_atomic(lib):
    """PARTIAL tiles added by st_f32b_splitsum equal the ATOMIC result on a zeroed C, bit for bit (dense C)."""
    L, native, mlp = lib
    for M, N, K, sp, am, bm, seed in fr.small_split_cases():
        p = fr.make_gemm("p", M, N, K, am, bm, fr.F32B_PARTIAL, sp, seed=seed, dense=True)
        a = fr.make_gemm("a", M, N, K, am, bm, fr.F32B_ATOMIC, sp, seed=seed, dense=True)
        a.C.put(np.zeros((M, N)))
        _, pb = _run_gemm(lib, p)
        _, ab = _run_gemm(lib, a)
        _, nz = fr.split_rule(K, sp)
        out = fband(np.full(M * N, np.nan, F))
        assert L.st_f32b_splitsum(pb["C"].ptr(), nz, p.zstride, out.ptr(), M * N, native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert out.guards_intact()
        assert fr.check_bits(np_of(out), np_of(ab["C"])[:M * N]) == 0, (M, N, K, sp)


def test_gemm_refusals(lib):
    L, native, mlp = lib
    base = dict(M=65, N=67, K=40, am=fr.LD_KF, bm=fr.LD_KF)

    def refused(epi, splits, written=(), **edit):
        c = fr.make_gemm("r", base["M"], base["N"], base["K"], base["am"], base["bm"], epi, max(splits, 1), seed=3)
        g, bands = _gemm_setup(mlp, c)
        for k, v in edit.items():
            setattr(g, k, v)
        snaps = snap_all(bands)
        rc = L.st_f32b_gemm(C.byref(g), splits, native.stream_handle())
        torch.cuda.synchronize()
        intact(bands, snaps, written)
        return rc

    for dim in ("M", "N", "K"):
        for v in (0, -1):
            assert refused(fr.F32B_STORE, 1, **{dim: v}) == INVALID, (dim, v)
    for epi in range(4):
        assert refused(epi, 0) == INVALID and refused(epi, -2) == INVALID
    assert refused(fr.F32B_STORE, 2) == INVALID and refused(fr.F32B_MASK, 2) == INVALID
    c = fr.make_gemm("r", 65, 67, 40, 0, 0, fr.F32B_PARTIAL, 2, seed=3)
    assert refused(fr.F32B_PARTIAL, 2, zstride=65 * c.C.sr - 1) == INVALID
    assert refused(fr.F32B_PARTIAL, 2, written=("C",)) == 0   # the same buffers with valid arguments run


# ----------------------------------------------------------------------------- st_f32b_fwd2
def _fwd2_setup(mlp, c):
    bands = dict(A=fband(c.A.flat), W1=fband(c.W1.reshape(-1)), W2=fband(c.W2.reshape(-1)),
                 H=fband(np.full(c.M * c.N1, np.nan, F)), Q=fband(np.full(c.M * 16, np.nan, F)))
    if c.b1 is not None:
        bands["b1"] = fband(c.b1)
    if c.b2 is not None:
        bands["b2"] = fband(c.b2)
    f = mlp.Fwd2F32()
    f.A, f.W1, f.W2, f.H, f.Q = (bands[k].ptr() for k in ("A", "W1", "W2", "H", "Q"))
    f.b1 = bands["b1"].ptr() if c.b1 is not None else None
    f.b2 = bands["b2"].ptr() if c.b2 is not None else None
    f.M, f.K, f.N1, f.nout, f.relu_out, f.lda = c.M, c.K, c.N1, c.nout, int(c.relu_out), c.A.sr
    return f, bands


@pytest.mark.parametrize("c", fr.fwd2_cases(), ids=lambda c: c.name)
def test_fwd2(lib, c):
    """H (row stride N1, a band right behind the last row) and the whole 16-wide Q row (columns nout..15 exactly
    +0.0) against float64; on exact cases also bit-equal to two st_f32b_gemm STORE launches on the same data."""
    L, native, mlp = lib
    f, bands = _fwd2_setup(mlp, c)
    assert f.lda > c.K
    snaps = snap_all(bands)
    assert L.st_f32b_fwd2(C.byref(f), native.stream_handle()) == 0
    torch.cuda.synchronize()
    intact(bands, snaps, written=("H", "Q"))
    Hg, Qg = np_of(bands["H"]), np_of(bands["Q"]).reshape(c.M, 16)
    d, r1, r2 = fr.check_fwd2(c, Hg, Qg)
    assert d == 0, (c.name, d, r1, r2)
    assert fr.check_bits(Qg[:, c.nout:], np.zeros((c.M, 16 - c.nout), F)) == 0
    if not c.exact:
        print(f"[meas] fwd2 {c.name}: max err/bound H = {r1:.4f}, Q = {r2:.4f}")
        return
    H2, Q2 = fband(np.full(c.M * c.N1, np.nan, F)), fband(np.full(c.M * 16, np.nan, F))
    g = mlp.GemmF32()
    g.A, g.B, g.C, g.bias = f.A, f.W1, H2.ptr(), f.b1
    g.M, g.N, g.K, g.am, g.ak, g.bn, g.bk, g.ldc = c.M, c.N1, c.K, c.A.sr, 1, c.K, 1, c.N1
    g.epi, g.relu = fr.F32B_STORE, 1
    assert L.st_f32b_gemm(C.byref(g), 1, native.stream_handle()) == 0
    g2 = mlp.GemmF32()
    g2.A, g2.B, g2.C, g2.bias = H2.ptr(), f.W2, Q2.ptr(), f.b2
    g2.M, g2.N, g2.K, g2.am, g2.ak, g2.bn, g2.bk, g2.ldc = c.M, c.nout, c.N1, c.N1, 1, c.N1, 1, 16
    g2.epi, g2.relu = fr.F32B_STORE, int(c.relu_out)
    assert L.st_f32b_gemm(C.byref(g2), 1, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert H2.guards_intact() and Q2.guards_intact()
    assert fr.check_bits(np_of(H2), Hg) == 0
    assert fr.check_bits(np_of(Q2).reshape(c.M, 16)[:, :c.nout], Qg[:, :c.nout]) == 0


def test_fwd2_refusals(lib):
    L, native, mlp = lib

    def refused(N1=64, K=36, nout=3, lda_add=0, off=()):
        c = fr.make_fwd2("r", 65, K, N1, max(1, min(nout, 3)), False, True, True, seed=1)
        f, bands = _fwd2_setup(mlp, c)
        f.nout, f.lda = nout, f.lda + lda_add
        for k in off:
            setattr(f, k, getattr(f, k) + 4)
        snaps = snap_all(bands)
        rc = L.st_f32b_fwd2(C.byref(f), native.stream_handle())
        torch.cuda.synchronize()
        intact(bands, snaps)
        return rc

    assert refused(N1=257) == INVALID
    assert refused(K=6) == INVALID and refused(lda_add=2) == INVALID
    assert refused(nout=0) == INVALID and refused(nout=4) == INVALID
    for k in ("A", "W1", "Q"):
        assert refused(off=(k,)) == INVALID, k


# ----------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("c", fr.colsum_cases(), ids=lambda c: c.name)
def test_colsum(lib, c):
    """Both entries on one case.  The contracts differ and both are asserted: st_f32b_colsum ADDS to ``out`` (a
    non-zero prior), st_f32b_colsum_det OVERWRITES it.  The deterministic entry gets exactly
    st_f32b_colsum_part_floats(E, N) floats of scratch inside a band, reports its block count (nparts * N fits), runs
    with nparts null as well, and two runs are bit-identical.  The form each entry takes (float4 / fallback) is the one
    the case is listed for: the block count equals the model's."""
    L, native, mlp = lib
    sh = native.stream_handle()
    D = fband(c.D.flat)
    prior = np.r_[np.full(c.out_off, np.nan, F), c.prior]
    assert c.D.sr > c.N
    # atomic entry
    out = fband(prior)
    snap = D.snap()
    assert L.st_f32b_colsum(D.ptr() + 4 * c.D.off, c.D.sr, c.E, c.N, out.ptr() + 4 * c.out_off, sh) == 0
    torch.cuda.synchronize()
    assert D.same(snap) and out.guards_intact()
    got = np_of(out)
    assert fr.check_bits(got[:c.out_off], prior[:c.out_off]) == 0
    assert fr.check_colsum(c, False, got[c.out_off:]) == 0, c.name
    if not c.exact:
        ref, bound = fr.colsum_ref(c, False)
        print(f"[meas] colsum {c.name}: max err/bound = {float((np.abs(got[c.out_off:] - ref) / bound).max()):.4f}")
    # deterministic entry
    nfl = int(L.st_f32b_colsum_part_floats(c.E, c.N))
    assert nfl == fr.colsum_part_floats(c.E, c.N)
    runs = []
    for with_nparts in (True, False, True):
        out = fband(prior)
        part = fband(np.full(nfl, np.nan, F))
        nparts = C.c_int(-1)
        rc = L.st_f32b_colsum_det(D.ptr() + 4 * c.D.off, c.D.sr, c.E, c.N, out.ptr() + 4 * c.out_off, part.ptr(),
                                  C.byref(nparts) if with_nparts else None, sh)
        torch.cuda.synchronize()
        assert rc == 0 and D.same(snap) and out.guards_intact() and part.guards_intact()
        got = np_of(out)
        _, _, nb = fr.colsum_model(c, True)
        if with_nparts:
            assert nparts.value == nb and nparts.value * c.N <= nfl, (c.name, nparts.value, nb)
        assert fr.check_colsum(c, True, got[c.out_off:], np_of(part), nb) == 0, c.name
        runs.append((got, np_of(part)))
    assert fr.check_bits(runs[0][0], runs[2][0]) == 0 and fr.check_bits(runs[0][1], runs[2][1]) == 0


def test_colsum_refusals(lib):
    L, native, mlp = lib
    c = fr.colsum_cases()[0]
    D, out, part = fband(c.D.flat), fband(c.prior), fband(np.full(8192, np.nan, F))
    bands = dict(D=D, out=out, part=part)
    snaps = snap_all(bands)
    for E, N in ((0, 4), (4, 0), (-1, 4)):
        assert L.st_f32b_colsum(D.ptr(), c.D.sr, E, N, out.ptr(), native.stream_handle()) == INVALID
        assert L.st_f32b_colsum_det(D.ptr(), c.D.sr, E, N, out.ptr(), part.ptr(), None, native.stream_handle()) == INVALID
    torch.cuda.synchronize()
    intact(bands, snaps)


# ----------------------------------------------------------------------------- st_f32b_splitsum
@pytest.mark.parametrize("c", fr.splitsum_cases(), ids=lambda c: c.name)
def test_splitsum(lib, c):
    """The float4 form (64-stride main loop + 16-stride tail + LDS fold) and the one-element form (n % 4, zstride % 4,
    a misaligned part or out): exact cases bit for bit, Gaussian ones within gamma(splits) sum |terms| + u |ref|; two
    runs bit-identical."""
    L, native, mlp = lib
    part = fband(c.part)
    # the form the launcher takes, by its rule on the real pointers
    runs = []
    for _ in range(2):
        out = fband(np.full(c.n + c.out_off, np.nan, F))
        pp, po = part.ptr() + 4 * c.part_off, out.ptr() + 4 * c.out_off
        assert bool(c.n % 4 or c.zstride % 4 or (pp | po) & 15) == c.one, c.name
        snap = part.snap()
        assert L.st_f32b_splitsum(pp, c.splits, c.zstride, po, c.n, native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert part.same(snap) and out.guards_intact()
        got = np_of(out)
        assert np.isnan(got[:c.out_off]).all()
        d, ratio = fr.check_splitsum(c, got[c.out_off:])
        assert d == 0, (c.name, d, ratio)
        runs.append(got)
    assert fr.check_bits(runs[0], runs[1]) == 0
    if not c.exact:
        print(f"[meas] splitsum {c.name}: max err/bound = {ratio:.4f}")


def test_splitsum_refusals(lib):
    L, native, mlp = lib
    c = fr.splitsum_cases()[1]
    part, out = fband(c.part), fband(np.full(c.n, np.nan, F))
    bands = dict(part=part, out=out)
    snaps = snap_all(bands)
    sh = native.stream_handle()
    assert L.st_f32b_splitsum(part.ptr(), 0, c.zstride, out.ptr(), c.n, sh) == INVALID
    assert L.st_f32b_splitsum(part.ptr(), c.splits, c.zstride, out.ptr(), 0, sh) == INVALID
    assert L.st_f32b_splitsum(part.ptr(), c.splits, c.zstride, out.ptr(), -4, sh) == INVALID
    assert L.st_f32b_splitsum(part.ptr(), c.splits, c.n - 4, out.ptr(), c.n, sh) == INVALID
    torch.cuda.synchronize()
    intact(bands, snaps)


# ----------------------------------------------------------------------------- gather, env, td
def _batch_setup(native, mlp, c, what):
    """Bands of everything one env-side launch may touch and the filled F32Batch."""
    from sharetrade.utils import rng as strng

    k, st, E = c.k, c.state, c.E
    b = dict(prices=fband(c.prices.reshape(-1)), X=fband(np.full(E * c.in_p, np.nan, F)),
             XN=fband(np.full(E * c.in_p, np.nan, F)), Q=fband(c.Q.reshape(-1)), QN=fband(c.QN.reshape(-1)),
             DQ=fband(np.full(E * 16, np.nan, F)), loss=fband(np.full(E, np.nan, F)),
             budget=fband(st["budget"]), shares=iband(st["shares"]), value=fband(st["value"]), pos=iband(st["pos"]),
             episodes=iband(st["episodes"]), last_final=fband(st["last_final"]), ret_sum=fband(st["ret_sum"]),
             actions_out=iband(np.full(E, -9, np.int32)), rewards_out=fband(np.full(E, np.nan, F)),
             ctrl=iband(np.array([k["step"], 1], np.int64), torch.int64),
             stat=Band(2, torch.float64, NAN).set(torch.from_numpy(c.stat0.copy())))
    if what == "td":
        b.update(s_b2=fband(c.scr["s_b2"]), s_s2=iband(c.scr["s_s2"]), s_rew=fband(c.scr["s_rew"]),
                 s_act=iband(c.scr["s_act"]))
    else:
        b.update(s_b2=fband(np.full(E, np.nan, F)), s_s2=iband(np.full(E, -9, np.int32)),
                 s_rew=fband(np.full(E, np.nan, F)), s_act=iband(np.full(E, -9, np.int32)))
    if c.QT is not None:
        b["QT"] = fband(c.QT.reshape(-1))
    r = mlp.F32Batch()
    r.E, r.in_p, r.H, r.T, r.bias_col, r.feat_mode = E, c.in_p, c.H, c.T, c.bias_col, k["feat_mode"]
    for n in ("X", "XN", "Q", "QN", "DQ", "loss", "s_b2", "s_s2", "s_rew", "s_act", "prices", "budget", "shares",
              "value", "pos", "episodes", "last_final", "ret_sum", "ctrl"):
        setattr(r, n, b[n].ptr())
    r.actions_out = b["actions_out"].ptr() if k["actions_out"] else None
    r.rewards_out = b["rewards_out"].ptr() if k["rewards_out"] else None
    r.stat = b["stat"].ptr() if k["stat"] else None
    r.QT = b["QT"].ptr() if c.QT is not None else None
    for n in ("compat_env", "target_compat", "output_relu", "s0", "env_offset", "reward_mode", "eps", "inv_ramp",
              "b0", "inv_b0", "gamma", "coef", "td_clip", "reward_scale", "double_dqn", "ramp_global"):
        setattr(r, n, k[n])
    k0, k1 = strng.key_for(k["seed"], 0)
    r.key0, r.key1 = int(k0), int(k1)
    return r, b


@pytest.mark.parametrize("c", fr.batch_cases(), ids=lambda c: c.name)
def test_gather_env(lib, c):
    """st_f32b_gather then st_f32b_env on the same buffers.  Gather: every column of X and X' written, zero pad
    included, the budget / shares columns of x' still 0.  Env: the draw, the exploit ramp, ties, the trade and the
    reward bit-equal to the fp32 op-by-op model on every case; actions_out / rewards_out null in some cases."""
    L, native, mlp = lib
    r, b = _batch_setup(native, mlp, c, "env")
    sh = native.stream_handle()
    snaps = snap_all(b)
    assert L.st_f32b_gather(C.byref(r), sh) == 0
    torch.cuda.synchronize()
    intact(b, snaps, written=("X", "XN"))
    X, XN = np_of(b["X"]).reshape(c.E, c.in_p), np_of(b["XN"]).reshape(c.E, c.in_p)
    assert fr.check_gather(c, X, XN) == 0, c.name
    assert fr.check_bits(XN[:, c.H:c.H + 2], np.zeros((c.E, 2), F)) == 0
    snaps = snap_all(b)
    assert L.st_f32b_env(C.byref(r), sh) == 0
    torch.cuda.synchronize()
    written = ["XN", "s_b2", "s_s2", "s_rew", "s_act"] + ["actions_out"] * bool(c.k["actions_out"]) + \
        ["rewards_out"] * bool(c.k["rewards_out"])
    intact(b, snaps, written=written)
    got = {n: np_of(b[n]) for n in ("s_b2", "s_s2", "s_rew", "s_act")}
    got["XN"] = np_of(b["XN"]).reshape(c.E, c.in_p)
    if c.k["actions_out"]:
        got["actions_out"] = np_of(b["actions_out"])
    if c.k["rewards_out"]:
        got["rewards_out"] = np_of(b["rewards_out"])
    assert fr.check_env(c, got) == 0, c.name


def test_gather_refusals(lib):
    L, native, mlp = lib
    c = fr.batch_cases()[2]
    for edit in ("in_p", "X", "XN"):
        r, b = _batch_setup(native, mlp, c, "env")
        if edit == "in_p":
            r.in_p = 6
        else:
            setattr(r, edit, getattr(r, edit) + 4)
        snaps = snap_all(b)
        assert L.st_f32b_gather(C.byref(r), native.stream_handle()) == INVALID, edit
        torch.cuda.synchronize()
        intact(b, snaps)


@pytest.mark.parametrize("c", fr.batch_cases(), ids=lambda c: c.name)
def test_td(lib, c):
    """st_f32b_td from given Q, Q(x'), target rows and scratch: the whole 16-wide dQ row, the loss, the new state
    (episode end at exactly pos + 1 == T - H), and -- dyadic cases -- the two double statistics added onto a non-zero
    prior, bit-equal to the float64 sums whatever the order of the two blocks' atomics (E = 1,025: one live thread in
    the last block)."""
    L, native, mlp = lib
    r, b = _batch_setup(native, mlp, c, "td")
    snaps = snap_all(b)
    assert L.st_f32b_td(C.byref(r), native.stream_handle()) == 0
    torch.cuda.synchronize()
    written = ["DQ", "loss"] + list(fr.STATE_KEYS) + ["stat"] * bool(c.k["stat"])
    intact(b, snaps, written=written)
    got = dict(DQ=np_of(b["DQ"]).reshape(c.E, 16), loss=np_of(b["loss"]), state={n: np_of(b[n]) for n in fr.STATE_KEYS})
    if c.k["stat"]:
        got["stat"] = np_of(b["stat"])
    assert fr.check_td(c, got) == 0, c.name


# ----------------------------------------------------------------------------- st_f32b_target_sync
def test_target_sync(lib):
    """The target equals the parameters bit for bit when ctrl[0] % every == 0 and is bit-unchanged otherwise."""
    L, native, mlp = lib
    for n, every, c0 in fr.SYNC_CASES:
        p = np.random.default_rng(n).standard_normal(n).astype(F)
        t = -p - 1
        P, Tg, ctrl = fband(p), fband(t), iband(np.array([c0, 7], np.int64), torch.int64)
        bands = dict(P=P, T=Tg, ctrl=ctrl)
        snaps = snap_all(bands)
        assert L.st_f32b_target_sync(P.ptr(), Tg.ptr(), n, ctrl.ptr(), every, native.stream_handle()) == 0
        torch.cuda.synchronize()
        intact(bands, snaps, written=("T",))
        assert fr.check_sync(p, t, every, c0, np_of(Tg)) == 0, (n, every, c0)
        for bad_n, bad_every in ((0, every), (-1, every), (n, 0), (n, -3)):
            snaps = snap_all(bands)
            assert L.st_f32b_target_sync(P.ptr(), Tg.ptr(), bad_n, ctrl.ptr(), bad_every,
                                         native.stream_handle()) == INVALID
            torch.cuda.synchronize()
            intact(bands, snaps)


# ----------------------------------------------------------------------------- st_f32_grad_optim, mode 2
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("P", [1, 255, 257, 1000])
def test_optim_mode2(lib, P, kind):
    """Three successive updates from a reduced gradient (mode 2), scale 0.37, a mask with zeros and non-unit entries,
    t from ctrl (ctrl[0] = 0, 1, 2 -> t = 1, 2, 3) and a fourth update with t from o.t (= 1,000; ctrl null).  Every
    update is compared with the float64 reference applied to the state the kernel started it from.  Masked entries
    are bit-unchanged in the parameters and both state buffers; grad is never written.  SGD and AdaGrad: within the
    bounds derived from the operation count (tests/f32b_refs.py; fma contraction only removes roundings).  Adam: the
    states within their derived bounds, the parameters within ADAM_MARGIN x ADAM_MEASURED x B_adam = 4 x 3.53 x B_adam:
    powf's error is measured on the GPU against the float64 reference (3.53 B_adam, profiles/f32b_refs.md), not assumed;
    the margin is 4 x because powf's error varies with t and beta and the test samples few values of them."""
    L, native, mlp = lib
    g = np.random.default_rng(10 * P + kind)
    w = (0.1 + 0.05 * g.standard_normal(P)).astype(F)
    mask = g.choice(np.array([0.0, 1.0, 1.0, 0.5, 2.0], F), P)
    mask[0] = 1.0 if P == 1 else 0.0
    mask[-1] = 1.0
    s1, s2 = (0.1 + g.random(P)).astype(F), (0.1 * g.random(P)).astype(F)
    if kind == 2:
        s1 = (0.1 * g.standard_normal(P)).astype(F)
    b = dict(params=fband(w), mask=fband(mask), s1=fband(s1), s2=fband(s2), grad=fband(np.zeros(P, F)),
             ctrl=iband(np.array([0, 0], np.int64), torch.int64))
    net = mlp.F32Net()
    net.P = P
    o = mlp.F32Optim()
    o.params, o.mask, o.s1, o.s2, o.grad = (b[n].ptr() for n in ("params", "mask", "s1", "s2", "grad"))
    o.acts, o.dz, o.B, o.kind, o.mode = None, None, 0, kind, 2
    o.lr, o.beta1, o.beta2, o.eps, o.scale = fr.OPT_LR, fr.OPT_B1, fr.OPT_B2, fr.OPT_EPS, 0.37
    dead = mask == 0
    worst = 0.0
    for it, t in enumerate((1, 2, 3, 1000)):
        grad = g.standard_normal(P).astype(F)
        b["grad"].set(torch.from_numpy(grad))
        if it < 3:
            b["ctrl"].set(torch.tensor([t - 1, 0]))
            o.ctrl, o.t = b["ctrl"].ptr(), -5
        else:
            o.ctrl, o.t = None, t
        w0, a0, c0 = np_of(b["params"]), np_of(b["s1"]), np_of(b["s2"])
        snaps = snap_all(b)
        assert L.st_f32_grad_optim(C.byref(net), C.byref(o), native.stream_handle()) == 0
        torch.cuda.synchronize()
        intact(b, snaps, written=("params",) + ((), ("s1",), ("s1", "s2"))[kind])
        w1, a1, c1 = np_of(b["params"]), np_of(b["s1"]), np_of(b["s2"])
        for new, old in ((w1, w0), (a1, a0), (c1, c0)):
            assert fr.check_bits(new[dead], old[dead]) == 0
        rw, ra, rc, bw, ba, bc = fr.optim_ref(kind, w0, mask, a0, c0, grad, t, 0.37)
        live = ~dead
        assert (np.abs(a1 - ra) <= ba)[live].all() and (np.abs(c1 - rc) <= bc)[live].all(), (kind, t)
        ratio = float((np.abs(w1 - rw)[live] / bw[live]).max())
        worst = max(worst, ratio)
        assert (w1 != w0)[live].any()
        if kind != 2:
            assert ratio <= 1.0, (kind, t, ratio)
    print(f"[meas] optim kind={kind} P={P}: max err/bound = {worst:.4f}")
    if kind == 2:
        assert worst <= ADAM_MARGIN * ADAM_MEASURED, worst
