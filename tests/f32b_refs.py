"""Float64 references, case lists, data-movement models and comparisons for the batched exact-fp32 step
(csrc/mlp_f32_mfma.hip) and the mode-2 optimizer pass (csrc/mlp_f32.hip f32_grad_optim).  No GPU; numpy.

tests/test_gpu_f32b_kernels.py launches the committed cases through the ``st_f32b_*`` entry points, every operand a
strided region inside a NaN-filled guard band, and compares with the references here through the ``check_*``
functions; tests/test_f32b_refs.py runs numpy models of the kernels' data movement through the same functions,
unmutated (0 differences) and with one mutation at a time (> 0 differences each).

Regions.  Every operand is a ``Region``: a strided 2-D view of a flat fp32 buffer whose gaps (row padding, the float
in front of a misaligned base) hold NaN.  The models read the flat buffers with the kernels' own index arithmetic,
so a load or a store outside the region meets a NaN or changes a gap, and both count as differences.  The references
never look at the flat buffers: they take the dense values.

Exact cases.  Operands are small integers, so every partial sum needs fewer than 24 bits (measured per case by
``step_refs.dot_bits`` -- ``assert_exact_*`` raises otherwise).  fp32 is then exact in any order: the kernel must
equal the float64 reference bit for bit, whatever the MFMA's internal order, the split or the order of the atomics.
The comparison is on bit patterns, signed zeros included: an accumulator starts at +0.0 and a sum of products that
cancels rounds to +0.0, and (+0.0) + (-0.0 bias) = +0.0, so -0.0 never reaches ``fmaxf`` and no output is -0.0; the
references normalise with ``+ 0.0`` and a kernel that leaves a -0.0 differs.

Gaussian cases.  Full-mantissa fp32 operands; per element, with u = 2^-24 and gamma(n) = n u / (1 - n u) (the
standard bound of an n-term sum of rounded products in any order, Higham, Accuracy and Stability, ch. 3/4):

    |got - ref| <= gamma(n + c) * sum |terms| + u |ref|

n is the number of products of the dot product (each rounded at most once, the partial sums at most n - 1 times),
c the extra roundings of the epilogue counted from the code, and the last term the rounding of the stored value:

    F32B_STORE    c = 1 with a bias (one add; the bias is one more term of sum |terms|), else 0
    F32B_MASK     c = 0 (a select)
    F32B_ATOMIC   c = splits (one atomic add per split, onto the prior C, which is one more term)
    F32B_PARTIAL  c = 0 per partial tile
    split-sum     n = splits, c = 0 (plain adds; any grouping)
    column sums   n = E, c = 1 (the atomic onto the prior ``out``, one more term), the same for both forms
    fwd2 H        as STORE with a bias;  fwd2 Q: n = N1 products h * w2 (fma chain, shuffles, LDS fold: some tree
                  over the N1 terms), c = 1 for b2, plus the error H carries in: sum_n |w2[a][n]| * bound_H[m][n]

The optimizer (mode 2), from the operation count of csrc/mlp_f32.hip (each * + / sqrt one rounding, correctly
rounded; an fma contraction removes a rounding, so it only lowers the error):

    g' = g * (m * scale)                                   relative 2u
    SGD      w' = w - lr g'            |err| <= gamma(3) |lr g'| + u |w'|
    AdaGrad  a = s1 + g'^2             |err| <= gamma(6) a          (g'^2: 5u; the add: u; all terms positive)
             w' = w - lr g' / sqrt(a)  |err| <= gamma(8) |upd| + u |w'|   (lr g': 3u, sqrt a: 3u + u, divide: u)
    Adam     m' = b1 s1 + (1 - b1) g'  |err| <= gamma(5) (|b1 s1| + |(1 - b1) g'|) =: e_m
             v' = b2 s2 + (1 - b2) g'^2  |err| <= gamma(8) v'
             upd = lr (m'/c1) / (sqrt(v'/c2) + eps):  c1, c2 one rounding each beyond powf; m'/c1: e_m / |m'| + 2u;
             sqrt(v'/c2) + eps: (8u + u + u) / 2 + u + u = 7u; lr * and the last divide: 2u
             |err| <= gamma(11) |upd| + |upd / m'| e_m + u |w'|  =: B_adam, powf's own error NOT included.
    powf's device error is measured in units of B_adam (profiles/f32b_refs.md) and the GPU test asserts 4 x that."""
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from step_refs import check_int, dot_bits, r32, reward, sum_bits, trade
from sharetrade.utils import rng as strng

F = np.float32
U = 2.0 ** -24
LIMIT_BITS = 24.0
F32B_STORE, F32B_MASK, F32B_ATOMIC, F32B_PARTIAL = 0, 1, 2, 3
EPI_NAMES = ("store", "mask", "atomic", "partial")
LD_KF, LD_RF, LD_SC = 0, 1, 2
LD_NAMES = ("KF", "RF", "SC")
GB_M = GB_N = 64
GB_K = 32
NAN = np.nan

MUTATIONS = (
    "kf_ktail_dropped", "rf_rtail_dropped", "row_R_loaded", "last_ktile_dropped", "splits_overlap",
    "kchunk_unrounded", "mask_ge", "mask_ldc_for_ldaux", "bias_after_relu", "atomic_stores", "partial_z_minus_1",
    "fwd2_hidden_tail", "fwd2_q_pad", "fwd2_b2_skipped", "colsum_last_group", "colsum_det_adds", "splitsum_tail16",
    "splitsum1_n_for_zstride", "xn_not_shifted", "no_bias_col", "tie_last", "u2_exploit", "no_env_offset",
    "step_hi_ignored", "td_reset_late", "loss_from_clipped", "ddqn_target_argmax", "scale_stored_reward",
    "sync_plus_one")


def gamma(n):
    return n * U / (1.0 - n * U)


def ld_mode(addr: int, sr: int, sk: int) -> int:
    """csrc/mlp_f32_mfma.hip ld_mode, re-derived: the loader an operand at byte address ``addr`` gets."""
    al = addr % 16 == 0
    if al and sk == 1 and sr % 4 == 0:
        return LD_KF
    if al and sr == 1 and sk % 4 == 0:
        return LD_RF
    return LD_SC


# ----------------------------------------------------------------------------- regions
class Region:
    """R x C values at flat[off + r * sr + c * sc] of a NaN-filled fp32 buffer (``tail`` more floats behind)."""

    def __init__(self, R, C, sr, sc, off=0, tail=0, fill=NAN):
        self.R, self.C, self.sr, self.sc, self.off = int(R), int(C), int(sr), int(sc), int(off)
        self.flat = np.full(self.off + (self.R - 1) * self.sr + (self.C - 1) * self.sc + 1 + int(tail), fill, F)

    def idx(self):
        return self.off + np.arange(self.R)[:, None] * self.sr + np.arange(self.C)[None, :] * self.sc

    def put(self, v):
        self.flat[self.idx()] = np.asarray(v, F)
        return self

    def get(self, flat=None):
        return (self.flat if flat is None else np.asarray(flat))[self.idx()].astype(np.float64)

    def mode(self, base_addr=0):
        """The loader of this region as a GEMM operand (rows = r, k = c)."""
        return ld_mode(base_addr + 4 * self.off, self.sr, self.sc)


def _rup(x, m):
    return -(-x // m) * m


def operand(R, K, mode, variant=0):
    """A Region of R rows and K k-values whose strides and base force loader ``mode``.  LD_SC comes three ways:
    an odd row stride, a base one float off, an odd k stride of a k-major layout."""
    if mode == LD_KF:
        return Region(R, K, _rup(K, 4) + 4, 1)
    if mode == LD_RF:
        return Region(R, K, 1, _rup(R, 4) + 4)
    v = variant % 3
    if v == 0:
        return Region(R, K, (K + 2) | 1, 1)
    if v == 1:
        return Region(R, K, _rup(K, 4) + 4, 1, off=1)
    return Region(R, K, 1, (R + 2) | 1)


def rd(flat, idx):
    """flat[idx], NaN where idx is outside the buffer (the guard band of the GPU test)."""
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < flat.size)
    return np.where(ok, flat[np.where(ok, idx, 0)].astype(np.float64), NAN)


def bits32(v):
    return np.ascontiguousarray(v, dtype=F).view(np.uint32)


def check_bits(got, ref):
    """Differing fp32 bit patterns (signed zeros and NaN payloads count)."""
    a, b = bits32(got), bits32(ref)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).sum())


def check_bound(got, ref64, bound, mask):
    """(violations, largest err / bound) over ``mask``; outside it the bit patterns of ``got`` must equal ref's."""
    got64 = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got64 - ref64)
        ratio = np.where(err == 0, 0.0, err / bound)
    bad = mask & ~(err <= bound)
    out = int(bad.sum()) + int((bits32(got) != bits32(np.asarray(ref64).astype(F)))[~mask].sum())
    return out, float(np.nan_to_num(ratio[mask], nan=np.inf).max()) if mask.any() else 0.0


# ----------------------------------------------------------------------------- GEMM: cases
@dataclass
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    am: int
    bm: int
    epi: int
    splits: int
    relu: bool
    exact: bool
    A: Region            # rows m, k
    B: Region            # rows n, k  (B(k, n) = flat[k * bk + n * bn]: sr = bn, sc = bk)
    C: Region            # [M][ldc]; PARTIAL: ``splits`` tiles, zstride apart
    bias: Optional[np.ndarray] = None
    aux: Optional[Region] = None
    zstride: int = 0
    notes: Dict[str, object] = field(default_factory=dict)


ACT_PALETTE = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0x3F800000, 0xBF800000],
                       np.uint32).view(F)   # +0, -0, smallest subnormals, +inf, +1, -1 (as gemm_refs.ACT_PALETTE)
ACT_PROB = (0.30, 0.10, 0.06, 0.06, 0.02, 0.23, 0.23)


def split_rule(K, splits, mut=None):
    """The launcher's (kchunk, split count): K per split rounded up to whole 32-wide k-tiles."""
    kc = -(-K // splits)
    if mut != "kchunk_unrounded":
        kc = _rup(kc, GB_K)
    return kc, -(-K // kc)


def make_gemm(name, M, N, K, am, bm, epi, splits=1, bias=False, relu=False, exact=True, seed=0, variant=0,
              dense=False):
    g = np.random.default_rng(seed)
    A, B = operand(M, K, am, variant), operand(N, K, bm, variant + 1)
    if exact:
        A.put(g.integers(-8, 9, (M, K)))
        B.put(g.integers(-8, 9, (N, K)))
    else:
        A.put(g.standard_normal((M, K)))
        B.put(g.standard_normal((N, K)))
    ldc = N if dense else N + 1 + (seed % 3)
    c = GemmCase(name, M, N, K, am, bm, epi, splits, relu, exact, A, B, None)
    if epi == F32B_PARTIAL:
        c.zstride = _rup(M * ldc, 4) + 4 if dense else M * ldc + 5
        c.C = Region(M, N, ldc, 1, tail=(splits - 1) * c.zstride + ldc - N)
    else:
        c.C = Region(M, N, ldc, 1, tail=ldc - N)
    if epi == F32B_ATOMIC:   # the contract is C +=: a non-zero prior
        c.C.put(g.integers(-64, 65, (M, N)) if exact else g.standard_normal((M, N)))
    if epi == F32B_STORE and bias:
        b = (g.integers(-64, 65, N) if exact else g.standard_normal(N)).astype(F)
        b[0] = F(-0.0)
        c.bias = b
    if epi == F32B_MASK:
        c.aux = Region(M, N, N + 3, 1)
        a = ACT_PALETTE[g.choice(len(ACT_PALETTE), size=M * N, p=ACT_PROB)]
        nfix = min(len(ACT_PALETTE), a.size)   # fixed positions: every palette value is known to occur
        a[:nfix] = ACT_PALETTE[:nfix]
        c.aux.put(a.reshape(M, N))
    if exact:
        c.notes["bits"] = assert_exact_gemm(c)
    return c


def assert_exact_gemm(c: GemmCase):
    extra = None
    if c.bias is not None:
        extra = c.bias.astype(np.float64)
    b = dot_bits(c.A.get(), c.B.get().T, extra)
    if c.epi == F32B_ATOMIC:   # the prior joins every sum: operands and prior are integers, so the grid is >= 1
        A, B, pr = c.A.get(), c.B.get().T, c.C.get()
        assert all(np.array_equal(x, np.rint(x)) for x in (A, B, pr))
        b = max(b, float(np.log2((np.abs(A) @ np.abs(B) + np.abs(pr)).max())))
    if b >= LIMIT_BITS:
        raise AssertionError(f"gemm case {c.name}: not exact in fp32, {b:.1f} bits")
    return b


_MS, _NS, _KS = (1, 63, 64, 65, 130), (3, 16, 64, 67, 200), (1, 4, 31, 32, 33, 67, 100)
_SPLITS = (1, 2, 3, 5)
_GEMM = None


def gemm_cases():
    """The covering set (built once): for every (AM, BM) loader pair seven exact cases -- every K, every epilogue;
    every M with every A loader, every N with every B loader -- the split cases (K = 40 / splits = 3 runs 2),
    every split count with both split epilogues, and one Gaussian case per loader pair."""
    global _GEMM
    if _GEMM is not None:
        return _GEMM
    out = []
    for am in range(3):
        for bm in range(3):
            for j in range(7):
                M, N, K = _MS[(j + bm) % 5], _NS[(j + 2 * am + bm) % 5], _KS[j]
                epi = (j + am + bm) % 4
                sp = _SPLITS[(j + am) % 4] if epi >= F32B_ATOMIC else 1
                out.append(make_gemm(f"{LD_NAMES[am]}{LD_NAMES[bm]}-{M}x{N}x{K}-{EPI_NAMES[epi]}{sp}", M, N, K, am, bm,
                                     epi, sp, bias=bool(j & 1) or epi != 0, relu=bool((j >> 1) & 1), seed=len(out),
                                     variant=j))
    for epi in (F32B_ATOMIC, F32B_PARTIAL):
        out.append(make_gemm(f"shrink-40-{EPI_NAMES[epi]}3", 65, 67, 40, LD_KF, LD_RF, epi, 3, seed=len(out)))
        for i, sp in enumerate(_SPLITS):
            M, N = (130, 67) if i & 1 else (63, 200)
            out.append(make_gemm(f"split-{M}x{N}x100-{EPI_NAMES[epi]}{sp}", M, N, 100, (i + epi) % 3, i % 3, epi, sp,
                                 seed=len(out), variant=i))
    # every tail with the two unsplit epilogues, bias / relu in all four combinations
    for i, (M, N, K) in enumerate(((63, 67, 31), (65, 3, 33), (130, 200, 67), (1, 16, 1))):
        out.append(make_gemm(f"tails-{M}x{N}x{K}-store", M, N, K, i % 3, (i + 1) % 3, F32B_STORE, 1, bias=bool(i & 1),
                             relu=bool(i & 2), seed=len(out), variant=i))
        out.append(make_gemm(f"tails-{M}x{N}x{K}-mask", M, N, K, (i + 1) % 3, i % 3, F32B_MASK, 1, seed=len(out),
                             variant=i))
    for am in range(3):
        for bm in range(3):
            epi = (am * 3 + bm) % 4
            out.append(make_gemm(f"gauss-{LD_NAMES[am]}{LD_NAMES[bm]}-{EPI_NAMES[epi]}", 130, 67, 100, am, bm, epi,
                                 3 if epi >= F32B_ATOMIC else 1, bias=True, relu=bool(am & 1), exact=False,
                                 seed=900 + len(out), variant=am + bm))
    _GEMM = out
    return out


def small_split_cases():
    """Dense-C cases (ldc == N, zstride % 4 == 0) on which PARTIAL + split-sum must equal ATOMIC bit for bit."""
    out = []
    for i, (M, N, K, sp) in enumerate(((63, 16, 100, 3), (65, 64, 67, 2), (130, 4, 40, 3), (1, 200, 100, 5))):
        out.append((M, N, K, sp, i % 3, (i + 1) % 3, 700 + i))
    return out


def gemm_tails(c: GemmCase):
    """Which tails a case has: partial row block, partial column block, partial k-tile, a float4 tail inside a row
    that is in range (per operand loader)."""
    t = set()
    if c.M % GB_M:
        t.add("row")
    if c.N % GB_N:
        t.add("col")
    if c.K % GB_K:
        t.add("k")
    if (c.am == LD_KF and c.K % 4) or (c.bm == LD_KF and c.K % 4) or (c.am == LD_RF and c.M % 4) or \
            (c.bm == LD_RF and c.N % 4):
        t.add("f4")
    return t


# ----------------------------------------------------------------------------- GEMM: reference
def gemm_ref(c: GemmCase):
    """(expected flat C as float64 -- NaN where nothing may be written --, per-element bound or None, written mask).
    Plain float64 matmuls of the dense operands; PARTIAL: one per split of the documented rule."""
    A, B = c.A.get(), c.B.get().T
    ref = c.C.flat.astype(np.float64).copy()
    bound = np.zeros(ref.size)
    mask = np.zeros(ref.size, bool)
    idx = c.C.idx()
    mag = np.abs(A) @ np.abs(B)
    if c.epi == F32B_PARTIAL:
        kc, nz = split_rule(c.K, c.splits)
        for z in range(nz):
            ks = slice(z * kc, min(c.K, (z + 1) * kc))
            ref[idx + z * c.zstride] = A[:, ks] @ B[ks] + 0.0
            bound[idx + z * c.zstride] = gamma(ks.stop - ks.start) * (np.abs(A[:, ks]) @ np.abs(B[ks]))
            mask[idx + z * c.zstride] = True
    else:
        acc = A @ B + 0.0
        if c.epi == F32B_ATOMIC:
            _, nz = split_rule(c.K, c.splits)
            prior = c.C.get()
            v = acc + prior
            bnd = gamma(c.K + nz) * (mag + np.abs(prior))
        elif c.epi == F32B_MASK:
            v = np.where(c.aux.get() > 0.0, acc, 0.0)
            bnd = gamma(c.K) * mag
        else:
            v = acc
            bnd = gamma(c.K) * mag
            if c.bias is not None:
                v = acc + c.bias.astype(np.float64)[None, :]
                bnd = gamma(c.K + 1) * (mag + np.abs(c.bias.astype(np.float64))[None, :])
            if c.relu:
                v = np.where(v > 0.0, v, 0.0)
        ref[idx], bound[idx], mask[idx] = v, bnd, True
    bound = bound + U * np.abs(np.nan_to_num(ref))
    return ref, (None if c.exact else bound), mask


def check_gemm(c: GemmCase, got_flat):
    """(differences, largest err / bound) of the whole flat C buffer, gaps and unwritten partial slots included."""
    ref, bound, mask = gemm_ref(c)
    if c.exact:
        assert np.array_equal(np.nan_to_num(ref), np.nan_to_num(ref.astype(F).astype(np.float64))), "reference not fp32"
        return check_bits(got_flat, ref.astype(F)), 0.0
    return check_bound(got_flat, ref, bound, mask)


# ----------------------------------------------------------------------------- GEMM: model of the data movement
OUTSIDE = [0]   # loads the models issued outside their operand (a row at r == R feeds no stored output: it only
                # shows here; on the GPU it is an over-read into the guard band)


def tile_ld(mode, flat, off, sr, sk, r0, R, k0, kend, mut=None):
    """csrc/mlp_f32_mfma.hip tile_ld + tile_st: the 64 x 32 tile (rows r0.., k from k0) as the 512 loads of a
    workgroup fill it, with their bounds."""
    tile = np.zeros((GB_M, GB_K))
    i = np.arange(512)
    t = np.arange(4)[None, :]
    hi = R + 1 if mut == "row_R_loaded" else R
    if mode == LD_KF:
        r, k = (i >> 3)[:, None], (k0 + 4 * (i & 7))[:, None]
        rok = r0 + r < hi
        ok = rok & (k + t < kend)
        if mut == "kf_ktail_dropped":
            ok = rok & (k + 3 < kend) & (t >= 0)
        v = np.where(ok, rd(flat, off + (r0 + r) * sr + k + t), 0.0)
        OUTSIDE[0] += int((ok & (r0 + r >= R)).sum())
        tile[np.broadcast_to(r, v.shape), k + t - k0] = v
    elif mode == LD_RF:
        kk, r = (i >> 4)[:, None], (4 * (i & 15))[:, None]
        k = k0 + kk
        ok = (r0 + r + t < hi) & (k < kend)
        if mut == "rf_rtail_dropped":
            ok = (r0 + r + 3 < hi) & (k < kend) & (t >= 0)
        v = np.where(ok, rd(flat, off + (r0 + r + t) + k * sk), 0.0)
        OUTSIDE[0] += int((ok & (r0 + r + t >= R)).sum())
        tile[r + t, np.broadcast_to(kk, v.shape)] = v
    else:
        q = i[:, None] * 4 + t
        r, k = q & 63, k0 + (q >> 6)
        ok = (r0 + r < hi) & (k < kend)
        v = np.where(ok, rd(flat, off + (r0 + r) * sr + k * sk), 0.0)
        OUTSIDE[0] += int((ok & (r0 + r >= R)).sum())
        tile[r, q >> 6] = v
    return tile


def gemm_model(c: GemmCase, mut=None, base_addr=0):
    """The flat C buffer after one st_f32b_gemm launch, by the kernel's tiling, loaders, split rule and epilogues."""
    am, bm = c.A.mode(base_addr), c.B.mode(base_addr)
    C = c.C.flat.copy()
    kc, nz = split_rule(c.K, c.splits, mut)
    ldc = c.C.sr
    for z in range(nz):
        kb = z * kc
        if mut == "splits_overlap" and z > 0:
            kb -= GB_K
        ke = min(c.K, z * kc + kc)
        for by in range(-(-c.M // GB_M)):
            for bx in range(-(-c.N // GB_N)):
                m0, n0 = by * GB_M, bx * GB_N
                acc = np.zeros((GB_M, GB_N))
                k0 = kb
                while k0 < ke:
                    if not (mut == "last_ktile_dropped" and k0 + GB_K >= ke):
                        ta = tile_ld(am, c.A.flat, c.A.off, c.A.sr, c.A.sc, m0, c.M, k0, ke, mut)
                        tb = tile_ld(bm, c.B.flat, c.B.off, c.B.sr, c.B.sc, n0, c.N, k0, ke, mut)
                        acc = acc + ta @ tb.T
                    k0 += GB_K
                mm, nn = min(GB_M, c.M - m0), min(GB_N, c.N - n0)
                v = acc[:mm, :nn] + 0.0
                dst = c.C.off + (m0 + np.arange(mm))[:, None] * ldc + n0 + np.arange(nn)[None, :]
                if c.epi == F32B_PARTIAL:
                    zz = z - 1 if mut == "partial_z_minus_1" else z
                    d = dst + zz * c.zstride
                    okk = (d >= 0) & (d < C.size)
                    C[d[okk]] = v[okk]
                elif c.epi == F32B_ATOMIC:
                    C[dst] = v if mut == "atomic_stores" else (C[dst].astype(np.float64) + v)
                elif c.epi == F32B_MASK:
                    ld = ldc if mut == "mask_ldc_for_ldaux" else c.aux.sr
                    a = rd(c.aux.flat, c.aux.off + (m0 + np.arange(mm))[:, None] * ld + n0 + np.arange(nn)[None, :])
                    with np.errstate(invalid="ignore"):
                        keep = (a >= 0.0) if mut == "mask_ge" else (a > 0.0)
                    C[dst] = np.where(keep, v, 0.0)
                else:
                    b = 0.0 if c.bias is None else c.bias.astype(np.float64)[None, n0:n0 + nn]
                    if mut == "bias_after_relu" and c.relu:
                        v = np.where(v > 0.0, v, 0.0) + b
                    else:
                        v = v + b
                        if c.relu:
                            v = np.where(v > 0.0, v, 0.0)
                    C[dst] = v
    return C


# ----------------------------------------------------------------------------- fused two-layer forward
@dataclass
class Fwd2Case:
    name: str
    M: int
    K: int
    N1: int
    nout: int
    relu_out: bool
    exact: bool
    A: Region                      # [M][lda], lda > K
    W1: np.ndarray                 # [N1, K] dense
    W2: np.ndarray                 # [nout, N1] dense (the kernel reads rows < nout only)
    b1: Optional[np.ndarray]
    b2: Optional[np.ndarray]
    notes: Dict[str, object] = field(default_factory=dict)


def make_fwd2(name, M, K, N1, nout, relu_out, b1, b2, exact=True, seed=0):
    g = np.random.default_rng(seed)
    A = Region(M, K, K + 4 + 4 * (seed % 2), 1)
    if exact:
        draw = lambda *s: g.integers(-4, 5, s).astype(F)
    else:
        draw = lambda *s: g.standard_normal(s).astype(F)
    A.put(draw(M, K))
    c = Fwd2Case(name, M, K, N1, nout, relu_out, exact, A, draw(N1, K), draw(nout, N1),
                 draw(N1) if b1 else None, draw(nout) if b2 else None)
    if exact:
        h = fwd2_ref(c)[0]
        c.notes["bits_h"] = dot_bits(A.get(), c.W1.astype(np.float64).T, None if c.b1 is None else c.b1)
        c.notes["bits_q"] = dot_bits(h, c.W2.astype(np.float64).T, None if c.b2 is None else c.b2)
        if max(c.notes["bits_h"], c.notes["bits_q"]) >= LIMIT_BITS:
            raise AssertionError(f"fwd2 case {name}: not exact in fp32, {c.notes}")
    return c


_FWD2 = None


def fwd2_cases():
    """Every M, K, N1 and nout of the list, both values of relu_out, b1 and b2 null and non-null; N1 = 256 stays
    exact with operands in [-4, 4] (the measured bits are in the notes), so no Gaussian fallback is needed there."""
    global _FWD2
    if _FWD2 is None:
        Ms, Ks, N1s = (1, 63, 65, 130), (4, 36, 100, 208), (1, 3, 64, 65, 200, 256)
        out = []
        for j in range(12):
            M, K, N1, nout = Ms[j % 4], Ks[(j + j // 4) % 4], N1s[j % 6], 1 + j % 3
            out.append(make_fwd2(f"fwd2-{M}x{K}x{N1}x{nout}", M, K, N1, nout, bool(j & 1), bool((j >> 1) & 1) or j < 2,
                                 bool((j >> 2) & 1) or j == 1, seed=40 + j))
        out.append(make_fwd2("fwd2-gauss-130x100x200x3", 130, 100, 200, 3, False, True, True, exact=False, seed=60))
        out.append(make_fwd2("fwd2-gauss-65x208x256x2", 65, 208, 256, 2, True, True, True, exact=False, seed=61))
        _FWD2 = out
    return _FWD2


def fwd2_ref(c: Fwd2Case):
    """(H [M, N1], Q [M, 16], bound_H, bound_Q) in float64."""
    A, W1, W2 = c.A.get(), c.W1.astype(np.float64), c.W2.astype(np.float64)
    b1 = np.zeros(c.N1) if c.b1 is None else c.b1.astype(np.float64)
    z = A @ W1.T + b1 + 0.0
    h = np.where(z > 0.0, z, 0.0)
    bh = gamma(c.K + 1) * (np.abs(A) @ np.abs(W1).T + np.abs(b1)) + U * np.abs(h)
    q = np.zeros((c.M, 16))
    bq = np.zeros((c.M, 16))
    b2 = np.zeros(c.nout) if c.b2 is None else c.b2.astype(np.float64)
    v = h @ W2.T + b2 + 0.0
    bq[:, :c.nout] = gamma(c.N1 + 1) * (np.abs(h) @ np.abs(W2).T + np.abs(b2)) + bh @ np.abs(W2).T + U * np.abs(v)
    q[:, :c.nout] = np.where(v > 0.0, v, 0.0) if c.relu_out else v
    return h, q, bh, bq


def fwd2_model(c: Fwd2Case, mut=None):
    """(H [M, N1] row stride N1 with a NaN tail, Q [M, 16]) as the kernel moves the data: LD_KF tiles of A and of
    the four 64-unit quarters of W1, the hidden tail n >= N1, the 16-wide output row."""
    W1 = Region(c.N1, c.K, c.K, 1, tail=64).put(c.W1)
    b1 = None if c.b1 is None else np.r_[c.b1, np.full(256, NAN, F)]
    W2 = np.r_[c.W2.reshape(-1), np.full(512, NAN, F)].astype(np.float64)
    Hb = np.full(c.M * c.N1 + 64, NAN, F)
    Q = np.full((c.M, 16), NAN, F)
    n = np.arange(256)
    ok = n < (256 if mut == "fwd2_hidden_tail" else c.N1)
    bb = np.where(ok, 0.0 if b1 is None else b1[n].astype(np.float64), 0.0)
    w2 = np.zeros((3, 256))
    for a in range(min(c.nout, 3)):
        w2[a] = np.where(ok, W2[a * c.N1 + n], 0.0)
    for blk in range(-(-c.M // GB_M)):
        m0 = blk * GB_M
        acc = np.zeros((GB_M, 256))
        for k0 in range(0, c.K, GB_K):
            ta = tile_ld(LD_KF, c.A.flat, c.A.off, c.A.sr, 1, m0, c.M, k0, c.K)
            for q in range(4):
                tb = tile_ld(LD_KF, W1.flat, 0, c.K, 1, 64 * q, c.N1, k0, c.K)
                acc[:, 64 * q:64 * q + 64] += ta @ tb.T
        z = acc + bb[None, :]
        h = np.where(z > 0.0, z, np.where(np.isnan(z), NAN, 0.0))
        mm = min(GB_M, c.M - m0)
        for r in range(mm):
            Hb[(m0 + r) * c.N1:(m0 + r) * c.N1 + c.N1] = h[r, :c.N1]
        with np.errstate(invalid="ignore"):
            part = np.stack([(h * w2[a][None, :]).sum(1) for a in range(3)], 1) + 0.0
        for a in range(16):
            if a < c.nout and a < 3:
                v = part[:mm, a]
                if c.b2 is not None and mut != "fwd2_b2_skipped":
                    v = v + float(c.b2[a])
                if c.relu_out:
                    v = np.where(v > 0.0, v, np.where(np.isnan(v), NAN, 0.0))
                Q[m0:m0 + mm, a] = v
            elif mut != "fwd2_q_pad":
                Q[m0:m0 + mm, a] = 0.0
    return Hb, Q


def check_fwd2(c: Fwd2Case, H_flat, Q):
    """H_flat: the M * N1 values and whatever follows them in the buffer (must stay NaN).  -> (differences, worst
    err / bound of H, of Q)."""
    h, q, bh, bq = fwd2_ref(c)
    n = c.M * c.N1
    tail = np.asarray(H_flat)[n:]
    d = check_bits(tail, np.full(tail.size, NAN, F))
    Hg = np.asarray(H_flat)[:n].reshape(c.M, c.N1)
    if c.exact:
        return d + check_bits(Hg, h.astype(F)) + check_bits(Q, q.astype(F)), 0.0, 0.0
    d1, r1 = check_bound(Hg, h, bh, np.ones(h.shape, bool))
    live = np.zeros(q.shape, bool)
    live[:, :c.nout] = True
    d2, r2 = check_bound(Q, q, bq, live)
    return d + d1 + d2, r1, r2


# ----------------------------------------------------------------------------- column sums
@dataclass
class ColsumCase:
    name: str
    E: int
    N: int
    D: Region
    out_off: int         # floats in front of ``out`` (1: misaligned)
    exact: bool
    vec: bool            # the form the launcher must take (asserted)
    prior: np.ndarray


def colsum_part_floats(E, N):
    """st_f32b_colsum_part_floats."""
    return 32 * 256 if (N % 4 == 0 and N <= 256) else -(-E // 256) * N


def colsum_form(c: ColsumCase, det, base_addr=0):
    al = lambda off: (base_addr + 4 * off) % 16 == 0
    return (c.N % 4 == 0 and c.N <= 256 and c.D.sr % 4 == 0 and al(c.D.off) and (not det or al(c.out_off)))


def make_colsum(name, E, N, ld, d_off=0, out_off=0, exact=True, seed=0):
    g = np.random.default_rng(seed)
    D = Region(E, N, ld, 1, off=d_off, tail=ld - N)
    D.put(g.integers(-8, 9, (E, N)) if exact else g.standard_normal((E, N)))
    prior = (g.integers(-64, 65, N) if exact else g.standard_normal(N)).astype(F)
    c = ColsumCase(name, E, N, D, out_off, exact, False, prior)
    c.vec = bool(colsum_form(c, det=False))
    if exact and sum_bits(np.r_[D.get(), prior[None, :].astype(np.float64)]) >= LIMIT_BITS:
        raise AssertionError(f"colsum case {name}: not exact in fp32")
    return c


_COLSUM = None


def colsum_cases():
    global _COLSUM
    if _COLSUM is None:
        out = []
        for i, E in enumerate((1, 5, 127, 128, 129, 1000)):
            N = (4, 16, 200, 256)[i % 4]
            out.append(make_colsum(f"vec-E{E}-N{N}", E, N, N + 4 * (1 + i % 2), seed=100 + i))
        out.append(make_colsum("vec-E1000-N4", 1000, 4, 8, seed=106))
        out.append(make_colsum("vec-E129-N16", 129, 16, 20, seed=107))
        for i, E in enumerate((1, 255, 256, 257, 600)):
            N = (3, 203, 260, 520)[i % 4]
            out.append(make_colsum(f"fb-E{E}-N{N}", E, N, N + 1 + i % 3, seed=110 + i))
        out.append(make_colsum("fb-E600-N520", 600, 520, 524, seed=115))
        out.append(make_colsum("fb-ld-E257-N16", 257, 16, 19, seed=116))              # ld % 4 != 0
        out.append(make_colsum("fb-Doff-E600-N16", 600, 16, 20, d_off=1, seed=117))   # D misaligned
        out.append(make_colsum("fb-outoff-E255-N200", 255, 200, 204, out_off=1, seed=118))   # out misaligned (det)
        out.append(make_colsum("gauss-vec-E1000-N200", 1000, 200, 204, exact=False, seed=120))
        out.append(make_colsum("gauss-fb-E600-N203", 600, 203, 205, exact=False, seed=121))
        _COLSUM = out
    return _COLSUM


def colsum_ref(c: ColsumCase, det):
    """(out [N] float64, bound): the atomic entry adds to the prior ``out``, the deterministic entry overwrites."""
    D = c.D.get()
    s = D.sum(0) + 0.0
    if det:
        return s, gamma(c.E) * np.abs(D).sum(0) + U * np.abs(s)
    pr = c.prior.astype(np.float64)
    return s + pr, gamma(c.E + 1) * (np.abs(D).sum(0) + np.abs(pr)) + U * np.abs(s + pr)


def colsum_model(c: ColsumCase, det, mut=None, base_addr=0):
    """(out [N] fp32, part flat fp32 of st_f32b_colsum_part_floats floats -- NaN where untouched --, nparts)."""
    E, N, ld = c.E, c.N, c.D.sr
    part = np.full(colsum_part_floats(E, N), NAN, F)
    rows_of = []
    if colsum_form(c, det, base_addr):
        rpi = 256 // (N // 4)
        rows = max(_rup(-(-E // 32), rpi), 4 * rpi)
        nb = -(-E // rows)
        for b in range(nb):
            e0, e1 = b * rows, min(E, b * rows + rows)
            grp = [np.arange(e0 + rg, e1, rpi) for rg in range(rpi)]
            if mut == "colsum_last_group":
                grp = grp[:-1]
            rows_of.append(np.concatenate(grp).astype(np.int64))
    else:
        nb = -(-E // 256)
        for b in range(nb):
            rows_of.append(np.arange(b * 256, min(E, b * 256 + 256)))
        if mut == "colsum_last_group":
            rows_of[-1] = rows_of[-1][:0]
    sums = [rd(c.D.flat, c.D.off + r[:, None] * ld + np.arange(N)[None, :]).sum(0) + 0.0 for r in rows_of]
    out = c.prior.astype(np.float64).copy()
    if det:
        for b, s in enumerate(sums):
            part[b * N:(b + 1) * N] = s
        tot = splitsum_model(part, nb, N, N, one=(N % 4 != 0 or (base_addr + 4 * c.out_off) % 16 != 0))
        out = out + tot if mut == "colsum_det_adds" else tot
    else:
        for s in sums:
            out = out + s
    return out.astype(F), part, nb


def check_colsum(c: ColsumCase, det, out, part=None, nparts=None):
    ref, bound = colsum_ref(c, det)
    if c.exact:
        d = check_bits(out, ref.astype(F))
    else:
        d = check_bound(out, ref, bound, np.ones(c.N, bool))[0]
    if part is not None:
        n = nparts * c.N
        if n > colsum_part_floats(c.E, c.N):
            return d + 1
        p = np.asarray(part)
        d += check_bits(p[n:], np.full(p.size - n, NAN, F))   # nothing beyond the blocks' rows
        if c.exact:   # the blocks' rows add up to the column sums
            d += check_bits((p[:n].astype(np.float64).reshape(nparts, c.N).sum(0) + 0.0).astype(F),
                            colsum_ref(c, True)[0].astype(F))
        else:
            d += int(np.isnan(p[:n]).sum())
    return d


# ----------------------------------------------------------------------------- split sums
@dataclass
class SplitsumCase:
    name: str
    splits: int
    n: int
    zstride: int
    part_off: int
    out_off: int
    exact: bool
    part: np.ndarray     # flat, NaN in the gaps, ``part_off`` floats in front
    one: bool            # the one-element form (asserted against the launcher's rule)


def make_splitsum(name, splits, n, zstride, part_off=0, out_off=0, exact=True, seed=0):
    g = np.random.default_rng(seed)
    R = Region(splits, n, zstride, 1, off=part_off, tail=zstride - n)
    R.put(g.integers(-64, 65, (splits, n)) if exact else g.standard_normal((splits, n)))
    one = bool(n % 4 or zstride % 4 or part_off % 4 or out_off % 4)
    c = SplitsumCase(name, splits, n, zstride, part_off, out_off, exact, R.flat, one)
    if exact and sum_bits(R.get()) >= LIMIT_BITS:
        raise AssertionError(f"splitsum case {name}: not exact in fp32")
    return c


def splitsum_dense(c: SplitsumCase):
    return c.part[c.part_off + np.arange(c.splits)[:, None] * c.zstride + np.arange(c.n)[None, :]].astype(np.float64)


_SPLITSUM = None


def splitsum_cases():
    global _SPLITSUM
    if _SPLITSUM is None:
        out = []
        ns = (4, 60, 64, 68, 160)
        for i, sp in enumerate((1, 2, 15, 16, 17, 63, 64, 65, 130)):
            n = ns[i % 5]
            out.append(make_splitsum(f"f4-s{sp}-n{n}", sp, n, n + 4 * (1 + i % 3), seed=200 + i))
        out.append(make_splitsum("f4-s130-n160", 130, 160, 164, seed=209))
        for i, n in enumerate((1, 3, 203)):
            out.append(make_splitsum(f"one-n{n}", (17, 2, 65)[i], n, n + 1 + i, seed=210 + i))
        out.append(make_splitsum("one-zstride", 17, 64, 70, seed=213))               # zstride % 4 != 0
        out.append(make_splitsum("one-partoff", 16, 64, 68, part_off=1, seed=214))   # misaligned part
        out.append(make_splitsum("one-outoff", 65, 60, 64, out_off=1, seed=215))     # misaligned out
        out.append(make_splitsum("gauss-f4-s130-n160", 130, 160, 164, exact=False, seed=216))
        out.append(make_splitsum("gauss-one-s65-n203", 65, 203, 205, exact=False, seed=217))
        _SPLITSUM = out
    return _SPLITSUM


def splitsum_model(part, splits, zstride, n, one, off=0, mut=None):
    """out [n] float64 by the kernels' indexing: the float4 form (16 split groups: a 64-stride main loop, a 16-stride
    tail, the LDS fold in group order) or the one-element form."""
    part = np.asarray(part)
    i = np.arange(n)
    if one:
        zs = n if mut == "splitsum1_n_for_zstride" else zstride
        return sum((rd(part, off + z * zs + i) for z in range(splits)), np.zeros(n)) + 0.0
    tot = np.zeros(n)
    for g in range(16):
        a = np.zeros(n)
        z = g
        while z + 48 < splits:
            for zz in (z, z + 16, z + 32, z + 48):
                a = a + rd(part, off + zz * zstride + i)
            z += 64
        while z < (splits // 16 * 16 if mut == "splitsum_tail16" else splits):
            a = a + rd(part, off + z * zstride + i)
            z += 16
        tot = tot + a
    return tot + 0.0


def check_splitsum(c: SplitsumCase, out):
    P = splitsum_dense(c)
    ref = P.sum(0) + 0.0
    if c.exact:
        return check_bits(out, ref.astype(F)), 0.0
    return check_bound(out, ref, gamma(c.splits) * np.abs(P).sum(0) + U * np.abs(ref), np.ones(c.n, bool))


# ----------------------------------------------------------------------------- env side: gather, env, td
@dataclass
class BatchCase:
    name: str
    E: int
    H: int
    in_p: int
    bias_col: int
    T: int
    k: Dict[str, object]
    prices: np.ndarray
    state: Dict[str, np.ndarray]
    Q: np.ndarray
    QN: np.ndarray
    QT: Optional[np.ndarray]
    scr: Dict[str, np.ndarray]      # the scratch the TD launch is given (its own test: not the env model's output)
    stat0: np.ndarray

    def knobs_for_rule(self):
        return dict(compat=bool(self.k["compat_env"]), budget0=float(self.k["b0"]), shares0=int(self.k["s0"]))


REWARD_MODES = ("absolute", "relative", "growth")
STATE_KEYS = ("budget", "shares", "value", "pos", "episodes", "last_final", "ret_sum")
Q_PALETTE = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [0, 0, 0], [-1, -1, -2], [2, 1, 0], [0, 2, 1],
                      [0, 1, 2]], np.float64)


def default_bknobs(**kw):
    k = dict(feat_mode=1, compat_env=0, target_compat=0, output_relu=0, s0=0, env_offset=0, reward_mode=0, eps=0.5,
             ramp=4.0, b0=4096.0, gamma=0.5, coef=0.25, td_clip=0.0, seed=1234, step=5, reward_scale=1.0,
             double_dqn=0, ramp_global=0, use_qt=False, stat=True, actions_out=True, rewards_out=True, dyadic=True)
    k.update(kw)
    k["inv_ramp"] = float(F(1.0 / k["ramp"]))
    k["inv_b0"] = float(F(1.0 / k["b0"]))
    return k


def make_batch(name, E, small, seed=0, **kw):
    """One env-side case.  Geometry: small (H 5, in_p 8, bias column 7, T 12) or the reference's (H 201, in_p 208,
    bias column 203, T 260).  Positions are mixed and include the last legal one (T - H - 1: the episode ends) and
    the one before it; budgets include some below and some equal to the next price, shares include 0, and with a
    relative reward some portfolios are worth 0.  Q rows come from Q_PALETTE (two-way and three-way ties)."""
    g = np.random.default_rng(5000 + seed)
    k = default_bknobs(**kw)
    H, in_p, bias_col, T = (5, 8, 7, 12) if small else (201, 208, 203, 260)
    e = np.arange(E)
    last = T - H - 1
    pos = (e * 5 + e // 7) % (last + 1)
    pos = np.where(e % 6 == 1, last, np.where(e % 6 == 4, last - 1, pos))
    if E == 1:
        pos = np.array([last])
    if k["dyadic"]:
        prices = (g.integers(1, 9, (E, T)) * 16.0).astype(F)
    else:
        prices = (50.0 * np.exp(0.1 * g.standard_normal((E, T)))).astype(F)
    vnew = prices[e, pos + H].astype(np.float64)
    budget = (g.integers(1, 5, E) * 2048.0) if k["dyadic"] else (4096.0 * g.random(E) + 100.0)
    budget = np.where(e % 5 == 1, vnew, np.where(e % 5 == 3, vnew * 0.5, budget))
    shares = np.where(e % 4 == 2, 0, g.integers(0, 4, E))
    if k["reward_mode"]:
        budget = np.where(e % 8 == 5, 0.0, budget)
        shares = np.where(e % 8 == 5, 0, shares)
    value = vnew + (g.integers(-2, 3, E) * 0.5 if k["dyadic"] else g.standard_normal(E))
    st = dict(budget=budget.astype(F), shares=shares.astype(np.int32), value=value.astype(F), pos=pos.astype(np.int32),
              episodes=(e % 3).astype(np.int32), last_final=np.full(E, -7.0, F),
              ret_sum=(g.integers(-4, 5, E) * 0.5).astype(F))
    Q = np.zeros((E, 16))
    QN = np.zeros((E, 16))
    Q[:, :3] = Q_PALETTE[(e + seed) % len(Q_PALETTE)]
    QN[:, :3] = Q_PALETTE[(e * 2 + 1 + seed) % len(Q_PALETTE)]
    if k["dyadic"]:
        Q[:, :3] += (g.integers(-1, 2, E) * 0.5)[:, None]
        QN[:, :3] *= 0.5
    else:
        rnd = e % 3 == 2   # every third env: untied Gaussian rows
        Q[rnd, :3] = g.standard_normal((int(rnd.sum()), 3))
        QN[rnd, :3] = g.standard_normal((int(rnd.sum()), 3))
    if k["output_relu"]:   # qs of +0, -0, negative and positive under the output ReLU's mask
        Q[e % 9 == 0, :3] = 0.0
        Q[e % 9 == 1, :3] = -0.0
        Q[e % 9 == 2, :3] = -1.5
    Q[:, 3:], QN[:, 3:] = NAN, NAN           # only the three action columns may be read
    QT = None
    if k["use_qt"]:
        QT = np.full((E, 16), NAN)
        QT[:, :3] = Q_PALETTE[(e * 4 + 3 + seed) % len(Q_PALETTE)][:, ::-1] * (0.25 if k["dyadic"] else 0.37)
    if k["dyadic"]:
        rew = g.integers(-16, 17, E) * 0.25
    else:
        rew = g.standard_normal(E)
    if k["td_clip"] > 0:   # errors on both sides of the clip
        rew = np.where(e % 3 == 0, rew + 8.0 * k["td_clip"], np.where(e % 3 == 1, rew - 8.0 * k["td_clip"], rew * 0.125))
    scr = dict(s_b2=(budget + g.integers(-2, 3, E) * 16.0).astype(F), s_s2=(shares + g.integers(0, 2, E)).astype(np.int32),
               s_rew=rew.astype(F), s_act=g.integers(0, 3, E).astype(np.int32))
    return BatchCase(name, E, H, in_p, bias_col, T, k, prices, st, Q.astype(F), QN.astype(F),
                     None if QT is None else QT.astype(F), scr, np.array([1000.5, -17.25]))


_BATCH = None


def batch_cases():
    """E in {1, 255, 257, 1025} x the two geometries; the knobs rotate so that every flag of the env and TD launches
    is on in some case and off in another (``batch_coverage`` says which case shows what)."""
    global _BATCH
    if _BATCH is None:
        kn = [
            dict(feat_mode=1, stat=True),
            dict(feat_mode=0, compat_env=1, s0=1, target_compat=1, output_relu=1, reward_mode=1, env_offset=77,
                 use_qt=True, reward_scale=0.5, td_clip=2.0),
            dict(feat_mode=1, reward_mode=2, ramp_global=1, step=2 ** 32 + 3, double_dqn=1, use_qt=True,
                 actions_out=False, stat=False, dyadic=False, reward_scale=0.37, td_clip=0.75, env_offset=1025),
            dict(feat_mode=0, reward_mode=1, step=2 ** 33 + 7, use_qt=True, rewards_out=False, output_relu=1,
                 dyadic=False, stat=False, env_offset=5),
            dict(feat_mode=1, ramp_global=1, step=2, double_dqn=1, use_qt=True, reward_scale=2.0, env_offset=3000),
            dict(feat_mode=0, target_compat=1, td_clip=1.0, reward_mode=2, stat=True, eps=1.0, ramp=1.0),
            dict(feat_mode=1, compat_env=1, s0=0, dyadic=False, stat=False, td_clip=0.0, output_relu=1, eps=1.0,
                 ramp=2.0),
            dict(feat_mode=0, reward_mode=0, step=2 ** 32 + 1, env_offset=9, double_dqn=1, use_qt=True, stat=True,
                 reward_scale=0.5),
        ]
        out = []
        i = 0
        for E in (1, 255, 257, 1025):
            for small in (True, False):
                out.append(make_batch(f"E{E}-{'small' if small else 'ref'}-k{i}", E, small, seed=i, **kn[i]))
                i += 1
        _BATCH = out
    return _BATCH


def _feat_budget(b, k):
    return r32(b * k["inv_b0"]) if k["feat_mode"] else np.asarray(b, np.float64)


def _feat_shares(s, last, k):
    return r32(r32(s * last) * k["inv_b0"]) if k["feat_mode"] else np.asarray(s, np.float64)


def gather_model(c: BatchCase, mut=None):
    """(X, XN) [E, in_p] float64: the fp32 op-by-op features of csrc/trade_rule.h, every column, zero pad included;
    the budget / shares columns of x' are left 0 for the env launch."""
    k, st = c.k, c.state
    E, H = c.E, c.H
    pos = st["pos"].astype(np.int64)
    idx = pos[:, None] + np.arange(H + 1)[None, :]
    win = np.take_along_axis(c.prices.astype(np.float64), idx, 1)
    last, vnew = win[:, H - 1], win[:, H]
    X = np.zeros((E, c.in_p))
    XN = np.zeros((E, c.in_p))
    wn = win[:, :H] if mut == "xn_not_shifted" else win[:, 1:H + 1]
    if k["feat_mode"]:
        X[:, :H] = r32(r32(win[:, :H] * r32(1.0 / last)[:, None]) - 1.0)
        XN[:, :H] = r32(r32(wn * r32(1.0 / vnew)[:, None]) - 1.0)
    else:
        X[:, :H], XN[:, :H] = win[:, :H], wn
    X[:, H] = _feat_budget(st["budget"].astype(np.float64), k)
    X[:, H + 1] = _feat_shares(st["shares"].astype(np.float64), last, k)
    if mut != "no_bias_col":
        X[:, c.bias_col] = 1.0
        XN[:, c.bias_col] = 1.0
    return X, XN


def argmax_first(q):
    return np.argmax(q[:, :3], axis=1)


def argmax_last(q):
    return 2 - np.argmax(q[:, 2::-1], axis=1)


def env_model(c: BatchCase, mut=None):
    """The env launch: the draw (Philox mirror of sharetrade/utils/rng), the exploit ramp, the trade and the reward of
    step_refs' fp32 op-by-op rule.  -> dict of everything the launch writes, plus exploit / greedy / rnd."""
    k, st = c.k, c.state
    E, H = c.E, c.H
    e = np.arange(E)
    step = int(k["step"])
    off = 0 if mut == "no_env_offset" else int(k["env_offset"])
    ids = ((off + e) & 0xFFFFFFFF).astype(np.uint32)
    u1, u2 = strng.uniforms(k["seed"], 0, ids, step & 0xFFFFFFFF if mut == "step_hi_ignored" else step)
    pos = st["pos"].astype(np.int64)
    rpos = np.full(E, F(step), F) if k["ramp_global"] else pos.astype(F)
    thr = np.minimum(F(k["eps"]), rpos * F(k["inv_ramp"]))
    exploit = (u2 if mut == "u2_exploit" else u1) < thr
    q = c.Q.astype(np.float64)
    greedy = argmax_last(q) if mut == "tie_last" else argmax_first(q)
    rnd = np.minimum((u2 * F(3.0)).astype(np.int64), 2)
    a = np.where(exploit, greedy, rnd)
    vnew = c.prices[e, pos + H].astype(np.float64)
    b, s, vprev = (st[n].astype(np.float64) for n in ("budget", "shares", "value"))
    b2, s2 = trade(a, b, s, vnew, c.knobs_for_rule())
    rew = reward(b, s, vprev, b2, s2, vnew, REWARD_MODES[k["reward_mode"]])
    return dict(s_b2=b2, s_s2=s2.astype(np.int64), s_rew=rew, s_act=a, xn_budget=_feat_budget(b2, k),
                xn_shares=_feat_shares(s2, vnew, k), exploit=exploit, greedy=greedy, rnd=rnd, u1=u1, u2=u2, vnew=vnew)


def td_model(c: BatchCase, mut=None):
    """The TD launch from the given Q, QN, QT and scratch: DQ [E, 16], loss, the new state, the statistics."""
    k, st, E = c.k, c.state, c.E
    rows = np.arange(E)
    qn3 = c.QN.astype(np.float64)[:, :3]
    am = argmax_first(qn3)
    boot = qn3[rows, am]
    act = c.scr["s_act"].astype(np.int64)
    slot = am if k["target_compat"] else act
    rew = c.scr["s_rew"].astype(np.float64)
    if c.QT is not None:
        qt = c.QT.astype(np.float64)[:, :3]
        if k["target_compat"] or k["double_dqn"]:
            boot = qt[rows, argmax_first(qt) if mut == "ddqn_target_argmax" else am]
        else:
            boot = qt.max(1)
    rs = r32(rew * float(F(k["reward_scale"]))) if float(F(k["reward_scale"])) != 1.0 else rew
    y = r32(rs + r32(float(F(k["gamma"])) * boot))
    qs = c.Q.astype(np.float64)[rows, slot]
    diff = r32(qs - y)
    clip = float(F(k["td_clip"]))
    d = np.clip(diff, -clip, clip) if clip > 0 else diff
    dqv = r32(float(F(k["coef"])) * d)
    if k["output_relu"]:
        dqv = np.where(qs > 0, dqv, 0.0)
    DQ = np.zeros((E, 16))
    DQ[rows, slot] = dqv
    dl = d if mut == "loss_from_clipped" else diff
    loss = r32(dl * dl)
    b2, s2 = c.scr["s_b2"].astype(np.float64), c.scr["s_s2"].astype(np.int64)
    pos = st["pos"].astype(np.int64)
    vnew = c.prices[rows, pos + c.H].astype(np.float64)
    np_ = pos + 1
    done = (np_ > c.T - c.H) if mut == "td_reset_late" else (np_ >= c.T - c.H)
    srew = rs if mut == "scale_stored_reward" else rew
    ns = dict(
        budget=np.where(done, k["b0"], b2), shares=np.where(done, k["s0"], s2), value=np.where(done, 0.0, vnew),
        pos=np.where(done, 0, np_), episodes=st["episodes"].astype(np.int64) + done,
        last_final=np.where(done, r32(b2 + r32(s2 * vnew)), st["last_final"].astype(np.float64)),
        ret_sum=np.where(done, 0.0, r32(st["ret_sum"].astype(np.float64) + srew)))
    stat = c.stat0 + np.array([srew.sum(), loss.sum()])
    return dict(DQ=DQ, loss=loss, state=ns, stat=stat, slot=slot, diff=diff, qs=qs, done=done, am=am, clip=clip)


def stat_bits(c: BatchCase):
    """Bits the two double sums of the statistics need (53 available): the terms are fp32 values."""
    t = td_model(c)
    return max(sum_bits(np.r_[c.scr["s_rew"].astype(np.float64), c.stat0[0]][:, None]),
               sum_bits(np.r_[t["loss"], c.stat0[1]][:, None]))


def batch_coverage(c: BatchCase):
    """What a case shows, counted on the models (as tests/test_oracle.py rule_coverage does for the oracle)."""
    k, st = c.k, c.state
    ev, td = env_model(c), td_model(c)
    q3 = np.sort(c.Q.astype(np.float64)[:, :3], 1)
    ex, a = ev["exploit"], ev["s_act"]
    kr = c.knobs_for_rule()
    bd = np.full(c.E, kr["budget0"]) if kr["compat"] else st["budget"].astype(np.float64)
    sd = np.full(c.E, kr["shares0"]) if kr["compat"] else st["shares"]
    cur = st["budget"].astype(np.float64) + st["shares"] * st["value"].astype(np.float64)
    out = dict(
        tie2=int((ex & (q3[:, 2] == q3[:, 1]) & (q3[:, 1] > q3[:, 0])).sum()),
        tie3=int((ex & (q3[:, 2] == q3[:, 0])).sum()), exploit=int(ex.sum()), explore=int((~ex).sum()),
        rnd0=int((~ex & (a == 0)).sum()), rnd1=int((~ex & (a == 1)).sum()), rnd2=int((~ex & (a == 2)).sum()),
        buy_uncovered=int(((a == 0) & (bd < ev["vnew"])).sum()), sell_no_shares=int(((a == 1) & (sd <= 0)).sum()),
        cur_not_positive=int((cur <= 0).sum()) if k["reward_mode"] else 0,
        last_pos=int((st["pos"] == c.T - c.H - 1).sum()), before_last=int((st["pos"] == c.T - c.H - 2).sum()),
        clip_hi=int((td["diff"] > td["clip"]).sum()) if td["clip"] > 0 else 0,
        clip_lo=int((td["diff"] < -td["clip"]).sum()) if td["clip"] > 0 else 0,
        clip_in=int((np.abs(td["diff"]) < td["clip"]).sum()) if td["clip"] > 0 else 0)
    if k["output_relu"]:
        b = bits32(td["qs"].astype(F))
        out.update(qs_pzero=int((b == 0).sum()), qs_nzero=int((b == 0x80000000).sum()),
                   qs_neg=int((td["qs"] < 0).sum()), qs_pos=int((td["qs"] > 0).sum()))
    return out


def check_gather(c: BatchCase, X, XN):
    x, xn = gather_model(c)
    return check_bits(X, x.astype(F)) + check_bits(XN, xn.astype(F))


def check_env(c: BatchCase, got):
    """got: s_b2, s_s2, s_rew, s_act, XN [E, in_p] (after gather + env), optional actions_out / rewards_out."""
    ev = env_model(c)
    _, xn = gather_model(c)
    xn[:, c.H], xn[:, c.H + 1] = ev["xn_budget"], ev["xn_shares"]
    d = check_bits(got["s_b2"], ev["s_b2"].astype(F)) + check_bits(got["s_rew"], ev["s_rew"].astype(F))
    d += check_int(got["s_s2"], ev["s_s2"])[0] + check_int(got["s_act"], ev["s_act"])[0]
    d += check_bits(got["XN"], xn.astype(F))
    if "actions_out" in got:
        d += check_int(got["actions_out"], ev["s_act"])[0]
    if "rewards_out" in got:
        d += check_bits(got["rewards_out"], ev["s_rew"].astype(F))
    return d


def check_td(c: BatchCase, got):
    """got: DQ, loss, state (dict), optional stat [2] float64."""
    td = td_model(c)
    d = check_bits(got["DQ"], td["DQ"].astype(F)) + check_bits(got["loss"], td["loss"].astype(F))
    for n in STATE_KEYS:
        ref = td["state"][n]
        if c.state[n].dtype == np.int32:
            d += check_int(got["state"][n], ref)[0]
        else:
            d += check_bits(got["state"][n], np.asarray(ref, np.float64).astype(F))
    if "stat" in got:
        d += int((np.asarray(got["stat"], np.float64).view(np.uint64) != td["stat"].view(np.uint64)).sum())
    return d


def env_outputs(c: BatchCase, mut=None):
    """What a kernel computing the (mutated) models would leave behind, in check_env's form."""
    ev = env_model(c, mut)
    _, xn = gather_model(c, mut)
    xn[:, c.H], xn[:, c.H + 1] = ev["xn_budget"], ev["xn_shares"]
    return dict(s_b2=ev["s_b2"].astype(F), s_s2=ev["s_s2"], s_rew=ev["s_rew"].astype(F), s_act=ev["s_act"],
                XN=xn.astype(F), actions_out=ev["s_act"], rewards_out=ev["s_rew"].astype(F))


def td_outputs(c: BatchCase, mut=None):
    td = td_model(c, mut)
    return dict(DQ=td["DQ"].astype(F), loss=td["loss"].astype(F), stat=td["stat"],
                state={n: (v.astype(F) if c.state[n].dtype == F else v) for n, v in td["state"].items()})


# ----------------------------------------------------------------------------- target sync
SYNC_CASES = [(n, every, c0) for n in (1, 255, 257) for every in (1, 3) for c0 in (0, 2, 3, 6, 2 ** 32 + 1)]


def sync_model(params, target, every, ctrl0, mut=None):
    c = ctrl0 + 1 if mut == "sync_plus_one" else ctrl0
    return params.copy() if c % every == 0 else target.copy()


def check_sync(params, target, every, ctrl0, got):
    return check_bits(got, params if ctrl0 % every == 0 else target)


# ----------------------------------------------------------------------------- optimizer, mode 2
OPT_LR, OPT_B1, OPT_B2, OPT_EPS = 1e-2, 0.9, 0.999, 1e-8


def optim_ref(kind, w, mask, s1, s2, g, t, scale):
    """One mode-2 update in float64 from fp32 inputs (hyper-parameters as the kernel receives them: fp32).
    -> (w', s1', s2', bound_w, bound_s1, bound_s2); for Adam bound_w is B_adam (module docstring)."""
    lr, b1, b2, eps, sc = (float(F(x)) for x in (OPT_LR, OPT_B1, OPT_B2, OPT_EPS, scale))
    w, mask, s1, s2, g = (np.asarray(x, F).astype(np.float64) for x in (w, mask, s1, s2, g))
    live = mask != 0
    gp = g * (mask * sc)
    z = np.zeros_like(w)
    if kind == 1:
        a = s1 + gp * gp
        upd = lr * gp / np.sqrt(np.where(live, a, 1.0))
        w2 = w - upd
        out = (w2, a, s2, gamma(8) * np.abs(upd) + U * np.abs(w2), gamma(6) * a, z)
    elif kind == 2:
        c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        m = b1 * s1 + (1.0 - b1) * gp
        v = b2 * s2 + (1.0 - b2) * gp * gp
        den = np.sqrt(v / c2) + eps
        upd = lr * (m / c1) / den
        em = gamma(5) * (np.abs(b1 * s1) + np.abs((1.0 - b1) * gp))
        w2 = w - upd
        out = (w2, m, v, gamma(11) * np.abs(upd) + np.abs(lr / (c1 * den)) * em + U * np.abs(w2), em,
               gamma(8) * v)
    else:
        upd = lr * gp
        w2 = w - upd
        out = (w2, s1, s2, gamma(3) * np.abs(upd) + U * np.abs(w2), z, z)
    keep = lambda new, old: np.where(live, new, old)
    return (keep(out[0], w), keep(out[1], s1), keep(out[2], s2), out[3], out[4], out[5])
