"""Host references, case lists and a tiling model for the bf16 GEMMs of csrc/gemm_bf16.hip (no GPU; numpy float64).

tests/test_gpu_gemm_refs.py launches the committed cases on the GPU and compares with these references through the
``check_*`` functions below; tests/test_gemm_refs.py runs a numpy model of the kernels' tiling through the same
functions, unmutated (0 differences) and with one mutation at a time (> 0).

Exact cases: A and B are integers in [-8, 8], alpha is 1, 0.5 or 0.25, bias and prior outputs are integers in
[-64, 64].  Every fp32 partial sum is then a multiple of 2^-2 below 2^24 in magnitude, so fp32 arithmetic is exact in
any order and the kernel's output must equal the float64 reference bit for bit, whatever the MFMA's internal order,
the K split or the order of the atomics.  ``assert_exact`` checks that precondition per case; it is not assumed.
Gaussian cases (full-mantissa bf16 operands) are compared within a per-element bound instead (``gauss_bound``).

Everything bf16 is carried on the host as uint16 bit patterns; ``bf16_rne`` rounds from float64 itself."""
import numpy as np

F = np.float32
GBK = 64
EPI_BF16, EPI_RELU_GRAD, EPI_F32 = 0, 1, 2
LIM = 2.0 ** 22   # multiples of 2^-2 below 2^22 are exact in fp32 (integers: below 2^24)


# ----------------------------------------------------------------------------- tiles
class Geo:
    """One st_gemm_nt tile id: block tile, wave grid, LDS stages, kernel family."""

    def __init__(self, tid, BM, BN, NWM, NWN, S, has_t, kind, key):
        self.id, self.BM, self.BN, self.NWM, self.NWN, self.S = tid, BM, BN, NWM, NWN, S
        self.has_t, self.kind, self.key = has_t, kind, key
        self.WM, self.WN = BM // NWM, BN // NWN


TILES = {g.id: g for g in (
    Geo(0, 128, 128, 2, 2, 2, True, "body", (128, 128)),
    Geo(1, 64, 64, 2, 2, 2, True, "body", (64, 64)),
    Geo(2, 128, 64, 2, 2, 2, True, "body", (128, 64)),
    Geo(3, 256, 128, 4, 2, 2, True, "body", (256, 128)),
    Geo(4, 128, 128, 2, 2, 3, True, "body", (128, 128, 3)),
    Geo(5, 128, 128, 2, 2, 4, True, "body", (128, 128, 4)),
    Geo(6, 256, 256, 2, 2, 2, False, "body", (256, 256)),
    Geo(7, 256, 256, 2, 4, 0, False, "pp", (256, 256, "pp")),
    Geo(8, 256, 256, 2, 4, 0, False, "pp", (256, 256, "ppp")),
    Geo(9, 256, 256, 2, 2, 0, False, "w4", (256, 256, "w4")),
)}
BODY_TILES = (0, 1, 2, 3, 4, 5, 6)
BIG_TILES = (7, 8, 9)


# ----------------------------------------------------------------------------- bf16
def bf16_round64(x) -> np.ndarray:
    """float64 -> the nearest bf16 value (ties to even) in one rounding, as float64."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.rint(x / q) * q


def _val_bits(v) -> np.ndarray:
    """The high 16 bits of the fp32 form: the bit patterns of values that already are bf16 values."""
    return (np.ascontiguousarray(v, dtype=F).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_rne(x) -> np.ndarray:
    """float64 -> bf16 bit patterns, round to nearest even."""
    return _val_bits(bf16_round64(x))


def bf16_trunc(x) -> np.ndarray:
    """float64 (exact in fp32) -> bf16 bit patterns by dropping the low 16 bits: a mutation."""
    return _val_bits(x)


def bf16_val(bits) -> np.ndarray:
    """bf16 bit patterns -> values (float64)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F).astype(np.float64)


# ----------------------------------------------------------------------------- operand makers (seeded, host)
def int_bits(shape, seed, lo=-8, hi=8) -> np.ndarray:
    """Integers uniform in [lo, hi] as bf16 bit patterns (exact: |v| <= 256)."""
    g = np.random.default_rng(seed)
    return bf16_rne(g.integers(lo, hi + 1, shape).astype(np.float64))


def int_vals(shape, seed, lo=-64, hi=64) -> np.ndarray:
    """Integers uniform in [lo, hi] (fp32 bias / prior output)."""
    return np.random.default_rng(seed).integers(lo, hi + 1, shape).astype(np.float64)


def gauss_bits(shape, seed) -> np.ndarray:
    """Standard normal values rounded to bf16: full-mantissa operands."""
    return bf16_rne(np.random.default_rng(seed).standard_normal(shape))


# relu-grad activations: exact zeros, -0.0, the smallest bf16 subnormals of both signs, +inf, +-1
ACT_PALETTE = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0x3F80, 0xBF80], dtype=np.uint16)
ACT_PROB = (0.30, 0.10, 0.06, 0.06, 0.02, 0.23, 0.23)
ACT_KNOWN = {(0, 0): 0x0000, (0, 1): 0x8000, (1, 0): 0x0001, (1, 1): 0x8001, (2, 2): 0x7F80, (3, 1): 0x3F80}


def act_bits(M, N, seed) -> np.ndarray:
    """The forward activation [M, N] (bit patterns) the relu-grad mask is built from; ACT_KNOWN positions are
    fixed, the rest drawn from ACT_PALETTE.  The kernel reads its transposed copy."""
    g = np.random.default_rng(seed)
    a = ACT_PALETTE[g.choice(len(ACT_PALETTE), size=(M, N), p=ACT_PROB)]
    for (m, n), b in ACT_KNOWN.items():
        a[m, n] = b
    return a


# ----------------------------------------------------------------------------- references
def acc_ref(A_bits, B_bits) -> np.ndarray:
    """A . B^T in float64: one matmul."""
    return bf16_val(A_bits) @ bf16_val(B_bits).T


def ref_bf16(acc, alpha=1.0, bias=None, relu=False) -> np.ndarray:
    """EPI_BF16 before the store's rounding: act(alpha * acc + bias[n]) in float64; the stored bits are
    bf16_rne of it."""
    x = alpha * acc + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :acc.shape[1]])
    return np.maximum(x, 0.0) if relu else x


def ref_relu_grad(acc, act, WM):
    """EPI_RELU_GRAD: out = acc where float(act) > 0 else 0, stored bf16; outT its transpose; colpart[M / WM, N]
    the sums of the stored values over each wave's WM rows.  Returns (out bits, outT bits, colpart)."""
    M, N = acc.shape
    bits = bf16_rne(np.where(bf16_val(act) > 0.0, acc, 0.0))
    cp = bf16_val(bits).reshape(M // WM, WM, N).sum(1)
    return bits, np.ascontiguousarray(bits.T), cp


def ref_f32(acc, alpha=1.0, bias=None, prior=None) -> np.ndarray:
    """EPI_F32: alpha * acc + bias[n] (+ the prior output when accumulating), whatever the K split."""
    x = alpha * acc + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :acc.shape[1]])
    return x if prior is None else x + prior


def ref_qhead(out_bits, qw_bits, nq, WN) -> np.ndarray:
    """qpart[N / WN, M, 4]: per row and head row a < nq, the sum over each wave's WN columns of the stored bf16
    output times qw[a][n]; columns a >= nq exactly 0."""
    M, N = out_bits.shape
    h = bf16_val(out_bits).reshape(M, N // WN, WN)
    w = bf16_val(qw_bits)[:nq, :N].reshape(nq, N // WN, WN)
    qp = np.zeros((N // WN, M, 4))
    qp[:, :, :nq] = np.einsum("mpw,apw->pma", h, w)
    return qp


# ----------------------------------------------------------------------------- exactness precondition
def _quarter(x) -> bool:
    x = np.asarray(x, np.float64)
    return bool(np.all(x * 4.0 == np.rint(x * 4.0)))


def assert_exact(p, inp, geo) -> None:
    """fp32 arithmetic on this problem is exact in any order: per element
    |alpha| sum|a||b| + |bias| + |prior| < 2^22 (so < 2^24) with every term a multiple of 2^-2; the folded
    reductions (colpart over WM rows, qpart over WN columns) stay below that as well."""
    A, B = bf16_val(inp["A"]), bf16_val(inp["B"])
    assert np.all(A == np.rint(A)) and np.all(B == np.rint(B)) and p["alpha"] in (1.0, 0.5, 0.25), p
    mag = abs(p["alpha"]) * (np.abs(A) @ np.abs(B).T)
    if inp["bias"] is not None:
        assert _quarter(inp["bias"])
        mag = mag + np.abs(inp["bias"])[None, :]
    if inp["prior"] is not None:
        assert _quarter(inp["prior"])
        mag = mag + np.abs(inp["prior"])
    assert float(mag.max()) < LIM, (p, float(mag.max()))
    M, N = mag.shape
    if p["colpart"]:   # stored values are bounded by mag (rounding is monotonic; 2^k bounds survive it)
        assert float(bf16_round64(mag).reshape(M // geo.WM, geo.WM, N).sum(1).max()) < LIM
    if p["nq"]:
        w = np.abs(bf16_val(inp["qw"]))
        assert np.all(w == np.rint(w))
        parts = np.einsum("mpw,apw->pma", bf16_round64(mag).reshape(M, N // geo.WN, geo.WN),
                          w[:, :N].reshape(-1, N // geo.WN, geo.WN))
        assert float(parts.max()) < LIM


def gauss_bound(p, inp) -> np.ndarray:
    """Per-element bound of the Gaussian cases: (K + 2) * 2^-23 * sum_k |a_k b_k| * |alpha|, float64.  2^-23 is
    twice the round-to-nearest unit: the rounding of the MFMA's internal adds is not specified."""
    A, B = bf16_val(inp["A"]), bf16_val(inp["B"])
    return (p["K"] + 2) * 2.0 ** -23 * (np.abs(A) @ np.abs(B).T) * abs(p["alpha"])


# ----------------------------------------------------------------------------- cases
def prob(M, N, K, epi, alpha=1.0, relu=False, bias=False, outT=False, accumulate=False, splitk=1, colpart=False,
         nq=0, gauss=False, small=False):
    return dict(M=M, N=N, K=K, epi=epi, alpha=alpha, relu=relu, bias=bias, outT=outT, accumulate=accumulate,
                splitk=splitk, colpart=colpart, nq=nq, gauss=gauss, small=small)


def case(name, kind, tile, probs, seed):
    return dict(name=name, kind=kind, tile=tile, probs=probs, seed=seed)


def _shape(g, i):
    """2 x 3 or 3 x 2 tiles (alternating), M != N."""
    a, b = ((2, 3), (3, 2))[i % 2]
    M, N = g.BM * a, g.BN * b
    assert M != N
    return M, N


_BF16_COMBOS = ((True, True, True), (False, False, False), (False, True, False), (True, False, True))   # relu bias outT


def body_cases(tid):
    """One gemm_body tile against every epilogue it supports: K / 64 in {1, 2, 3, 5, 7} (staged rings: also 4, so
    that {1, S-2, S-1, S, S+1} are all there), split-K 2 and 4 including one K-tile per split."""
    g = TILES[tid]
    kts = (1, 2, 3, 4, 5, 7) if g.S > 2 else (1, 2, 3, 5, 7)
    out = []
    for i, kt in enumerate(kts):
        M, N = _shape(g, i)
        K = kt * GBK
        for c in (i % 4, (i + 1) % 4):
            relu, bias, oT = _BF16_COMBOS[c]
            out.append(case(f"t{tid}-bf16-k{kt}-c{c}", "nt", tid,
                            [prob(M, N, K, EPI_BF16, alpha=0.5, relu=relu, bias=bias, outT=oT and g.has_t)],
                            1000 * tid + 10 * kt + c))
        out.append(case(f"t{tid}-rg-k{kt}", "nt", tid,
                        [prob(M, N, K, EPI_RELU_GRAD, outT=g.has_t, colpart=True)], 1000 * tid + 10 * kt + 5))
        out.append(case(f"t{tid}-f32-k{kt}", "nt", tid,
                        [prob(M, N, K, EPI_F32, alpha=0.25, bias=True, accumulate=i % 2 == 0)],
                        1000 * tid + 10 * kt + 6))
    for j, (kt, sk) in enumerate(((2, 2), (4, 2), (4, 4), (8, 4))):
        M, N = _shape(g, j)
        out.append(case(f"t{tid}-f32-k{kt}-sk{sk}", "nt", tid,
                        [prob(M, N, kt * GBK, EPI_F32, alpha=0.25, bias=True, accumulate=j % 2 == 1, splitk=sk)],
                        1000 * tid + 100 + 10 * kt + sk))
    return out


def qhead_cases(tid):
    """nq = 1..4 on one gemm_body tile (the test gives the head rows a leading dimension > N)."""
    g = TILES[tid]
    out = []
    for nq in (1, 2, 3, 4):
        M, N = _shape(g, nq)
        out.append(case(f"t{tid}-qh{nq}", "nt", tid,
                        [prob(M, N, (1, 3, 2, 5)[nq - 1] * GBK, EPI_BF16, alpha=0.5, relu=nq % 2 == 1, bias=nq != 2,
                              outT=g.has_t and nq == 3, nq=nq)], 2000 + 10 * tid + nq))
    return out


# 4 problems of different shapes per launch; workgroup totals 19, 15, 17, 12: remainders 3, 7, 1, 4 mod 8
BATCHED_CASES = [
    case("b-f32-t0", "batched", 0,
         [prob(256, 384, 256, EPI_F32, alpha=0.25, bias=True), prob(128, 256, 256, EPI_F32, bias=True, splitk=2, small=True),
          prob(256, 128, 256, EPI_F32, alpha=0.5, bias=True, accumulate=True, splitk=4, small=True),
          prob(128, 128, 64, EPI_F32, accumulate=True, small=True)], 3001),
    case("b-qh-t1", "batched", 1,
         [prob(128, 192, 128, EPI_BF16, alpha=0.5, relu=True, bias=True, nq=3),
          prob(192, 128, 64, EPI_BF16, alpha=0.5, bias=True, outT=True),
          prob(64, 128, 192, EPI_BF16, relu=True, bias=True, nq=2, small=True),
          prob(64, 64, 64, EPI_BF16, alpha=0.25, bias=True, small=True)], 3002),
    case("b-rg-t2", "batched", 2,
         [prob(256, 192, 128, EPI_RELU_GRAD, outT=True, colpart=True), prob(384, 128, 64, EPI_RELU_GRAD, colpart=True),
          prob(256, 128, 192, EPI_RELU_GRAD, outT=True), prob(128, 64, 64, EPI_RELU_GRAD, colpart=True, small=True)], 3003),
    case("b-bf16-t3", "batched", 3,
         [prob(512, 384, 128, EPI_BF16, alpha=0.5, relu=True, bias=True, outT=True),
          prob(512, 256, 64, EPI_BF16, bias=True), prob(256, 128, 192, EPI_BF16, alpha=0.25, bias=True, small=True),
          prob(256, 128, 64, EPI_BF16, relu=True, bias=True, outT=True, small=True)], 3004),
]

# the three accepted pairs on 128 x 128 tiles; the first is the learner's backward launch (relu-grad with outT and
# colpart beside a split-K weight gradient)
DUAL_CASES = [
    case("d-rg-f32", "dual", 0, [prob(256, 384, 128, EPI_RELU_GRAD, outT=True, colpart=True),
                                 prob(384, 256, 256, EPI_F32, splitk=4)], 4001),
    case("d-rg-f32-sk1", "dual", 0, [prob(384, 256, 192, EPI_RELU_GRAD, outT=True, colpart=True),
                                     prob(256, 384, 128, EPI_F32, alpha=0.5, bias=True, accumulate=True)], 4002),
    case("d-f32-f32", "dual", 0, [prob(256, 384, 192, EPI_F32, alpha=0.25, bias=True, splitk=3),
                                  prob(384, 256, 128, EPI_F32, alpha=0.5, accumulate=True, splitk=2)], 4003),
    case("d-bf16-f32", "dual", 0, [prob(384, 256, 128, EPI_BF16, alpha=0.5, relu=True, bias=True, outT=True),
                                   prob(256, 384, 256, EPI_F32, bias=True, splitk=2)], 4004),
]


def big_cases(tid):
    """The 256 x 256 ping-pong / w4 kernels: both epilogues, K / 64 in {1, 2, 3, 6, 7} on 2 x 3 / 3 x 2 tiles, and
    the tile grids 1 x 1, 3 x 5, 9 x 2, 10 x 2 at K = 64 (the XCD-grouped order with a ragged last group)."""
    out = []
    for i, kt in enumerate((1, 2, 3, 6, 7)):
        M, N = ((512, 768), (768, 512))[i % 2]
        relu, bias, _ = _BF16_COMBOS[i % 4]
        out.append(case(f"t{tid}-bf16-k{kt}", "nt", tid, [prob(M, N, kt * GBK, EPI_BF16, alpha=0.5, relu=relu, bias=bias)],
                        5000 + 100 * tid + kt))
        out.append(case(f"t{tid}-f32-k{kt}", "nt", tid,
                        [prob(M, N, kt * GBK, EPI_F32, alpha=0.25, bias=i % 2 == 0, accumulate=i % 3 != 0)],
                        5050 + 100 * tid + kt))
    for j, (a, b) in enumerate(((1, 1), (3, 5), (9, 2), (10, 2))):
        out.append(case(f"t{tid}-bf16-g{a}x{b}", "nt", tid,
                        [prob(256 * a, 256 * b, GBK, EPI_BF16, alpha=0.5, relu=j % 2 == 0, bias=True, small=a == b)],
                        6000 + 100 * tid + j))
        out.append(case(f"t{tid}-f32-g{a}x{b}", "nt", tid,
                        [prob(256 * a, 256 * b, GBK, EPI_F32, alpha=0.25, bias=True, accumulate=j % 2 == 1, small=a == b)],
                        6050 + 100 * tid + j))
    return out


def gauss_cases(tid):
    """Two Gaussian-operand cases per tile: a bf16 store and an fp32 store."""
    g = TILES[tid]
    M, N = _shape(g, tid)
    return [case(f"t{tid}-gauss-bf16", "nt", tid, [prob(M, N, 448, EPI_BF16, alpha=0.5, bias=True, gauss=True)], 7000 + tid),
            case(f"t{tid}-gauss-f32", "nt", tid,
                 [prob(M, N, 320, EPI_F32, alpha=0.25, bias=True, gauss=True, splitk=1 if tid > 6 or tid % 2 else 5)],
                 7100 + tid)]


def exact_cases():
    out = []
    for t in BODY_TILES:
        out += body_cases(t) + qhead_cases(t)
    out += BATCHED_CASES + DUAL_CASES
    for t in BIG_TILES:
        out += big_cases(t)
    return out


def blocks(c) -> int:
    """Workgroups of the launch."""
    g = TILES[c["tile"]]
    return sum((p["M"] // g.BM) * (p["N"] // g.BN) * max(1, p["splitk"]) for p in c["probs"])


def case_inputs(c):
    """Host operands of every problem of a case (bit patterns for bf16, float64 values for fp32)."""
    out = []
    for i, p in enumerate(c["probs"]):
        s = 100 * c["seed"] + 10 * i
        M, N, K = p["M"], p["N"], p["K"]
        mk = gauss_bits if p["gauss"] else int_bits
        inp = dict(A=mk((M, K), s), B=mk((N, K), s + 1), bias=None, prior=None, act=None, qw=None)
        if p["bias"]:
            inp["bias"] = (np.random.default_rng(s + 2).standard_normal(N).astype(F).astype(np.float64) if p["gauss"]
                           else int_vals(N, s + 2))
        if p["accumulate"]:
            inp["prior"] = int_vals((M, N), s + 3)
        if p["epi"] == EPI_RELU_GRAD:
            inp["act"] = act_bits(M, N, s + 4)
        if p["nq"]:
            inp["qw"] = int_bits((p["nq"], N), s + 5, -4, 4)
        out.append(inp)
    return out


def case_refs(c, inputs):
    """Expected outputs per problem: out (bf16 bits, or float64 for EPI_F32) and, where the problem has them, outT,
    colpart, qpart; x = the bf16 epilogue's value before the store's rounding (Gaussian interval check)."""
    g = TILES[c["tile"]]
    refs = []
    for p, inp in zip(c["probs"], inputs):
        acc = acc_ref(inp["A"], inp["B"])
        r = {}
        if p["epi"] == EPI_F32:
            r["out"] = ref_f32(acc, p["alpha"], inp["bias"], inp["prior"])
        elif p["epi"] == EPI_RELU_GRAD:
            r["out"], oT, cp = ref_relu_grad(acc, inp["act"], g.WM)
            if p["outT"]:
                r["outT"] = oT
            if p["colpart"]:
                r["colpart"] = cp
        else:
            r["x"] = ref_bf16(acc, p["alpha"], inp["bias"], p["relu"])
            r["out"] = bf16_rne(r["x"])
            if p["outT"]:
                r["outT"] = np.ascontiguousarray(r["out"].T)
            if p["nq"]:
                r["qpart"] = ref_qhead(r["out"], inp["qw"], p["nq"], g.WN)
        refs.append(r)
    return refs


# ----------------------------------------------------------------------------- comparisons
def check_bf16(got_bits, ref_bits) -> int:
    """Differing bf16 bit patterns, -0 counted as +0 (a NaN left by the prefill differs from every reference)."""
    a = np.asarray(got_bits, np.uint16).copy()
    b = np.asarray(ref_bits, np.uint16).copy()
    assert a.shape == b.shape, (a.shape, b.shape)
    a[a == 0x8000] = 0
    b[b == 0x8000] = 0
    return int((a != b).sum())


def check_f32(got, ref) -> int:
    """Differing fp32 bit patterns against the float64 reference (which must be an fp32 value), -0 as +0."""
    a = np.ascontiguousarray(got, dtype=F)
    r64 = np.asarray(ref, np.float64)
    b = r64.astype(F)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(b.astype(np.float64), r64), "reference not exact in fp32"
    ab, bb = a.view(np.uint32).copy(), b.view(np.uint32).copy()
    ab[ab == 0x80000000] = 0
    bb[bb == 0x80000000] = 0
    return int((ab != bb).sum())


def check_problem(got, ref) -> dict:
    """Exact comparison of every output a problem has: name -> differing entries."""
    n = {}
    for k in ("out", "outT", "colpart", "qpart"):
        if k in ref:
            f32 = k in ("colpart", "qpart") or ref[k].dtype != np.uint16
            n[k] = (check_f32 if f32 else check_bf16)(got[k], ref[k])
    return n


def check_gauss(p, got, ref, bound):
    """Gaussian case: (entries outside the bound, largest err / bound).  A bf16 output must be bf16_rne of some value
    within the bound of the reference: rne(ref - bound) <= got <= rne(ref + bound); its err is the distance from the
    reference to the nearest value that rounds to the stored one."""
    if p["epi"] == EPI_F32:
        g = np.asarray(got["out"], np.float64)
        err = np.abs(g - ref["out"])
        bad = ~(err <= bound)
    else:
        v = bf16_val(got["out"])
        x = ref["x"]
        bad = ~((bf16_round64(x - bound) <= v) & (v <= bf16_round64(x + bound)))
        _, e = np.frexp(v)
        half = np.ldexp(1.0, np.maximum(e, -125) - 9)
        err = np.maximum(np.abs(v - x) - half, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return int(bad.sum()), float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("inf")


# ----------------------------------------------------------------------------- index maps
def xcd_remap(bid, n, remainder=True):
    """Workgroup id -> work index: neighbouring indices on one XCD (blockIdx % 8)."""
    xcd, q, r = bid % 8, n // 8, (n % 8 if remainder else 0)
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + bid // 8


def pp_tile(idx, ntm, ntn, ragged=True):
    """The ping-pong kernel's tile order: groups of 8 tile rows walked column by column."""
    gsz = 8 * ntn
    g, r = idx // gsz, idx % gsz
    gm = min(ntm - 8 * g, 8) if ragged else 8
    return 8 * g + r % gm, r // gm


# ----------------------------------------------------------------------------- numpy model of the kernels' tiling
MUTATIONS = ("drop_last_ktile", "swap_kchunks", "bias_local", "alpha_after_bias", "bias_every_split",
             "accumulate_ignores_prior", "bf16_trunc", "mask_ge", "mask_untransposed", "outT_in_tile",
             "colpart_unrounded", "colpart_row", "qpart_unrounded", "qpart_part", "qpart_col_nq", "batch_bias0",
             "pp_gm8", "xcd_no_remainder")


def _put(dst, r0, c0, blk):
    """Store a block where it lands inside dst (a mutated index may fall outside: those elements stay unwritten)."""
    r1, c1 = min(r0 + blk.shape[0], dst.shape[0]), min(c0 + blk.shape[1], dst.shape[1])
    if r0 < dst.shape[0] and c0 < dst.shape[1]:
        dst[r0:r1, c0:c1] = blk[:r1 - r0, :c1 - c0]


def _model_block(g, p, inp, got, idx, mut, bias):
    """One workgroup: tile (and K split) idx of problem p, wave by wave where the epilogue reduces per wave."""
    M, N, K = p["M"], p["N"], p["K"]
    ntm, ntn = M // g.BM, N // g.BN
    nsplit = max(1, p["splitk"])
    ks, t = divmod(idx, ntm * ntn)
    if g.kind == "pp":
        tm, tn = pp_tile(t, ntm, ntn, ragged=mut != "pp_gm8")
    else:
        tm, tn = divmod(t, ntn)
    if tm >= ntm or tn >= ntn:
        return
    m0, n0 = tm * g.BM, tn * g.BN
    nk = K // GBK // nsplit
    kb = ks * nk * GBK
    A = bf16_val(inp["A"][m0:m0 + g.BM]).copy()
    B = bf16_val(inp["B"][n0:n0 + g.BN])
    acc = np.zeros((g.BM, g.BN))
    for kt in range(nk - 1 if mut == "drop_last_ktile" else nk):
        a = A[:, kb + kt * GBK: kb + (kt + 1) * GBK].copy()
        if mut == "swap_kchunks":
            a[:, 0:8], a[:, 8:16] = a[:, 8:16].copy(), a[:, 0:8].copy()
        acc += a @ B[:, kb + kt * GBK: kb + (kt + 1) * GBK].T
    bb = np.zeros(g.BN)
    if bias is not None:
        bb = bias[0:g.BN] if mut == "bias_local" else bias[n0:n0 + g.BN]
    rows, cols = slice(m0, m0 + g.BM), slice(n0, n0 + g.BN)
    if p["epi"] == EPI_F32:
        if ks != 0 and mut != "bias_every_split":
            bb = np.zeros(g.BN)
        v = p["alpha"] * (acc + bb) if mut == "alpha_after_bias" else p["alpha"] * acc + bb
        if nsplit > 1 or p["accumulate"]:
            got["out"][rows, cols] += v
        else:
            got["out"][rows, cols] = v
        return
    rnd = bf16_trunc if mut == "bf16_trunc" else bf16_rne
    if p["epi"] == EPI_BF16:
        x = p["alpha"] * (acc + bb) if mut == "alpha_after_bias" else p["alpha"] * acc + bb
        v = np.maximum(x, 0.0) if p["relu"] else x
    else:
        aT = inp["act"].T.copy()                       # the buffer the kernel reads: [N][M]
        act = aT.reshape(M, N) if mut == "mask_untransposed" else aT.T
        h = bf16_val(act[rows, cols])
        v = np.where(h >= 0.0 if mut == "mask_ge" else h > 0.0, acc, 0.0)
    bits = rnd(v)
    got["out"][rows, cols] = bits
    if p["outT"]:
        if mut == "outT_in_tile":
            _put(got["outT"], tm * g.BN, tn * g.BM, bits.T)
        else:
            got["outT"][cols, rows] = bits.T
    stored = bf16_val(bits)
    if p["colpart"]:
        src = v if mut == "colpart_unrounded" else stored
        for wm in range(g.NWM):
            row = wm * ntm + tm if mut == "colpart_row" else tm * g.NWM + wm
            got["colpart"][row, cols] = src[wm * g.WM:(wm + 1) * g.WM].sum(0)
    if p["nq"]:
        src = v if mut == "qpart_unrounded" else stored
        nq, w = p["nq"], bf16_val(inp["qw"])
        for wn in range(g.NWN):
            part = (n0 + wn * g.WN) // g.WN
            if mut == "qpart_part":
                part = (part + 1) % (N // g.WN)
            q = np.zeros((g.BM, 4))
            q[:, :nq] = src[:, wn * g.WN:(wn + 1) * g.WN] @ w[:, n0 + wn * g.WN: n0 + (wn + 1) * g.WN].T
            if mut == "qpart_col_nq" and nq < 4:
                q[:, nq] = q[:, nq - 1]
            got["qpart"][part, rows, :] = q


def model_launch(c, inputs, mut=None):
    """What the launch of case c leaves in its outputs (prefilled with NaN, or the prior / zeros where the kernel
    adds), computed workgroup by workgroup through the kernels' index maps.  ``mut``: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS, mut
    g = TILES[c["tile"]]
    gots, nblk = [], []
    for p, inp in zip(c["probs"], inputs):
        M, N = p["M"], p["N"]
        got = {}
        if p["epi"] == EPI_F32:
            if p["accumulate"]:
                got["out"] = np.zeros((M, N)) if mut == "accumulate_ignores_prior" else inp["prior"].copy()
            else:
                got["out"] = np.zeros((M, N)) if p["splitk"] > 1 else np.full((M, N), np.nan)
        else:
            got["out"] = np.full((M, N), 0x7FC0, np.uint16)
        if p["outT"]:
            got["outT"] = np.full((N, M), 0x7FC0, np.uint16)
        if p["colpart"]:
            got["colpart"] = np.full((M // g.WM, N), np.nan)
        if p["nq"]:
            got["qpart"] = np.full((N // g.WN, M, 4), np.nan)
        gots.append(got)
        nblk.append((M // g.BM) * (N // g.BN) * max(1, p["splitk"]))
    total = sum(nblk)
    for bid in range(total):
        idx = xcd_remap(bid, total, remainder=mut != "xcd_no_remainder")
        pi = 0
        while pi + 1 < len(nblk) and idx >= nblk[pi]:
            idx -= nblk[pi]
            pi += 1
        if idx >= nblk[pi]:
            continue
        bias = inputs[pi]["bias"]
        if mut == "batch_bias0" and pi == 1 and inputs[0]["bias"] is not None:
            bias = np.resize(inputs[0]["bias"], c["probs"][1]["N"])
        _model_block(g, c["probs"][pi], inputs[pi], gots[pi], idx, mut, bias)
    return gots
