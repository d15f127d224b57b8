"""Every bf16 GEMM tile and epilogue of csrc/gemm_bf16.hip against the float64 references of tests/gemm_refs.py.

Exact cases (integer operands: fp32 arithmetic is exact in any order, see gemm_refs) must match bit for bit: every
tile id against every epilogue it has, alpha, bias, relu on and off, accumulate, split-K, outT, the relu-grad column
partials (colpart), the folded head (qpart, part by part), grouped and dual launches, and the 256 x 256 ping-pong /
w4 kernels against the reference itself.  Gaussian cases are held to gemm_refs.gauss_bound per element.

Every operand and output is a strided region (row stride > row) of a NaN-filled guard band: after the launch the
guards and the gaps between rows must be bit-unchanged, every in-range output written (a left-over NaN differs from
every reference), and the inputs unchanged.  Refused launches must leave everything untouched."""
import time

import numpy as np
import pytest
import torch

import gemm_refs as R
from guard_band import Band, bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32


def _bf(b: np.ndarray) -> torch.Tensor:
    """bf16 bit patterns -> a bf16 tensor (no cast involved)."""
    return torch.from_numpy(np.ascontiguousarray(b, np.uint16).view(np.int16)).view(BF)


class Plane:
    """[rows, cols] with row stride cols + pad inside a NaN-filled Band."""

    def __init__(self, rows, cols, dtype, pad):
        self.band = Band(rows * (cols + pad), dtype, NAN)
        self.all = self.band.v.view(rows, cols + pad)
        self.v = self.all[:, :cols]
        self.gap = self.all[:, cols:]
        self._gap = bits(self.gap).clone()

    def put(self, t):
        self.v.copy_(t.to(self.v.dtype) if t.dtype != self.v.dtype else t)
        return self

    def intact(self) -> bool:
        return self.band.guards_intact() and torch.equal(bits(self.gap), self._gap)

    def numpy(self) -> np.ndarray:
        c = self.v.contiguous()
        return bits(c).cpu().numpy().view(np.uint16) if c.dtype == BF else c.cpu().numpy()


class Flat:
    """A contiguous region inside a NaN-filled Band (bias, qpart)."""

    def __init__(self, shape, dtype):
        self.band = Band(int(np.prod(shape)), dtype, NAN)
        self.v = self.band.v.view(*shape)

    def put(self, t):
        self.v.copy_(t)
        return self

    def intact(self) -> bool:
        return self.band.guards_intact()

    def numpy(self) -> np.ndarray:
        return self.v.cpu().numpy()


class Problem:
    """One product's device buffers: ``args`` = (A, B, out, kwargs) for the wrappers of sharetrade.ops.gemm."""

    def __init__(self, p, inp, g, colpart_rows=None, pads=None):
        pad = dict(A=8, B=16, out=8, outT=8, aux=4, cp=8, qw=8)
        pad.update(pads or {})
        M, N, K = p["M"], p["N"], p["K"]
        f32 = p["epi"] == R.EPI_F32
        self.p = p
        self.ins = {"A": Plane(M, K, BF, pad["A"]).put(_bf(inp["A"])), "B": Plane(N, K, BF, pad["B"]).put(_bf(inp["B"]))}
        self.outs = {"out": Plane(M, N, F32 if f32 else BF, pad["out"])}
        if p["accumulate"]:
            self.outs["out"].put(torch.from_numpy(inp["prior"].astype(np.float32)))
        kw = dict(alpha=p["alpha"], relu=p["relu"], accumulate=p["accumulate"], splitk=p["splitk"])
        if p["bias"]:
            self.ins["bias"] = Flat((N,), F32).put(torch.from_numpy(inp["bias"].astype(np.float32)))
            kw["bias"] = self.ins["bias"].v
        if p["outT"]:
            self.outs["outT"] = Plane(N, M, BF, pad["outT"])
            kw["outT"] = self.outs["outT"].v
        if p["epi"] == R.EPI_RELU_GRAD:
            self.ins["aux"] = Plane(N, M, BF, pad["aux"]).put(_bf(inp["act"].T))
            kw["auxT"] = self.ins["aux"].v
        if p["colpart"]:
            self.outs["colpart"] = Plane(colpart_rows or M // g.WM, N, F32, pad["cp"])
            kw["colpart"] = self.outs["colpart"].v
        if p["nq"]:
            self.ins["qw"] = Plane(p["nq"], N, BF, pad["qw"]).put(_bf(inp["qw"]))
            self.outs["qpart"] = Flat((N // g.WN, M, 4), F32)
            kw["qhead"] = (self.ins["qw"].v, self.outs["qpart"].v)
        self.kw = kw
        self.args = (self.ins["A"].v, self.ins["B"].v, self.outs["out"].v, kw)
        self._snap = {k: b.band.snap() for k, b in self.ins.items()}
        self._osnap = {k: b.band.snap() for k, b in self.outs.items()}

    def inputs_unchanged(self) -> bool:
        return all(b.band.same(self._snap[k]) for k, b in self.ins.items())

    def untouched(self) -> bool:
        return self.inputs_unchanged() and all(b.band.same(self._osnap[k]) for k, b in self.outs.items())

    def surroundings(self) -> dict:
        return {k: b.intact() for k, b in self.outs.items()}

    def got(self) -> dict:
        return {k: b.numpy() for k, b in self.outs.items()}


def _launch(c, probs):
    from sharetrade.ops import gemm as gm

    g = R.TILES[c["tile"]]
    if c["kind"] == "nt":
        A, B, out, kw = probs[0].args
        gm.gemm_nt(A, B, out, c["probs"][0]["epi"], tile=g.key, **kw)
    elif c["kind"] == "batched":
        gm.gemm_nt_batched([q.args for q in probs], c["probs"][0]["epi"], tile=g.key)
    else:
        gm.gemm_dual(probs[0].args, c["probs"][0]["epi"], probs[1].args, c["probs"][1]["epi"])
    torch.cuda.synchronize()


def _run_exact(cases, label):
    """Launch every case once; all outputs bit-equal to the reference, surroundings and inputs unchanged."""
    t0 = time.time()
    bad = []
    for c in cases:
        g = R.TILES[c["tile"]]
        inputs = R.case_inputs(c)
        refs = R.case_refs(c, inputs)
        probs = [Problem(p, inp, g) for p, inp in zip(c["probs"], inputs)]
        _launch(c, probs)
        for i, (q, ref) in enumerate(zip(probs, refs)):
            n = R.check_problem(q.got(), ref)
            sur = q.surroundings()
            if any(n.values()) or not all(sur.values()) or not q.inputs_unchanged():
                bad.append((c["name"], i, n, sur, q.inputs_unchanged()))
    print(f"[gemm-refs] {label}: {len(cases)} launches, {len(bad)} wrong, {time.time() - t0:.2f} s")
    assert not bad, bad[:8]


@pytest.mark.parametrize("tid", R.BODY_TILES)
def test_body_tile_exact(native_built, tid):
    """One gemm_body tile: bf16 (alpha 0.5, relu / bias / outT on and off), relu-grad with outT and colpart, fp32
    (alpha 0.25, bias, accumulate), split-K 2 and 4, and the folded head with nq = 1..4, ldqw > N."""
    _run_exact(R.body_cases(tid) + R.qhead_cases(tid), f"tile {tid} {R.TILES[tid].key}")


def test_batched_exact(native_built):
    """gemm_nt_batched: 4 problems of different shapes (and K splits) per launch, with qhead, colpart, outT; the
    launches' workgroup counts are 1, 3, 4 and 7 mod 8 (xcd_remap's remainder branch)."""
    _run_exact(R.BATCHED_CASES, "batched")


def test_dual_exact(native_built):
    """gemm_dual: relu-grad (outT, colpart) + f32 split-K as the learner's backward launches it, f32 + f32,
    bf16 + f32."""
    _run_exact(R.DUAL_CASES, "dual")


@pytest.mark.parametrize("tid", R.BIG_TILES)
def test_big_tile_exact(native_built, tid):
    """Ping-pong, ping-pong with priority, w4: both epilogues against the float64 reference itself, K / 64 in
    {1, 2, 3, 6, 7}, tile grids 1 x 1, 3 x 5, 9 x 2, 10 x 2, strided operands and outputs."""
    _run_exact(R.big_cases(tid), f"tile {tid} {R.TILES[tid].key}")


@pytest.mark.parametrize("tid", sorted(R.TILES))
def test_gauss_within_bound(native_built, tid):
    """Full-mantissa operands: every element within (K + 2) 2^-23 sum|a b| |alpha| of the float64 reference (a bf16
    output: the rounding of some value that close).  Prints the largest err / bound."""
    g = R.TILES[tid]
    for c in R.gauss_cases(tid):
        (p,), (inp,) = c["probs"], R.case_inputs(c)
        (ref,) = R.case_refs(c, [inp])
        q = Problem(p, inp, g)
        _launch(c, [q])
        bad, ratio = R.check_gauss(p, q.got(), ref, R.gauss_bound(p, inp))
        print(f"[gemm-refs] {c['name']} {g.key} K={p['K']} splitk={p['splitk']}: outside {bad}, err/bound {ratio:.4g}")
        assert bad == 0 and ratio <= 1.0 and all(q.surroundings().values()) and q.inputs_unchanged(), c["name"]


def _refused(c, q):
    with pytest.raises(RuntimeError):
        _launch(c, [q])
    torch.cuda.synchronize()
    assert q.untouched(), c["name"]


def test_refusals_leave_everything_untouched(native_built):
    """Launches the host check must refuse, before any write: a colpart whose row count is not M / WM of the
    launch's tile (M / 64 rows on the 64 x 64 or 256 x 256 tile among them; the buffers still hold enough rows),
    colpart / qhead on the ping-pong and w4 ids, and leading dimensions off their alignment."""
    n = 0
    for tid in R.BODY_TILES:
        g = R.TILES[tid]
        M, N = 2 * g.BM, 3 * g.BN
        p = R.prob(M, N, 64, R.EPI_RELU_GRAD, outT=g.has_t, colpart=True)
        c = R.case(f"refuse-cp-t{tid}", "nt", tid, [p], 9000 + tid)
        (inp,) = R.case_inputs(c)
        big = Problem(p, inp, g, colpart_rows=M // 32 + 1)
        want = M // g.WM
        for rows in sorted({M // 32, M // 64, M // 128, want - 1, want + 1} - {want}):
            big.kw["colpart"] = big.outs["colpart"].v[:rows]
            _refused(c, big)
            n += 1
    for tid in R.BIG_TILES:
        g = R.TILES[tid]
        for p in (R.prob(512, 768, 64, R.EPI_RELU_GRAD, colpart=True), R.prob(512, 768, 64, R.EPI_BF16, nq=3)):
            c = R.case(f"refuse-side-t{tid}", "nt", tid, [p], 9100 + tid)
            (inp,) = R.case_inputs(c)
            _refused(c, Problem(p, inp, g))
            n += 1
    for tid, epi, key in ((0, R.EPI_BF16, "A"), (1, R.EPI_BF16, "B"), (2, R.EPI_BF16, "out"), (3, R.EPI_BF16, "outT"),
                          (4, R.EPI_RELU_GRAD, "aux"), (6, R.EPI_RELU_GRAD, "out"), (7, R.EPI_BF16, "A"),
                          (8, R.EPI_F32, "B"), (9, R.EPI_BF16, "out")):
        g = R.TILES[tid]
        p = R.prob(2 * g.BM, 3 * g.BN, 128, epi, outT=key == "outT")
        c = R.case(f"refuse-ld-t{tid}", "nt", tid, [p], 9200 + tid)
        (inp,) = R.case_inputs(c)
        _refused(c, Problem(p, inp, g, pads={key: 2 if key == "aux" else 4}))
        n += 1
    print(f"[gemm-refs] refusals: {n} launches refused")
