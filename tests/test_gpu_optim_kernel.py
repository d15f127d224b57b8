"""csrc/optim.hip against plain float64 references, on hand-built tensors (no engine).

`st_reduce_optim` ends every engine step: slab reduction, SGD / AdaGrad / Adam, the bf16 refresh, the
step statistics, the Polyak average and the ws weight image.  These tests drive its three modes
(0 = reduce + update, 1 = reduce only, 2 = update only) and both template instances at the shapes the
engine never produces: a partial last workgroup, G below / off the row-group count, P % 128 != 0 with
bf16 slabs, scale != 1, nstat < 8, tdelay, and the -1 entries of img_map.

Slab layouts pinned here:
  fp32 slabs   [G][P]          (P % 4 == 0; a workgroup of 256 threads covers 64 parameters, 16 row groups)
  bf16 slabs   [P/32][G][32]   (P % 32 == 0; a workgroup of 512 threads covers 128 parameters = 4 column
                               blocks, 32 row groups); element (r, p) is at (p // 32) * G * 32 + r * 32 + p % 32.
                               The slab is allocated at exactly P/32 * G * 32 elements: the kernel must not
                               need P rounded up to 128.

Every buffer sits in a guard band (tests/guard_band.py): NaN around what is read, a sentinel around what
is only written; after each launch the surroundings are bit-unchanged and no result holds a NaN.
"""
import math

import numpy as np
import pytest
import torch

from guard_band import Band, bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
KIND = {"sgd": 0, "adagrad": 1, "adam": 2}
NAN = float("nan")
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8

P_F32 = [4, 60, 64, 68, 1028]      # 64 parameters per workgroup
P_BF16 = [32, 96, 128, 160, 4128]  # 128 parameters per workgroup
G_ALL = [1, 2, 15, 16, 17, 31, 32, 33, 64, 257]
# every P and every G for both slab dtypes; the largest P meets the largest G (the last entry)
SLAB_CASES = [(bf, (P_BF16 if bf else P_F32)[i % 5], g) for bf in (False, True) for i, g in enumerate(G_ALL)]
EDGE_CASES = [(bf, p) for bf in (False, True) for p in (P_BF16 if bf else P_F32)]


def _f32(x: float) -> float:
    """A hyper-parameter as the kernel receives it."""
    return float(np.float32(x))


def _id(v):
    return ("bf16" if v else "f32") if isinstance(v, bool) else str(v)


class Case:
    """Every buffer of one st_reduce_optim launch, each inside its own guard band."""

    def __init__(self, native, P: int, G: int, bf: bool, nstat: int = 8, img_bytes: int = 16):
        self.native, self.P, self.G, self.bf = native, P, G, bf
        f = torch.float32
        self.b = {
            "params": Band(P, f, NAN).set(0.125),
            "params_bf": Band(P, torch.bfloat16, -7776.0).set(0.125),
            "mask": Band(P, f, NAN).set(1.0),
            "s1": Band(P, f, NAN).set(0.5),
            "s2": Band(P, f, NAN).set(0.25),
            "slab": Band(G * P, torch.bfloat16 if bf else f, NAN).set(0.0),
            "grad": Band(P, f, NAN).set(123.0),
            "ema": Band(P, f, NAN).set(0.375),
            "ctrl": Band(2, torch.int64, 0x5A5A5A5A5A5A).set(torch.tensor([0, 1])),
            "stats": Band(G * nstat, f, NAN).set(0.0),
            "stat_acc": Band(8, torch.float64, NAN).set(torch.arange(8, dtype=torch.float64) * 1000.5 + 17.25),
            "heads": Band(256, torch.int32, 0x0BADF00D).set(torch.arange(256, dtype=torch.int32) + 0x1000),
            "img_map": Band(P, torch.int32, -1).set(-1),
            "img": Band(img_bytes, torch.uint8, 0x3C).set(0xA5),
        }

    def __getattr__(self, name):
        try:
            return self.__dict__["b"][name]
        except KeyError:
            raise AttributeError(name)

    def load(self, st: dict) -> "Case":
        """params / mask / s1 / s2 (cpu fp32) and the matching bf16 copy."""
        for k in ("params", "mask", "s1", "s2"):
            self.b[k].set(st[k])
        self.b["params_bf"].set(st["params"].to(torch.bfloat16))
        return self

    def launch(self, mode: int, kind: int = 0, scale: float = 1.0, stats=False, nstat: int = 0, heads=False,
               ema=False, ema_decay: float = 0.0, img=False, tdelay: int = 0, null=()) -> int:
        n = self.native
        o = n.OptimParams()
        for k in ("params", "params_bf", "mask", "s1", "s2", "slab", "grad", "ctrl", "stat_acc"):
            setattr(o, k, None if k in null else self.b[k].ptr())
        o.G, o.P, o.kind, o.mode = self.G, self.P, kind, mode
        o.slab_bf16 = int(self.bf)
        o.lr, o.beta1, o.beta2, o.eps, o.scale, o.tdelay = LR, B1, B2, EPS, scale, tdelay
        if stats:
            o.stats, o.nstat = self.b["stats"].ptr(), nstat
        if heads:
            o.chunk_heads = self.b["heads"].ptr()
        if ema:
            o.ema, o.ema_decay = self.b["ema"].ptr(), ema_decay
        if img:
            o.img, o.img_map = self.b["img"].ptr(), self.b["img_map"].ptr()
        rc = n.lib().st_reduce_optim(o, n.stream_handle())
        torch.cuda.synchronize()
        return rc

    def snap(self) -> dict:
        return {k: v.snap() for k, v in self.b.items()}

    def check(self, before: dict, written=()) -> None:
        """Everything outside ``written`` is bit-unchanged (guards included); the written regions' guards
        are intact and they hold no NaN."""
        for k, v in self.b.items():
            if k in written:
                assert v.guards_intact(), f"{k}: write outside its region"
                if v.v.is_floating_point():
                    assert not torch.isnan(v.v).any(), f"{k}: NaN in a result (over-read of a guard band?)"
            else:
                assert v.same(before[k]), f"{k} changed"


def _slab_layout(g: torch.Tensor, bf: bool) -> torch.Tensor:
    """g [G, P] float64 (values exact in the slab dtype) -> the slab in device layout."""
    if not bf:
        return g.float()
    G, P = g.shape
    return g.view(G, P // 32, 32).permute(1, 0, 2).contiguous().to(torch.bfloat16)


def _edge_mask(P: int, bf: bool) -> torch.Tensor:
    """0/1 mask with zeros inside and at both ends of every workgroup's range."""
    wg = 128 if bf else 64
    i = torch.arange(P)
    m = torch.ones(P, dtype=torch.float64)
    m[(i % wg == 0) | (i % wg == 17) | (i % wg == wg - 1) | (i == P - 1)] = 0.0
    return m


def _exact_g(G: int, P: int, mod: int = 257) -> torch.Tensor:
    r = torch.arange(G, dtype=torch.int64)[:, None]
    p = torch.arange(P, dtype=torch.int64)[None, :]
    return (((7 * r + 13 * p) % mod) - 128).double()


# --------------------------------------------------------------------------- A. slab reduction, mode 1
@pytest.mark.parametrize("bf,P,G", SLAB_CASES, ids=_id)
def test_slab_reduce_exact(native_built, bf, P, G):
    """Integer gradients g[r][p] = ((7 r + 13 p) mod 257) - 128 (exact in bf16, partial sums < 2^24):
    grad is bit-equal to mask * scale * sum_r g[r][p]; a dropped, doubled or permuted row, 16-byte piece
    or column block changes it.  Over exactly 257 rows every column of that pattern has the same sum (7 r
    runs through all residues), so columns could trade places unseen: the same pattern mod 251 runs too.
    Mode 1 writes grad and nothing else."""
    c = Case(native_built, P, G, bf)
    mask = _edge_mask(P, bf)
    c.mask.set(mask)
    live_map = torch.full((P,), -1, dtype=torch.int32)
    live_map[1], live_map[2] = 0, -3   # a bf16 element and an fp32 word an update would write
    c.img_map.set(live_map)
    for scale, mod in ((1.0, 257), (0.5, 257), (1.0, 251), (0.5, 251)):
        g = _exact_g(G, P, mod)
        c.slab.set(_slab_layout(g, bf))
        c.grad.set(123.0)
        before = c.snap()
        assert c.launch(1, scale=scale, ema=True, ema_decay=0.9, img=True) == 0
        c.check(before, written=("grad",))
        ref = (mask * scale * g.sum(0)).float()
        got = c.grad.cpu()
        bad = (bits(got) != bits(ref)).nonzero().flatten()
        assert bad.numel() == 0, (scale, bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())


@pytest.mark.parametrize("bf,P,G", SLAB_CASES, ids=_id)
def test_slab_reduce_random(native_built, bf, P, G):
    """Values over six decades, scale = 1/3.  Bound (derived, not measured): each of the RG row groups
    sums ceil(G/RG) rows in a chain, two chains of RG/2 fold the row groups, then one add and the scale
    and mask multiplies: |got - ref64| <= (ceil(G/RG) + RG/2 + 4) 2^-24 |scale| sum_r |g[r][p]|."""
    gen = torch.Generator().manual_seed(1000 * G + P)
    g = torch.randn(G, P, dtype=torch.float64, generator=gen)
    g = g * 10.0 ** (torch.rand(G, P, dtype=torch.float64, generator=gen) * 6.0 - 3.0)
    g = g.to(torch.bfloat16 if bf else torch.float32).double()   # the bits the kernel decodes
    mask = _edge_mask(P, bf)
    scale = _f32(1.0 / 3.0)
    c = Case(native_built, P, G, bf)
    c.slab.set(_slab_layout(g, bf))
    c.mask.set(mask)
    before = c.snap()
    assert c.launch(1, scale=scale) == 0
    c.check(before, written=("grad",))
    rg = 32 if bf else 16
    ref = mask * scale * g.sum(0)
    bound = (math.ceil(G / rg) + rg / 2 + 4) * U * abs(scale) * g.abs().sum(0)
    got = c.grad.cpu().double()
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    print(f"[meas] slab_reduce_random {_id(bf)} P={P} G={G}: max err/bound = {ratio:.4f}")
    assert (err <= bound).all(), ratio
    assert (got[mask == 0] == 0).all()


# --------------------------------------------------------------------------- B. statistics, chunk heads
@pytest.mark.parametrize("G", [1, 31, 32, 33, 64, 65, 257])
@pytest.mark.parametrize("nstat", [1, 3, 8])
@pytest.mark.parametrize("bf", [False, True], ids=_id)
def test_stats_fold(native_built, bf, nstat, G):
    """stat_acc[:nstat] += column sums of stats [G][nstat] (fp64, exact on integers) in modes 0 and 1;
    thread t of block 0 sums stat t & 7 over rows t/8, t/8 + RT/8, ... (RT/8 = 32 or 64)."""
    c = Case(native_built, 32 if bf else 4, G, bf, nstat=nstat)
    stats = (torch.arange(G * nstat, dtype=torch.float64).view(G, nstat) * 3.0 + 1.0)   # distinct per (row, stat)
    c.stats.set(stats)
    start = c.stat_acc.cpu()
    for mode in (0, 1):
        before = c.snap()
        assert c.launch(mode, stats=True, nstat=nstat) == 0
        c.check(before, written=("stat_acc", "grad") if mode == 1 else ("stat_acc", "params", "params_bf", "ctrl"))
    want = start.clone()
    want[:nstat] += 2.0 * stats.sum(0)
    got = c.stat_acc.cpu()
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    # mode 2, and a pass without stats, leave the totals alone
    before = c.snap()
    assert c.launch(2, stats=True, nstat=nstat) == 0
    c.check(before, written=("params", "params_bf", "ctrl"))
    before = c.snap()
    assert c.launch(1, stats=False) == 0
    c.check(before, written=("grad",))
    assert torch.equal(c.stat_acc.cpu(), want)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bf", [False, True], ids=_id)
def test_chunk_heads(native_built, bf, mode):
    """The slab pass (modes 0, 1) re-zeroes the 8 chunk-claim heads (stride 32 words); mode 2 does not."""
    c = Case(native_built, 160 if bf else 68, 3, bf)
    start = c.heads.cpu()
    before = c.snap()
    assert c.launch(mode, heads=True) == 0
    c.check(before, written=("heads",) + (("grad",) if mode == 1 else ("params", "params_bf", "ctrl")))
    want = start.clone()
    if mode != 2:
        want[0::32] = 0
    assert torch.equal(c.heads.cpu(), want)


# --------------------------------------------------------------------------- C. update arithmetic
def _state(P: int, kind: int, seed: int) -> dict:
    """A non-trivial optimizer state (cpu fp32): params around 0.1, a 0/1 mask, Adam m / v from three
    earlier random steps (zero where masked, as every masked update leaves them), AdaGrad acc >= 0.1."""
    gen = torch.Generator().manual_seed(seed)
    w = (0.1 + 0.05 * torch.randn(P, generator=gen)).float()
    mask = (torch.rand(P, generator=gen) < 0.75).float()
    mask[0] = 0.0
    mask[P - 1] = 0.0
    mask[1] = 1.0
    if kind == 2:
        b1, b2 = _f32(B1), _f32(B2)
        m = torch.zeros(P, dtype=torch.float64)
        v = torch.zeros(P, dtype=torch.float64)
        for _ in range(3):
            g = torch.randn(P, dtype=torch.float64, generator=gen) * mask
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
        s1, s2 = m.float(), v.float()
    else:
        s1 = (0.1 + torch.rand(P, generator=gen)).float()
        s2 = torch.rand(P, generator=gen).float()   # unused: must stay
    return {"params": w, "mask": mask, "s1": s1, "s2": s2}


def _ref_update(kind: int, st: dict, g: torch.Tensor, t: int):
    """One update in float64, hyper-parameters rounded to fp32 first (as the kernel receives them)."""
    lr, b1, b2, eps = _f32(LR), _f32(B1), _f32(B2), _f32(EPS)
    w, mask, s1, s2 = (st[k].double() for k in ("params", "mask", "s1", "s2"))
    gk = g * mask
    if kind == 1:
        s1 = s1 + gk * gk
        w = w - lr * gk / torch.sqrt(s1)
    elif kind == 2:
        s1 = b1 * s1 + (1 - b1) * gk
        s2 = b2 * s2 + (1 - b2) * gk * gk
        w = w - lr * (s1 / (1 - b1 ** t)) / (torch.sqrt(s2 / (1 - b2 ** t)) + eps) * mask
    else:
        w = w - lr * gk
    return w, s1, s2


def _img_map(P: int, seed: int):
    """A synthetic image map: ~1/3 bf16 elements (scattered over bytes [0, 4 nb)), ~1/3 fp32 words (scattered
    over the bytes behind them), the rest -1.  Returns (map int32 [P], image bytes)."""
    gen = torch.Generator().manual_seed(seed)
    nb = nw = max(1, P // 3)
    perm = torch.randperm(P, generator=gen)
    m = torch.full((P,), -1, dtype=torch.int32)
    m[perm[:nb]] = torch.randperm(2 * nb, generator=gen)[:nb].int()
    words = nb + torch.randperm(2 * nw, generator=gen)[:nw]
    m[perm[nb:nb + nw]] = (-words - 2).int()
    return m, 4 * (nb + 2 * nw)


def _img_expected(m: torch.Tensor, nbytes: int, w: torch.Tensor) -> torch.Tensor:
    """The image bytes after every mapped parameter of w (cpu fp32) was written into 0xA5 sentinels."""
    img = np.full(nbytes, 0xA5, dtype=np.uint8)
    mm = m.numpy()
    isb, isw = mm >= 0, mm <= -2
    img.view(np.int16)[mm[isb]] = bits(w.to(torch.bfloat16)).numpy()[isb]
    img.view(np.int32)[-mm[isw] - 2] = bits(w).numpy()[isw]
    return torch.from_numpy(img)


def _case_with_state(native, P, G, bf, st, seed) -> Case:
    """A Case holding state ``st``, a synthetic image map and a Polyak average off the parameters."""
    m, nbytes = _img_map(P, seed)
    c = Case(native, P, G, bf, img_bytes=nbytes).load(st)
    c.img_map.set(m)
    c.ema.set(st["params"] + 0.01)
    c.map_cpu, c.img_bytes = m, nbytes
    return c


def _gradient(c: Case, mode: int, seed: int):
    """Feed a gradient that reaches the update exactly: mode 2 reads grad (scale 0.5: a power of two);
    mode 0 reduces a slab of integers / 128 (exact sums).  Returns (scale, g float64 as the update sees it)."""
    if mode == 2:
        gen = torch.Generator().manual_seed(seed)
        grad = torch.randn(c.P, generator=gen).float()
        c.grad.set(grad)
        return 0.5, 0.5 * grad.double()
    g = _exact_g(c.G, c.P) / 128.0
    c.slab.set(_slab_layout(g, c.bf))
    return 0.5, 0.5 * g.sum(0)


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("bf,P", EDGE_CASES, ids=_id)
def test_update_matches_float64(native_built, bf, P, kind):
    """Modes 0 and 2 from a non-trivial state at ctrl[1] in {1, 2, 1000}.  Parameters within the project's
    rtol 1e-5 / atol 1e-6 of float64 (updates are ~1e-2: an O(1) error in the update fails); the states
    within a few roundings of their own operands; masked entries bit-unchanged."""
    k = KIND[kind]
    st = _state(P, k, seed=7 * P + k)
    keep = st["mask"] == 0
    for t in (1, 2, 1000):
        for mode in (0, 2):
            c = _case_with_state(native_built, P, 5, bf, st, seed=P)
            c.ctrl.set(torch.tensor([77, t]))
            scale, g = _gradient(c, mode, seed=P + t)
            before = c.snap()
            assert c.launch(mode, kind=k, scale=scale, ema=True, ema_decay=0.999, img=True) == 0
            written = ("params", "params_bf", "ctrl", "ema", "img") + ((), ("s1",), ("s1", "s2"))[k]
            c.check(before, written=written)
            w, s1, s2 = _ref_update(k, st, g, t)
            got = c.params.cpu()
            err = (got.double() - w).abs()
            assert (err <= 1e-6 + 1e-5 * w.abs()).all(), (kind, mode, t, float(err.max()))
            gk = g * st["mask"].double()
            if k == 1:
                e = (c.s1.cpu().double() - s1).abs()
                assert (e <= 3 * U * (st["s1"].double() + gk * gk)).all(), float(e.max())
            if k == 2:
                b1, b2 = _f32(B1), _f32(B2)
                e = (c.s1.cpu().double() - s1).abs()
                assert (e <= 4 * U * ((b1 * st["s1"].double()).abs() + ((1 - b1) * gk).abs())).all(), float(e.max())
                e = (c.s2.cpu().double() - s2).abs()
                assert (e <= 6 * U * ((b2 * st["s2"].double()).abs() + (1 - b2) * gk * gk)).all(), float(e.max())
            # masked entries do not drift; the bf16 copy is the rounded master; the step index is committed
            for name in ("params", "s1", "s2"):
                assert torch.equal(bits(c.b[name].cpu())[keep], bits(st[name])[keep]), name
            assert torch.equal(bits(c.params_bf.cpu())[keep], bits(st["params"].to(torch.bfloat16))[keep])
            assert torch.equal(bits(c.params_bf.cpu()), bits(got.to(torch.bfloat16)))
            assert c.ctrl.cpu().tolist() == [t, t]


def _random_slab(c: Case, seed: int) -> None:
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(c.G, c.P, dtype=torch.float64, generator=gen)
    c.slab.set(_slab_layout(g.to(torch.bfloat16 if c.bf else torch.float32).double(), c.bf))


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("bf", [False, True], ids=_id)
def test_mode0_equals_mode1_then_mode2(native_built, bf, kind):
    """One fused launch (mode 0, scale s) against reduce-only (mode 1, scale s) + update-only (mode 2,
    scale 1) on the written grad, from identical copies of one state: bit for bit."""
    k = KIND[kind]
    s = _f32(1.0 / 3.0)
    for P in (P_BF16 if bf else P_F32):
        st = _state(P, k, seed=11 * P + k)
        a = _case_with_state(native_built, P, 33, bf, st, seed=P)
        b = _case_with_state(native_built, P, 33, bf, st, seed=P)
        for c in (a, b):
            _random_slab(c, seed=3 * P)
            c.ctrl.set(torch.tensor([2, 3]))
        kw = dict(kind=k, ema=True, ema_decay=0.999, img=True)
        assert a.launch(0, scale=s, **kw) == 0
        assert b.launch(1, scale=s, **kw) == 0
        assert b.launch(2, scale=1.0, **kw) == 0
        for name in ("params", "params_bf", "s1", "s2", "ema", "img", "ctrl"):
            assert torch.equal(a.b[name].snap(), b.b[name].snap()), (P, name)
        assert not torch.equal(a.params.cpu(), st["params"])


@pytest.mark.parametrize("t", [1, 5])
@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
def test_tdelay(native_built, kind, t):
    """ctrl[1] = t + 1 with tdelay = 1 applies update number t (overlapped data parallelism applies
    step t's gradient during step t + 1): bit-equal to ctrl[1] = t, tdelay = 0 on everything but ctrl."""
    k = KIND[kind]
    for bf, P, mode in ((False, 68, 2), (True, 160, 0)):
        st = _state(P, k, seed=13 * P + k)
        a = _case_with_state(native_built, P, 5, bf, st, seed=P)
        b = _case_with_state(native_built, P, 5, bf, st, seed=P)
        a.ctrl.set(torch.tensor([t, t + 1]))
        b.ctrl.set(torch.tensor([t - 1, t]))
        for c, td in ((a, 1), (b, 0)):
            scale, _ = _gradient(c, mode, seed=P)
            assert c.launch(mode, kind=k, scale=scale, ema=True, ema_decay=0.9, img=True, tdelay=td) == 0
        for name, band in a.b.items():
            if name != "ctrl":
                assert torch.equal(band.snap(), b.b[name].snap()), (P, name)
        assert a.ctrl.cpu().tolist() == [t + 1, t + 1] and b.ctrl.cpu().tolist() == [t, t]


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_polyak_average(native_built, decay):
    """ema' = ema + (1 - decay) (w' - ema) within 3 * 2^-24 (|ema| + |w'|) of float64 (one rounding of the
    difference, one of the fused multiply-add); with ema = None nothing is written."""
    d = _f32(decay)
    for bf, P, mode in ((False, 68, 2), (True, 160, 0)):
        st = _state(P, 2, seed=17 * P)
        for with_ema in (True, False):
            c = _case_with_state(native_built, P, 5, bf, st, seed=P)
            gen = torch.Generator().manual_seed(P)
            ema0 = (st["params"] + 0.01 * torch.randn(P, generator=gen)).float()
            c.ema.set(ema0)
            scale, _ = _gradient(c, mode, seed=P)
            before = c.snap()
            assert c.launch(mode, kind=2, scale=scale, ema=with_ema, ema_decay=decay) == 0
            c.check(before, written=("params", "params_bf", "ctrl", "s1", "s2") + (("ema",) if with_ema else ()))
            if with_ema:
                w = c.params.cpu().double()
                ref = ema0.double() + (1 - d) * (w - ema0.double())
                e = (c.ema.cpu().double() - ref).abs()
                assert (e <= 3 * U * (ema0.double().abs() + w.abs())).all(), float(e.max())
                assert not torch.equal(c.ema.cpu(), ema0)


@pytest.mark.parametrize("bf,P", EDGE_CASES, ids=_id)
def test_weight_image(native_built, bf, P):
    """The update keeps the ws weight image current through img_map: entries >= 0 are bf16 elements,
    <= -2 fp32 words (-d - 2), -1 not in the image.  Mapped places hold bf16(w') / w' bitwise, every other
    byte keeps the sentinel, and img_pack of the updated parameters gives the same bytes."""
    native = native_built
    st = _state(P, 1, seed=19 * P)
    for mode in (0, 2):
        c = _case_with_state(native, P, 5, bf, st, seed=23 * P + mode)
        scale, _ = _gradient(c, mode, seed=P)
        before = c.snap()
        assert c.launch(mode, kind=1, scale=scale, img=True) == 0
        c.check(before, written=("params", "params_bf", "ctrl", "s1", "img"))
        w = c.params.cpu()
        assert not torch.equal(w, st["params"])
        want = _img_expected(c.map_cpu, c.img_bytes, w)
        assert torch.equal(c.img.cpu(), want)
        fresh = Band(c.img_bytes, torch.uint8, 0x3C).set(0xA5)
        native.img_pack(c.params.v, c.img_map.v, fresh.v)
        torch.cuda.synchronize()
        assert fresh.guards_intact()
        assert torch.equal(fresh.cpu(), want)


# --------------------------------------------------------------------------- D. to_bf16, rejections
_SPECIAL_BITS = [
    0x00000000, 0x80000000,                  # +-0
    0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x007F8000,   # denormals (a tie among them)
    0x7F7FFFFF, 0xFF7FFFFF,                  # largest finite: rounds to inf
    0x7F800000, 0xFF800000,                  # +-inf
    0x7FC00000,                              # NaN
    0x3F808000, 0x3F818000,                  # exact ties: to even, down and up
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,               # their neighbours
    0xBF808000, 0xBF818000, 0x7F7F8000, 0x7F7F7FFF,
]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_to_bf16(native_built, n):
    """fp32 -> bf16 round-to-nearest-even over zeros, denormals, the largest finite value, infinities, a
    NaN, exact ties and their neighbours (and random bit patterns), bit-equal to torch's conversion."""
    rng = np.random.default_rng(n)
    sp = np.array(_SPECIAL_BITS, dtype=np.uint32)
    for shift in range(len(sp) if n == 1 else 1):   # n = 1 sees every special in turn
        pat = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        pat[(pat & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)   # random patterns stay finite
        k = min(n, len(sp))
        pat[:k] = np.roll(sp, -shift)[:k]
        x = torch.from_numpy(pat.view(np.float32).copy())
        src = Band(n, torch.float32, NAN).set(x)
        dst = Band(n, torch.bfloat16, -7776.0).set(1.0)
        before = src.snap()
        native_built.to_bf16(src.v, dst.v)
        torch.cuda.synchronize()
        assert dst.guards_intact() and src.same(before)
        got, want = dst.cpu(), x.to(torch.bfloat16)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(bits(got)[~nan], bits(want)[~nan]), (n, shift)


def test_launcher_rejections(native_built):
    """st_reduce_optim refuses these before any launch; every buffer stays bit-unchanged."""
    def rejected(c, *a, **kw):
        before = c.snap()
        rc = c.launch(*a, **kw)
        c.check(before)
        return rc != 0

    c = Case(native_built, 6, 3, False)          # fp32 slabs: one float4 per thread column
    for mode in (0, 1, 2):
        assert rejected(c, mode), ("P % 4", mode)
    c = Case(native_built, 48, 3, True)          # bf16 slabs: whole 32-parameter column blocks
    for mode in (0, 1):
        assert rejected(c, mode), ("P % 32", mode)
    for bf, P in ((False, 64), (True, 128)):
        c = Case(native_built, P, 3, bf, nstat=9)
        for nstat in (0, 9):
            assert rejected(c, 1, stats=True, nstat=nstat), ("nstat", nstat)
        for mode in (0, 1, 2):
            assert rejected(c, mode, null=("mask",)), ("mask", mode)
            assert rejected(c, mode, null=("params",)), ("params", mode)
        assert c.launch(1, stats=True, nstat=8) == 0   # the same buffers with valid arguments run
