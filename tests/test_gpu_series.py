"""csrc/series.hip: random_walk_kernel against a float64 mirror, replicate4_kernel against indexing.

random_walk_kernel generates the price bank of every synthetic run.  One wave makes one series, 64 days
at a time: Philox4x32-10 at counter (row, t, 0x5EED, 2), a Box-Muller normal from its first two words,
a wave scan of the log-returns, and a carry of the log-price into the next 64-day block.  The mirror
below states that definition in float64 with a plain cumulative sum, so a lost carry, a wrong increment
at t == 0, a wrong counter word or an error when T % 64 != 0 shows as a deviation orders of magnitude
above rounding.  replicate4_kernel makes the shifted / padded copies every bf16 step kernel gathers its
windows from: dst[s][e][i] = src[e][i + s], 0 past the end.

Outputs sit in guard bands (tests/guard_band.py): a sentinel behind the last element must survive.
"""
import functools

import numpy as np
import pytest
import torch

from guard_band import Band, bits
from sharetrade.utils.rng import philox4x32

pytestmark = pytest.mark.gpu

START, VOL, KEY0, KEY1 = 50.0, 0.02, 123, 456
ES = [1, 3, 4, 5]                       # four waves (series) per workgroup
TS = [1, 2, 63, 64, 65, 128, 129, 200]  # around the 64-day block
WALKS = [(e, t, 0.0) for e in ES for t in TS] + [(5, 200, 1e-3), (3, 129, -2e-3)]
SENTINEL = -7777.0


def _uniform_words(E: int, T: int, k0: int, k1: int):
    n = E * T
    row = np.repeat(np.arange(E, dtype=np.uint32), T)
    t = np.tile(np.arange(T, dtype=np.uint32), E)
    c0, c1, _, _ = philox4x32(row, t, np.full(n, 0x5EED, np.uint32), np.full(n, 2, np.uint32),
                              np.full(n, k0, np.uint32), np.full(n, k1, np.uint32))
    return (c0 >> np.uint32(8)).reshape(E, T), (c1 >> np.uint32(8)).reshape(E, T)


def _walk(E: int, T: int, start: float, vol: float, drift: float, k0: int, k1: int, ft):
    """The bank's definition in precision ``ft`` (float64: the mirror; float32: the plain reference whose
    own rounding sets the tolerance), with a sequential cumulative sum.  Scalars as the kernel receives
    them (rounded to fp32)."""
    a, b = _uniform_words(E, T, k0, k1)
    u1 = (a.astype(ft) + ft(1)) * ft(2.0 ** -24)
    u2 = b.astype(ft) * ft(2.0 ** -24)
    z = np.sqrt(ft(-2) * np.log(u1)) * np.cos(ft(np.float32(6.283185307179586)) * u2)
    inc = ft(np.float32(vol)) * z + ft(np.float32(drift))
    inc[:, 0] = 0
    lp = np.cumsum(inc, axis=1, dtype=ft)
    out = ft(np.float32(start)) * np.exp(lp)
    assert out.dtype == ft
    return out


def _dev(a, ref64) -> float:
    return float(np.abs(np.log(np.asarray(a, dtype=np.float64) / ref64)).max())


@functools.lru_cache(maxsize=None)
def _mirror(E, T, drift, k0=KEY0, k1=KEY1):
    return _walk(E, T, START, VOL, drift, k0, k1, np.float64)


@functools.lru_cache(maxsize=None)
def _fp32_reference_dev() -> float:
    """Largest |log(fp32 formula / float64 mirror)| over the tested shapes."""
    return max(_dev(_walk(e, t, START, VOL, d, KEY0, KEY1, np.float32), _mirror(e, t, d)) for e, t, d in WALKS)


def _run_walk(native, E, T, drift=0.0, k0=KEY0, k1=KEY1) -> torch.Tensor:
    band = Band(E * T, torch.float32, SENTINEL).set(SENTINEL)
    native.random_walk(band.v.view(E, T), START, VOL, drift, k0, k1)
    torch.cuda.synchronize()
    assert band.guards_intact(), (E, T)
    out = band.cpu().view(E, T)
    assert torch.isfinite(out).all() and (out > 0).all(), (E, T)
    return out


def test_random_walk_matches_float64_mirror(native_built):
    """|log(kernel / mirror)| <= 8 x the deviation of the same formula in numpy float32 with a sequential
    fp32 cumulative sum.  The margin covers the device's logf / cosf / expf against numpy's and the wave
    scan's summation order; a lost carry or a wrong counter word is >= 1e4 x above it."""
    ref_dev = _fp32_reference_dev()
    worst = 0.0
    for E, T, drift in WALKS:
        out = _run_walk(native_built, E, T, drift)
        assert (out[:, 0] == START).all(), (E, T)
        d = _dev(out.numpy(), _mirror(E, T, drift))
        worst = max(worst, d)
        assert d <= 8.0 * ref_dev, (E, T, drift, d, ref_dev)
    print(f"[meas] random_walk fp32-reference deviation |log(ref32 / ref64)| = {ref_dev:.3e}")
    print(f"[meas] random_walk kernel deviation |log(kernel / ref64)| = {worst:.3e} (limit {8.0 * ref_dev:.3e})")


def test_random_walk_structure(native_built):
    """A row depends only on (row, day, keys): no tolerance."""
    e5 = _run_walk(native_built, 5, 130)
    e3 = _run_walk(native_built, 3, 130)
    assert torch.equal(bits(e3), bits(e5[:3]))
    for t1, t2 in ((63, 64), (64, 65), (100, 130), (129, 200)):
        a, b = _run_walk(native_built, 4, t1), _run_walk(native_built, 4, t2)
        assert torch.equal(bits(a), bits(b[:, :t1])), (t1, t2)
    other = _run_walk(native_built, 5, 130, k0=KEY0 + 1)
    other1 = _run_walk(native_built, 5, 130, k1=KEY1 + 1)
    for r in range(5):
        assert not torch.equal(e5[r, 1:], other[r, 1:]) and not torch.equal(e5[r, 1:], other1[r, 1:])
        for q in range(r):
            assert not torch.equal(e5[r, 1:], e5[q, 1:])


# --------------------------------------------------------------------------- replicate4
def _src(E: int, T: int) -> torch.Tensor:
    return (torch.arange(E * T, dtype=torch.float32).view(E, T) * 0.25 + 1.0)   # distinct per (e, t), non-zero


def _replicas(src: torch.Tensor, reps: int, T4: int) -> torch.Tensor:
    E, T = src.shape
    want = torch.zeros(reps, E, T4)
    for s in range(reps):
        want[s, :, :max(T - s, 0)] = src[:, s:]
    return want


@pytest.mark.parametrize("T", [1, 5, 201, 260])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("reps", [1, 4])
def test_replicate4(native_built, reps, E, T):
    """out[s, e, i] == src[e, i + s] for i + s < T and 0 elsewhere, bit-equal."""
    native = native_built
    src = Band(E * T, torch.float32, float("nan")).set(_src(E, T))
    out = native.replicate4(src.v.view(E, T), reps)
    torch.cuda.synchronize()
    T4 = native.replica_stride(T)
    assert tuple(out.shape) == (reps, E, T4)
    want = _replicas(_src(E, T), reps, T4)
    assert torch.equal(bits(out.cpu()), bits(want))
    # the same launch into a guard band: nothing behind reps * E * T4 is written, the source is only read
    T4 = (T + 3) // 4 * 4   # the smallest stride the launcher accepts
    before = src.snap()
    dst = Band(reps * E * T4, torch.float32, SENTINEL).set(SENTINEL)
    assert native.lib().st_replicate4(src.ptr(), dst.ptr(), E, T, T4, reps, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert dst.guards_intact() and src.same(before)
    assert torch.equal(bits(dst.cpu().view(reps, E, T4)), bits(_replicas(_src(E, T), reps, T4)))


def test_replicate4_rejections(native_built):
    native = native_built
    E, T = 3, 5
    src = Band(E * T, torch.float32, float("nan")).set(_src(E, T))
    dst = Band(4 * E * 8, torch.float32, SENTINEL).set(SENTINEL)
    before = dst.snap()
    for T4, reps in ((6, 1), (4, 1), (8, 0), (8, 5)):   # T4 % 4 != 0, T4 < T, reps out of 1..4
        assert native.lib().st_replicate4(src.ptr(), dst.ptr(), E, T, T4, reps, native.stream_handle()) != 0, (T4, reps)
    torch.cuda.synchronize()
    assert dst.same(before)
    assert native.lib().st_replicate4(src.ptr(), dst.ptr(), E, T, 8, 4, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu().view(4, E, 8), _replicas(_src(E, T), 4, 8))
