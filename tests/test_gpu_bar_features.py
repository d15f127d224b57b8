"""The raw-bar kernels (``csrc/bar_features.hip``) on the GPU: the generator with its OHLCV planes is the
generator; the tiled kernel and the one-thread-per-series kernel agree bit for bit; pieces and the one-bar-per-launch
sessions kernel reproduce the whole; the unrounded rows are as close to the float64 reference as the float32 host
reference is; serving raw bars equals serving the batch kernel's rows; and a learner on an external bank that holds
the default bank trains as the default learner does, bit for bit on the ordered update.

Shapes: N in {3, 64, 67} series (below a wave: the fallback; one full wave; a full wave beside a ragged one) of
T = 2 * 13 + 7 bars in sessions of 13 (a tile's ragged end; two session starts).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DAY = 13
T = 2 * DAY + 7
NMAX = 67
DEV = torch.device("cuda", 0)
NAMES = ("ret", "range", "pos", "logvol", "sin", "cos", "mom", "sig")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


_data = {}


def _case():
    """67 series from the generator on the device (host copies of the planes), parameters fitted on them, and the
    batch kernel's result on all of them: computed once, shared, never modified."""
    if not _data:
        from sharetrade.data import minute_bars as mb
        from sharetrade.data import ohlcv as ov

        bp = mb.BarParams(day=DAY)
        gb, gfeat = ov.generate_ohlcv_gpu(NMAX, T, DEV, bp, seed=11)
        close0, feat0 = mb.generate_gpu(NMAX, T, DEV, bp, seed=11)
        torch.cuda.synchronize()
        bars = ov.Bars(*(getattr(gb, k).cpu().numpy() for k in ov.PLANES), minute=gb.minute)
        fp = ov.fit_feature_params(bars, day=DAY)
        whole = ov.featurise_gpu(bars, fp, DEV, want32=True)
        torch.cuda.synchronize()
        _data.update(bars=bars, gfeat=gfeat, close0=close0, feat0=feat0, fp=fp, whole=whole)
    return _data


def _sub(n):
    """The first n series of the case: bars and parameters."""
    from sharetrade.data import ohlcv as ov

    d = _case()
    b, fp = d["bars"], d["fp"]
    return (ov.Bars(*(getattr(b, k)[:n] for k in ov.PLANES), minute=b.minute),
            ov.FeatureParams(fp.day, fp.alpha, fp.beta, fp.sigma[:n], fp.vol_scale[:n]))


def test_generator_with_ohlcv_is_the_generator(native_built):
    d = _case()
    assert _same(torch.from_numpy(d["bars"].close), d["close0"]) and _same(d["gfeat"], d["feat0"])
    b = d["bars"]
    assert np.array_equal(b.open[:, 1:], b.close[:, :-1])
    assert np.all(b.high >= np.maximum(b.open, b.close)) and np.all(b.low <= np.minimum(b.open, b.close))
    assert np.all(b.volume > 0)


@pytest.mark.parametrize("n", [3, 64, 67])
def test_tiled_and_fallback_paths_agree_bitwise(native_built, n):
    from sharetrade.data import ohlcv as ov
    from sharetrade.ops import bar_features as BF

    whole = _case()["whole"]
    bars, fp = _sub(n)
    outs = {v: ov.featurise_gpu(bars, fp, DEV, want32=True, variant=v) for v in (BF.AUTO, BF.NAIVE, BF.TILED)}
    torch.cuda.synchronize()
    for v, r in outs.items():
        # the same series give the same bits whichever kernel and whichever neighbours (n = 3: the fallback
        # against the tiled kernel's rows of the 67-series launch)
        assert _same(r.feat, whole.feat[:n]) and _same(r.feat32, whole.feat32[:n]), (n, v)
        assert _same(r.state, whole.state[:n]) and _same(r.close, whole.close[:n]), (n, v)
    assert _same(outs[BF.AUTO].close, torch.from_numpy(bars.close))
    assert _same(outs[BF.AUTO].feat, outs[BF.AUTO].feat32.to(torch.bfloat16))
    assert torch.isfinite(whole.feat32).all()


@pytest.mark.parametrize("n", [3, 67])
def test_pieces_equal_the_whole_bitwise(native_built, n):
    from sharetrade.data import ohlcv as ov

    whole = _case()["whole"]
    bars, fp = _sub(n)
    st, feats, closes = None, [], []
    cuts = [0, 1, 7, DAY, T]
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = ov.featurise_gpu(bars.piece(a, b), fp, DEV, state=st)
        st = r.state
        feats.append(r.feat)
        closes.append(r.close)
    torch.cuda.synchronize()
    assert _same(torch.cat(feats, dim=1), whole.feat[:n]) and _same(torch.cat(closes, dim=1), whole.close[:n])
    assert _same(st, whole.state[:n])


def test_replay_of_the_generator_on_the_device(native_built):
    """The kernel on the device generator's own bars with the true parameters: the five direct features are the
    generator's bf16 bits; ret / mom / sig within the host test's bounds (twice the rounding bound of a return taken
    from the float32 close) plus the half ulp of the bf16 rows the generator stores."""
    from sharetrade.data import minute_bars as mb
    from sharetrade.data import ohlcv as ov

    d = _case()
    r = ov.featurise_gpu(d["bars"], ov.true_params(NMAX, mb.BarParams(day=DAY)), DEV, want32=True)
    torch.cuda.synchronize()
    gen, got = d["gfeat"].cpu(), r.feat.cpu()
    for i in (1, 2, 3, 4, 5):
        assert _same(got[:, :, i], gen[:, :, i]), NAMES[i]
    f32, g = r.feat32.cpu(), gen.float()
    half_ulp = g.abs() * 2.0 ** -8
    assert bool(((f32[:, :, 0] - g[:, :, 0]).abs() <= 4e-5 + half_ulp[:, :, 0]).all())
    assert bool(((f32[:, :, 6] - g[:, :, 6]).abs() <= 2e-4 + half_ulp[:, :, 6]).all())
    assert bool(((f32[:, :, 7] - g[:, :, 7]).abs() <= (1e-4 + 2.0 ** -8) * g[:, :, 7]).all())


def test_accuracy_against_float64(native_built):
    """Per feature, the kernel's largest error against the float64 reference is at most twice the float32 host
    reference's on the same input (the factor allows for the device's logf / sinf / cosf ulps)."""
    from sharetrade.data import ohlcv as ov

    d = _case()
    ref64 = ov.featurise_numpy(d["bars"], d["fp"], dtype=np.float64).feat
    ref32 = ov.featurise_numpy(d["bars"], d["fp"]).feat
    gpu = d["whole"].feat32.cpu().numpy()
    e_gpu = np.abs(gpu.astype(np.float64) - ref64).max(axis=(0, 1))
    e_ref = np.abs(ref32.astype(np.float64) - ref64).max(axis=(0, 1))
    for i, n in enumerate(NAMES):
        print(f"{n}: kernel {e_gpu[i]:.3g}  float32 numpy {e_ref[i]:.3g}")
    for i, n in enumerate(NAMES):
        assert e_gpu[i] <= 2.0 * e_ref[i], (n, e_gpu[i], e_ref[i])


def _sessions_run():
    """B = 5 request rows (four sessions in a permutation that changes every launch, one -1 padding row) over T
    launches of the sessions kernel, against the batch kernel on the same four series."""
    if "sessions" not in _data:
        import ctypes as C

        from sharetrade.ops import bar_features as BF
        from sharetrade.ops import native

        bars, fp = _sub(4)
        S = 9
        slots_of = [7, 2, 5, 0]                 # series i lives in slot slots_of[i]
        table = torch.zeros(S, BF.NSTATE, device=DEV)
        table[torch.tensor(slots_of, device=DEV)] = torch.from_numpy(fp.initial_state()).to(DEV)
        untouched = table.clone()
        X = np.stack([getattr(bars, k) for k in ("open", "high", "low", "close", "volume")], axis=2)   # [4, T, 5]
        M = bars.minutes(DAY)
        feat = torch.zeros(T, 4, BF.NF, dtype=torch.bfloat16, device=DEV)
        close = torch.zeros(T, 4, device=DEV)
        g = np.random.default_rng(0)
        pad_ok = True
        for t in range(T):
            order = list(g.permutation(4))
            pad = int(g.integers(0, 5))
            rows = order[:pad] + [-1] + order[pad:]             # series of each request row, -1 = padding
            slot = torch.tensor([slots_of[i] if i >= 0 else -1 for i in rows], dtype=torch.int32, device=DEV)
            nan = np.full(5, np.nan, np.float32)
            x = torch.from_numpy(np.stack([X[i, t] if i >= 0 else nan for i in rows])).to(DEV)
            m = torch.tensor([int(M[i, t]) if i >= 0 else 0 for i in rows], dtype=torch.int32, device=DEV)
            f = torch.full((5, BF.NF), -7.0, dtype=torch.bfloat16, device=DEV)
            c = torch.full((5,), -7.0, device=DEV)
            a = BF.BarSessionsArgs(slot.data_ptr(), x.data_ptr(), m.data_ptr(), table.data_ptr(), f.data_ptr(),
                                   c.data_ptr(), 5, S, DAY, fp.alpha, fp.beta)
            native.check(BF.lib().st_bar_features_sessions(C.byref(a), native.stream_handle()), "sessions")
            torch.cuda.synchronize()
            for r, i in enumerate(rows):
                if i >= 0:
                    feat[t, i], close[t, i] = f[r], c[r]
                else:
                    pad_ok = pad_ok and bool((f[r] == -7.0).all()) and float(c[r]) == -7.0
        _data["sessions"] = (feat.transpose(0, 1), close.transpose(0, 1), table, untouched, slots_of, pad_ok)
    return _data["sessions"]


def test_sessions_kernel_equals_the_batch_kernel_bitwise(native_built):
    whole = _case()["whole"]
    feat, close, table, untouched, slots_of, pad_ok = _sessions_run()
    assert _same(feat, whole.feat[:4]) and _same(close, whole.close[:4])
    assert _same(table[torch.tensor(slots_of, device=DEV)], whole.state[:4])
    rest = [s for s in range(table.shape[0]) if s not in slots_of]
    assert _same(table[rest], untouched[rest]) and pad_ok       # a padding row touches nothing


def test_step_raw_equals_step_on_the_batch_kernels_rows(native_built):
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.serve.gru_serve import GruSessionServer

    whole = _case()["whole"]
    n = 5
    bars, fp = _sub(n)
    pol = GruPolicy(gq.init_params(5), device=DEV, seed=5)
    a = GruSessionServer(pol, 16, ep_len=10, backend="hip", bar_day=DAY)
    b = GruSessionServer(pol, 16, ep_len=10, backend="hip", bar_day=DAY)
    sa, sb = a.open_raw(n, fp.sigma, fp.vol_scale), b.open(n)
    assert sa == sb
    X = np.stack([getattr(bars, k) for k in ("open", "high", "low", "close", "volume")], axis=2)
    M = bars.minutes(DAY)
    perm = np.array([3, 0, 4, 1, 2])
    for t in range(T):
        order = perm if t % 2 else np.arange(n)
        sl = [sa[i] for i in order]
        fresh = np.full(n, t == DAY)
        idx = torch.from_numpy(order).to(DEV)
        da = a.step_raw(sl, X[order, t], M[order, t], new_episode=fresh, return_q=True)
        db = b.step(sl, whole.feat[idx, t], whole.close[idx, t], new_episode=fresh, return_q=True)
        torch.cuda.synchronize()
        assert torch.equal(da.actions, db.actions) and torch.equal(da.position, db.position), t
        assert _same(da.reward, db.reward) and _same(da.q, db.q), t
    assert _same(a.fstate[torch.tensor(sa, device=DEV)], whole.state[:n])
    assert torch.equal(a.table["rec"], b.table["rec"]) and _same(a.table["h"], b.table["h"])
    plain = a.open(1)
    before = a.batches
    with pytest.raises(ValueError, match="open_raw"):
        a.step_raw(plain, X[:1, 0], M[:1, 0])
    assert a.batches == before


_trained = {}
ADAM_KEYS = ("flat", "mflat", "vflat")   # the parameters and their Adam moments
# what depends on the weights (tests/test_gpu_runs.py): the update sums its gradients with atomics, so two runs of one
# learner agree in these to fp32 reduction-order noise, not bit for bit
WEIGHTY = ADAM_KEYS + ("tflat", "h", "rh0", "loss", "stats")


def _learners(eps, deterministic=False):
    """A default learner, a second default learner of the same seed, and a learner on an external bank that holds
    the default bank, three iterations each (E = 64): trained once per setting, shared."""
    key = (eps, deterministic)
    if key not in _trained:
        from sharetrade.config import preset_config
        from sharetrade.trainer.recurrent import RecurrentDQN

        def learner(**kw):
            cfg = preset_config("recurrent")
            if eps is not None:
                cfg.agent.epsilon = eps
            return RecurrentDQN(cfg, DEV, envs=64, seq=4, burn_in=1, bars=600, ep_len=5, batch=128,
                                replay_segments=1024, deterministic=deterministic, **kw)

        w0 = learner().flat.clone()
        d0, twin = learner(), learner()
        d1 = learner(bank=(d0.close.clone(), d0.feat.clone()))
        for d in (d0, twin, d1):
            for _ in range(3):
                d.iteration(1)
        torch.cuda.synchronize()
        _trained[key] = dict(d0=d0, twin=twin, d1=d1, w0=w0, make=learner)
    return _trained[key]


def test_external_bank_changes_nothing_else(native_built):
    """With epsilon 0 every action is a Philox draw, so the trajectories do not depend on Q: envs, the replay ring
    (its rows are the bank's features, its rewards the bank's closes) and every counter are bit-equal to the default
    learner's after three iterations; what depends on the weights agrees within the bound tests/test_gpu_runs.py
    holds a resumed run to (see the next test for why not bit for bit)."""
    t = _learners(0.0)
    d0, d1 = t["d0"], t["d1"]
    assert d1.external_bank and not d0.external_bank
    s0, s1 = d0.state_dict(), d1.state_dict()
    assert s0.keys() == s1.keys()
    for k in s0:
        if k in WEIGHTY:
            assert torch.allclose(s0[k].float(), s1[k].float(), rtol=1e-4, atol=1e-5), k
        else:
            assert _same(s0[k], s1[k]) if s0[k].is_floating_point() else torch.equal(s0[k], s1[k]), k
    assert d0.stats_dict()["env_steps"] == d1.stats_dict()["env_steps"] > 0
    assert not torch.allclose(d0.flat, t["w0"], rtol=1e-4, atol=1e-5)     # three iterations did train
    with pytest.raises(ValueError, match="external bank"):
        d1.backtest()
    with pytest.raises(ValueError, match="bank close"):
        t["make"](bank=(d0.close[:, :-1].contiguous(), d0.feat))
    assert d1.backtest(d0.close, d0.feat).steps == 599


def test_external_bank_parameters_are_bit_equal(native_built):
    """After three iterations the parameters, Adam moments, target net and stats of the learner on the external bank
    are bit-equal to those of the default learner of the same seed (default epsilon, E = 64).

    Both learners run the ordered update (``deterministic=True``: no split-K in the weight-gradient GEMMs, the
    Q-head gradient summed per workgroup and then in order).  The default update sums those gradients with atomics,
    so its bits depend on the order in which workgroups arrive: measured on an MI355X over five runs, two default
    learners of ONE seed, neither with a bank, differed by 1.9e-9 to 2.6e-7 in their parameters after the first
    iteration, and the bank learner differed from them by the same amounts -- a bit-equality check on that path
    fails whatever the bank path does (tests/test_gpu_runs.py holds a resumed run to that noise).  On the ordered
    path a second default learner is bit-equal too, which is what makes the comparison with the bank learner say
    something."""
    t = _learners(None, deterministic=True)
    d0, d1, twin = t["d0"], t["d1"], t["twin"]
    for name, x in (("bank", d1), ("second default learner", twin)):
        for k in ADAM_KEYS:
            diff = float((getattr(d0, k) - getattr(x, k)).abs().max())
            print(f"{name} vs default, {k}: max abs difference {diff:.3g}")
    assert d1.external_bank and d1.deterministic and d0.deterministic
    for x in (d1, twin):
        assert _same(d0.stats, x.stats)
        for k in ADAM_KEYS + ("tflat", "h"):
            assert _same(getattr(d0, k), getattr(x, k)), k
    assert not torch.allclose(d0.flat, t["w0"], rtol=1e-4, atol=1e-5)     # three iterations did train
    # the ordered update computes what the default update computes, up to that reduction-order noise
    ref = _learners(None)["d0"]
    assert torch.allclose(d0.flat, ref.flat, rtol=1e-4, atol=1e-5)


def test_ordered_update_is_bit_reproducible_under_hip_graphs(native_built):
    """The ordered update captured into HIP graphs with the actor beside it (``overlap_act``): two learners of one
    seed hold bit-equal parameters after the captured warm-up and three replayed iterations."""
    from sharetrade.config import preset_config
    from sharetrade.trainer.recurrent import RecurrentDQN

    def run():
        d = RecurrentDQN(preset_config("recurrent"), DEV, envs=64, seq=4, burn_in=1, bars=600, ep_len=5, batch=256,
                         replay_segments=1024, overlap_act=True, deterministic=True)
        d.capture()
        for _ in range(3):
            d.iteration(1)
        torch.cuda.synchronize()
        return d

    a, b = run(), run()
    assert a.updates == b.updates == 4
    for k in ADAM_KEYS + ("tflat",):
        assert _same(getattr(a, k), getattr(b, k)), k
    assert _same(a.stats, b.stats)
