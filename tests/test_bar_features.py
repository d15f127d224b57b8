"""Raw OHLCV minute bars -> the GRU(256) policy's feature rows (``sharetrade/data/ohlcv.py``), on the host: replaying
the generator's own bars recovers the generator's features, pieces and bar-by-bar streaming reproduce the whole bit
for bit, the parameters see only the bars they may, the loaders round-trip, and the command line and the session
server take raw bars on the ``torch`` backend."""
import json
import math

import numpy as np
import pytest
import torch

from sharetrade.data import minute_bars as mb
from sharetrade.data import ohlcv as ov

DAY = 13
T = 2 * DAY + 7


@pytest.fixture(scope="module")
def replay():
    """The generator's bars (E = 32, T = 1200, seed 3), its features, and the replay with the true parameters."""
    bars, feat = ov.generate_ohlcv_numpy(32, 1200, seed=3)
    close, gen = mb.generate_numpy(32, 1200, seed=3)
    return bars, feat, close, gen, ov.featurise_numpy(bars, ov.true_params(32))


@pytest.fixture(scope="module")
def small():
    """Bars of short sessions (day = 13, T = 2 * day + 7) with parameters fitted on them."""
    bp = mb.BarParams(day=DAY)
    bars, _ = ov.generate_ohlcv_numpy(5, T, bp, seed=11)
    return bars, ov.fit_feature_params(bars, day=DAY)


def test_generator_with_ohlcv_is_the_generator(replay):
    bars, feat, close, gen, _ = replay
    assert np.array_equal(bars.close, close) and np.array_equal(feat, gen)
    assert np.all(bars.high >= np.maximum(bars.open, bars.close))
    assert np.all(bars.low <= np.minimum(bars.open, bars.close))
    assert np.array_equal(bars.open[:, 1:], bars.close[:, :-1])


def test_replay_recovers_the_generator(replay):
    """Bounds: twice the rounding bound of a return taken from the float32 close (3 * 2^-24 * 100 = 1.8e-5 absolute;
    the momentum sums five)."""
    bars, _, close, gen, r = replay
    assert r.close.dtype == np.float32 and np.array_equal(r.close, close)
    for i in (1, 2, 3, 4, 5):
        assert np.array_equal(r.feat[:, :, i], gen[:, :, i]), i
    err_ret = np.abs(r.feat[:, :, 0] - gen[:, :, 0]).max()
    err_mom = np.abs(r.feat[:, :, 6] - gen[:, :, 6]).max()
    err_sig = (np.abs(r.feat[:, :, 7] - gen[:, :, 7]) / gen[:, :, 7]).max()
    print(f"replay: ret {err_ret:.3g} abs, mom {err_mom:.3g} abs, sig {err_sig:.3g} rel")
    assert err_ret <= 4e-5 and err_mom <= 2e-4 and err_sig <= 1e-4


def test_pieces_equal_the_whole_bitwise(small):
    bars, fp = small
    whole = ov.featurise_numpy(bars, fp)
    cuts = [0, 1, 7, DAY, T]
    st, feats, closes = None, [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = ov.featurise_numpy(bars.piece(a, b), fp, state=st)
        st = r.state
        feats.append(r.feat)
        closes.append(r.close)
    assert np.array_equal(np.concatenate(feats, axis=1).view(np.uint32), whole.feat.view(np.uint32))
    assert np.array_equal(np.concatenate(closes, axis=1), whole.close)
    assert np.array_equal(st.view(np.uint32), whole.state.view(np.uint32))


def test_streaming_equals_the_whole_bitwise(small):
    bars, fp = small
    whole = ov.featurise_numpy(bars, fp)
    st = None
    for t in range(T):
        r = ov.featurise_numpy(bars.piece(t, t + 1), fp, state=st)
        st = r.state
        assert np.array_equal(r.feat[:, 0].view(np.uint32), whole.feat[:, t].view(np.uint32)), t
    assert np.array_equal(st.view(np.uint32), whole.state.view(np.uint32))


def test_minute_zero_takes_open_as_the_reference_price(small):
    bars, fp = small
    gap = ov.Bars(bars.open.copy(), bars.high.copy(), bars.low.copy(), bars.close.copy(), bars.volume.copy(),
                  minute=bars.minute)
    gap.open[:, DAY] *= np.float32(1.25)    # an overnight gap before the second session
    gap.high[:, DAY] = np.maximum(gap.high[:, DAY], gap.open[:, DAY])
    r = ov.featurise_numpy(gap, fp)
    want = np.log(gap.close[:, DAY] / gap.open[:, DAY]).astype(np.float32) * np.float32(100)
    assert np.array_equal(r.feat[:, DAY, 0], want)
    # a bar inside a session takes the previous close, whatever its open says
    ins = ov.Bars(bars.open.copy(), bars.high, bars.low, bars.close, bars.volume, minute=bars.minute)
    ins.open[:, 5] *= np.float32(1.25)
    assert np.array_equal(ov.featurise_numpy(ins, fp).feat[:, :, 0], ov.featurise_numpy(bars, fp).feat[:, :, 0])
    # the very first bar has no previous close
    first = np.log(bars.close[:, 0] / bars.open[:, 0]).astype(np.float32) * np.float32(100)
    assert np.array_equal(ov.featurise_numpy(bars, fp).feat[:, 0, 0], first)


def test_float64_reference_is_close_to_float32(small):
    bars, fp = small
    a, b = ov.featurise_numpy(bars, fp), ov.featurise_numpy(bars, fp, dtype=np.float64)
    assert a.feat.dtype == np.float32 and b.feat.dtype == np.float64
    assert np.abs(a.feat - b.feat).max() < 1e-4


def test_fit_ignores_later_bars_and_recovers_the_generator(replay):
    bars = replay[0]
    fp = ov.fit_feature_params(bars, upto=800)
    later = ov.Bars(*(np.array(getattr(bars, k)) for k in ov.PLANES), minute=bars.minute)
    later.close[:, 800:] *= 3.0
    later.volume[:, 800:] *= 7.0
    later.open[:, 800:] *= 0.5
    fp2 = ov.fit_feature_params(later, upto=800)
    assert np.array_equal(fp.sigma, fp2.sigma) and np.array_equal(fp.vol_scale, fp2.vol_scale)
    assert fp.day == mb.BarParams.day and fp.alpha == mb.BarParams.alpha and fp.beta == mb.BarParams.beta
    # 800 bars of a series: the sample error of a log-mean of lognormal(0, 0.5) volumes is 0.5 / sqrt(800) = 1.8 %,
    # of a GARCH variance a few times 1 / sqrt(800); the mean over the 32 series is tighter
    assert np.all(np.abs(fp.vol_scale - 1.0) < 0.1) and abs(float(fp.vol_scale.mean()) - 1.0) < 0.03
    assert np.all(np.abs(fp.sigma / mb.BarParams.sigma - 1.0) < 0.3)
    assert abs(float(fp.sigma.mean()) / mb.BarParams.sigma - 1.0) < 0.1
    with pytest.raises(ValueError):
        ov.fit_feature_params(bars, upto=0)


def test_load_bars_npz_round_trip(tmp_path, small):
    bars, _ = small
    named = ov.Bars(*(getattr(bars, k) for k in ov.PLANES), minute=bars.minute, names=[f"s{i}" for i in range(5)])
    p = str(tmp_path / "bars.npz")
    ov.save_bars(p, named)
    got = ov.load_bars(p)
    for k in ov.PLANES:
        assert np.array_equal(getattr(got, k), getattr(bars, k)), k
    assert np.array_equal(got.minutes(DAY), bars.minutes(DAY)) and got.names == named.names
    # without a minute array: t % day
    np.savez(str(tmp_path / "plain.npz"), **{k: getattr(bars, k) for k in ov.PLANES})
    plain = ov.load_bars(str(tmp_path / "plain.npz"), day=DAY)
    assert np.array_equal(plain.minutes(DAY), bars.minutes(DAY)) and plain.names is None
    assert ov.file_crc32c(p) == ov.file_crc32c(p) != ov.file_crc32c(str(tmp_path / "plain.npz"))


def test_load_bars_csv_drops_bad_rows(tmp_path):
    rows = ["2024-03-01 09:30,10,10.5,9.5,10.2,100",
            "2024-03-01 09:31,10.2,10.6,10.1,10.4,150",
            "not a date,1,1,1,1,1",
            "2024-03-01 09:32,10.4,10.4,0,10.3,90",        # a non-positive price
            "2024-03-01 09:33,10.4,x,10.0,10.3,90",        # does not parse
            "2024-03-01 09:34,10.4,10.5,10.0",             # too few fields
            "2024-03-01 09:35,10.4,10.5,10.0,10.1,80",
            "2024-03-04 09:30,11,11.5,10.9,11.2,300",
            "2024-03-04 09:31,11.2,11.3,11.0,11.1,200"]
    p = tmp_path / "ACME.csv"
    p.write_text("\n".join(rows) + "\n")
    b = ov.load_bars(str(p))
    assert b.shape == (1, 5) and b.names == ["ACME"]
    assert b.close[0].tolist() == [np.float32(v) for v in (10.2, 10.4, 10.1, 11.2, 11.1)]
    assert b.volume[0].tolist() == [100.0, 150.0, 80.0, 300.0, 200.0]
    assert np.asarray(b.minute).tolist() == [0, 1, 2, 0, 1]
    fp = ov.fit_feature_params(b)
    assert fp.day == 3
    r = ov.featurise_numpy(b, fp)
    assert np.isfinite(r.feat).all()
    # the second session's first return starts at its own open: the weekend gap is not in it
    assert r.feat[0, 3, 0] == np.log(np.float32(11.2) / np.float32(11.0)).astype(np.float32) * np.float32(100)


def test_window_bank(small):
    bars, fp = small
    r = ov.featurise_numpy(bars, fp)
    close, feat = torch.from_numpy(r.close), torch.from_numpy(r.feat).to(torch.bfloat16)
    c1, f1 = ov.window_bank(close, feat, 12, 20, seed=4)
    c2, f2 = ov.window_bank(close, feat, 12, 20, seed=4)
    c3, _ = ov.window_bank(close, feat, 12, 20, seed=5)
    assert c1.shape == (12, 20) and f1.shape == (12, 20, 8) and c1.is_contiguous() and f1.is_contiguous()
    assert c1.dtype == torch.float32 and f1.dtype == torch.bfloat16
    assert torch.equal(c1, c2) and torch.equal(f1, f2) and not torch.equal(c1, c3)
    start = np.random.default_rng(4).integers(0, T - 20 + 1, size=12)
    for e in range(12):
        s = int(start[e])
        assert torch.equal(c1[e], close[e % 5, s:s + 20]) and torch.equal(f1[e], feat[e % 5, s:s + 20])
    full, _ = ov.window_bank(close, feat, 3, T, seed=0)
    assert torch.equal(full, close[:3])
    with pytest.raises(ValueError, match="bars"):
        ov.window_bank(close, feat, 4, T + 1)


def test_learner_refuses_a_misshapen_bank_before_touching_the_gpu():
    from sharetrade.config import preset_config
    from sharetrade.trainer.recurrent import RecurrentDQN

    with pytest.raises(ValueError, match="GPU"):
        RecurrentDQN(preset_config("recurrent"), torch.device("cpu"), bank=(None, None))


def _cli(capsys, *argv):
    from sharetrade.__main__ import main

    assert main(list(argv)) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_command_line_backtest_on_a_bars_file(capsys, tmp_path):
    bp = mb.BarParams(day=20)
    bars, _ = ov.generate_ohlcv_numpy(3, 100, bp, seed=2)
    p = str(tmp_path / "bars.npz")
    ov.save_bars(p, bars)
    out = _cli(capsys, "backtest", "--policy", "gru", "--bars-file", p, "--ep-len", "20", "--device", "cpu")
    assert out["policy_kind"] == "gru" and out["backend"] == "torch" and out["weights"] == "init"
    assert out["series"] == 3 and out["bars"] == 100 and out["steps"] == 99
    assert out["feature_params"] == "first_session" and out["held_out"] is False and out["first_bar"] == 0
    for k in ("policy", "always_long", "uniform_random", "flat"):
        assert math.isfinite(out[k]["mean"]) and out[k]["n"] == 3
    assert out["flat"]["mean"] == 0.0 and out["always_long"]["long_frac"] == 1.0
    held = _cli(capsys, "backtest", "--policy", "gru", "--bars-file", p, "--held-out", "--ep-len", "10",
                "--device", "cpu")
    assert held["first_bar"] == 80 and held["bars"] == 20 and held["steps"] == 19


def test_command_line_csv_refusal_names_the_bars_file(capsys, tmp_path):
    from sharetrade.__main__ import main

    with pytest.raises(SystemExit) as ei:
        main(["backtest", "--policy", "gru", "--csv", str(tmp_path / "x.csv"), "--device", "cpu"])
    assert ei.value.code == 2 and "--bars-file" in capsys.readouterr().err
    bars, _ = ov.generate_ohlcv_numpy(1, 30, seed=2)
    ov.save_bars(str(tmp_path / "b.npz"), bars)
    with pytest.raises(SystemExit):
        main(["backtest", "--policy", "mlp", "--bars-file", str(tmp_path / "b.npz"), "--device", "cpu"])


def _server(S=8, ep_len=10):
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.serve.gru_serve import GruSessionServer

    pol = GruPolicy(gq.init_params(5), device="cpu", seed=5)
    return GruSessionServer(pol, S, ep_len=ep_len, backend="torch", bar_day=DAY)


def test_step_raw_equals_step_on_the_reference_rows(small):
    bars, fp = small
    N = bars.shape[0]
    whole = ov.featurise_numpy(bars, fp)
    a, b = _server(), _server()
    sa = a.open_raw(N, fp.sigma, fp.vol_scale)
    sb = b.open(N)
    assert sa == sb and all(a.is_raw(s) for s in sa) and not b.is_raw(sb[0])
    M = bars.minutes(DAY)
    X = np.stack([getattr(bars, k) for k in ov.PLANES], axis=2)   # [N, T, 5]
    perm = np.array([3, 0, 4, 1, 2])
    for t in range(T):
        order = perm if t % 2 else np.arange(N)
        sl = [sa[i] for i in order]
        fresh = np.full(N, t == DAY)
        da = a.step_raw(sl, X[order, t], M[order, t], new_episode=fresh)
        db = b.step(sl, whole.feat[order, t], whole.close[order, t], new_episode=fresh)
        assert torch.equal(da.actions, db.actions) and torch.equal(da.position, db.position), t
        assert torch.equal(da.reward.view(torch.int32), db.reward.view(torch.int32)), t
    idx = torch.tensor(sa)
    assert np.array_equal(a.fstate[idx].numpy().view(np.uint32), whole.state.view(np.uint32))
    assert torch.equal(a.table["rec"], b.table["rec"])
    # step on a raw session stays legal
    a.step(sa[:1], whole.feat[:1, 0], whole.close[:1, 0])


def test_step_raw_refusals(small):
    bars, fp = small
    srv = _server()
    plain = srv.open(1)
    raw = srv.open_raw(2, float(fp.sigma[0]), float(fp.vol_scale[0]))
    bar = [[10.0, 10.5, 9.5, 10.2, 100.0]]
    before = srv.batches
    with pytest.raises(ValueError, match="open_raw"):
        srv.step_raw(plain, bar, [0])
    with pytest.raises(ValueError, match="minute"):
        srv.step_raw(raw[:1], bar, [DAY])
    with pytest.raises(ValueError, match="positive"):
        srv.step_raw(raw[:1], [[10.0, 10.5, 0.0, 10.2, 100.0]], [0])
    with pytest.raises(ValueError):
        srv.open_raw(1, 0.0, 1.0)
    assert srv.batches == before
    assert torch.equal(srv.fstate[raw[0]], torch.tensor([0, 0, 0, 0, 0, 0, fp.sigma[0], fp.vol_scale[0]]))
    srv.step_raw(raw, bar * 2, [0, 0])
    srv.close(raw)
    again = srv.open(2)     # the slots come back without raw state
    assert sorted(again) == sorted(raw) and not srv.is_raw(again[0])
    with pytest.raises(ValueError, match="open_raw"):
        srv.step_raw(again, bar * 2, [0, 0])


def test_batcher_and_http_take_raw_bars(small):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from sharetrade.serve.gru_serve import GruBatcher
    from sharetrade.serve.http import make_gru_app

    bars, fp = small
    whole = ov.featurise_numpy(bars, fp)
    ref = _server()
    rs = ref.open(1)
    srv = _server()
    M = bars.minutes(DAY)
    with GruBatcher(srv, max_batch=4, max_delay_us=50.0) as bat:
        c = TestClient(make_gru_app(srv, bat))
        assert c.post("/session", json={"raw": True}).status_code == 400
        sid = c.post("/session", json={"raw": True, "sigma": float(fp.sigma[0]),
                                       "vol_scale": float(fp.vol_scale[0])}).json()
        assert sid == {"session": 0, "raw": True}
        old = c.post("/session").json()
        assert old == {"session": 1}
        for t in range(6):
            body = {k: float(getattr(bars, k)[0, t]) for k in ov.PLANES}
            got = c.post("/session/0/ohlcv", json={**body, "minute": int(M[0, t])}).json()
            want = ref.step(rs, whole.feat[:1, t], whole.close[:1, t])
            assert got["index"] == int(want.actions[0]) and got["position"] == int(want.position[0])
            assert got["reward"] == float(want.reward[0])
        assert c.post("/session/1/ohlcv", json={**body, "minute": 0}).status_code == 409
        assert c.post("/session/0/ohlcv", json={**body, "minute": DAY}).status_code == 409
        assert c.post("/session/7/ohlcv", json={**body, "minute": 0}).status_code == 404
        feats = [float(x) for x in whole.feat[0, 0]]
        assert c.post("/session/1/bar", json={"features": feats, "close": 10.0}).status_code == 200
