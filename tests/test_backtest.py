"""Backtesting on the CPU: the rollout oracle (``sharetrade.serve.rollout.reference_rollout``) against a
day-by-day loop of the serving oracle and the env transition, chained half-episodes, the compat env, the torch
backend of ``PolicyServer.backtest``, the ``backtest`` command, and the launch struct's ctypes mirror."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sharetrade.serve.rollout import RolloutParams, reference_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSFT = os.path.join(ROOT, "tests", "golden", "MSFT-stock-prices-revised.txt")
H, BUDGET, SEED = 201, 120.0, 3


def _prices(E, steps):
    g = np.random.default_rng(3)
    return torch.from_numpy((50.0 * np.exp(np.cumsum(g.normal(0, 0.02, size=(E, H + steps)), axis=1))).astype(np.float32))


@pytest.fixture(scope="module")
def net():
    from sharetrade.config import preset_config
    from sharetrade.models import qnet as qn

    cfg = preset_config("flagship")
    layout = qn.QNetLayout.from_config(cfg.model)
    return layout, qn.init_params(layout, cfg.model, seed=SEED, host_mirror=True)


def _roll(net, P, *, epsilon=math.inf, compat=False, **kw):
    layout, params = net
    return reference_rollout(params, layout, P, history=H, feat_mode="relative", output_relu=False, budget0=BUDGET,
                             shares0=0, compat=compat, epsilon=epsilon, ramp=4.0, key_seed=SEED, **kw)


@pytest.mark.parametrize("epsilon", [math.inf, 0.9])
def test_reference_rollout_is_the_day_by_day_loop(net, epsilon):
    from sharetrade.env import trading as tr
    from sharetrade.serve import reference_select
    from sharetrade.utils import rng

    layout, params = net
    E, steps, off = 12, 30, 7
    P = _prices(E, steps)
    out = _roll(net, P, epsilon=epsilon, env_offset=off)
    b = torch.full((E,), BUDGET)
    s = torch.zeros(E, dtype=torch.int32)
    buys, sells = torch.zeros(E, dtype=torch.int32), torch.zeros(E, dtype=torch.int32)
    for t in range(steps):
        rows = torch.cat([P[:, t:t + H], b[:, None], s[:, None].float()], 1)
        a, q = reference_select(params, layout, rows, history=H, feat_mode="relative", output_relu=False,
                                budget0=BUDGET, epsilon=0.9, ramp=4.0, key_seed=SEED)
        a = a.long()
        if not math.isinf(epsilon):
            u1, u2 = rng.uniforms(SEED, 0, np.arange(off, off + E, dtype=np.uint32), t, stream=4)
            ex = torch.from_numpy(u1 < np.minimum(np.float32(0.9), np.float32(t) * np.float32(0.25)))
            a = torch.where(ex, a, torch.from_numpy(np.minimum((u2 * np.float32(3)).astype(np.int64), 2)))
        v = P[:, t + H]
        b2, s2, _ = tr.env_transition(a, b, s, v, v, False, BUDGET, 0)
        buys += (s2 > s).int()
        sells += (s2 < s).int()
        b, s = b2, s2
        assert torch.equal(out["actions"][:, t].long(), a), t
        assert torch.equal(out["q"][:, t], q), t
        assert torch.equal(out["equity"][:, t], b + s.float() * v), t
    assert torch.equal(out["budget"], b) and torch.equal(out["shares"], s)
    assert torch.equal(out["portfolio"], b + s.float() * P[:, -1])
    assert torch.equal(out["buys"], buys) and torch.equal(out["sells"], sells)
    assert int(buys.sum()) > 0 and int(sells.sum()) > 0
    if not math.isinf(epsilon):   # day 0 explores everywhere (ramp 0): the draws decide
        assert not torch.equal(out["actions"], _roll(net, P)["actions"])


@pytest.mark.parametrize("epsilon", [math.inf, 0.9])
def test_two_half_episodes_equal_one(net, epsilon):
    P = _prices(9, 40)
    whole = _roll(net, P, epsilon=epsilon)
    a = _roll(net, P, epsilon=epsilon, start=0, steps=17)
    b = _roll(net, P, epsilon=epsilon, start=17, steps=23, budget=a["budget"], shares=a["shares"])
    for k in ("budget", "shares", "portfolio"):
        assert torch.equal(b[k], whole[k]), k
    for k in ("buys", "sells"):
        assert torch.equal(a[k] + b[k], whole[k]), k
    for k in ("actions", "q", "equity"):
        assert torch.equal(torch.cat([a[k], b[k]], dim=1), whole[k]), k


def test_compat_env_never_accumulates(net):
    P = _prices(16, 40)
    forced = torch.zeros(16, 40, dtype=torch.int8)   # Buy every day
    out = _roll(net, P, compat=True, forced_actions=forced)
    # every day trades from (b0, 0): the state after the last day is one Buy from the start state, or the start
    covered = P[:, -1] <= BUDGET
    assert torch.equal(out["shares"], covered.int())
    assert torch.equal(out["budget"], torch.where(covered, BUDGET - P[:, -1], torch.full((16,), BUDGET)))
    assert torch.equal(out["buys"], (P[:, H:] <= BUDGET).sum(1).int()) and int(out["sells"].sum()) == 0
    free = _roll(net, P, compat=False, forced_actions=forced)
    assert int(free["shares"].max()) >= 2                                   # the intended env does accumulate
    with pytest.raises(ValueError):
        _roll(net, P, start=1, steps=40)


def test_policy_server_torch_backtest_on_msft():
    from sharetrade.data import prices as dp
    from sharetrade.serve import BacktestResult, PolicyServer

    _, series = dp.sorted_series(dp.load_csv(MSFT))
    srv = PolicyServer(device=torch.device("cpu"), backend="torch")
    res = srv.backtest(series[: srv.H + 50], trace=True)
    assert isinstance(res, BacktestResult) and res.steps == 50
    assert res.final_portfolio.shape == (1,) and res.actions.shape == (1, 50) and res.q.shape == (1, 50, 3)
    assert float(res.equity[0, -1]) == float(res.final_portfolio[0])
    sm = res.summary()
    assert sm["n"] == 1 and sm["steps"] == 50 and sm["std"] == 0.0 and sm["mean"] == sm["median"]
    assert all(math.isfinite(float(v)) for v in sm.values())
    assert sm["buys"] == int(res.buys.sum()) and sm["sells"] == int(res.sells.sum())
    # a second piece from the first one's end state: the server-level chaining
    head = srv.backtest(series[: srv.H + 50], steps=20)
    tail = srv.backtest(series[: srv.H + 50], start=20, budget=head.budget, shares=head.shares)
    assert torch.equal(tail.final_portfolio, res.final_portfolio)
    assert srv.backtest(series[: srv.H + 50]).actions is None
    with pytest.raises(ValueError):
        srv.backtest(series[: srv.H])


def test_summary_statistics():
    from sharetrade.serve import BacktestResult

    fin = torch.tensor([100.0, 130.0, 90.0, 180.0])
    z = torch.zeros(4, dtype=torch.int32)
    sm = BacktestResult(budget=fin, shares=z, final_portfolio=fin, buys=z + 2, sells=z + 1, budget0=100.0, start=0,
                        steps=5).summary()
    d = np.array([0.0, 30.0, -10.0, 80.0])
    assert sm["mean"] == d.mean() and abs(sm["std"] - d.std()) < 1e-9 and sm["median"] == 0.0   # (lower median)
    assert sm["buys"] == 8 and sm["sells"] == 4 and sm["n"] == 4


def test_backtest_command_prints_json(tmp_path):
    with open(MSFT) as f:
        lines = f.readlines()
    csv = tmp_path / "msft_head.csv"
    csv.write_text("".join(lines[:260]))
    r = subprocess.run([sys.executable, "-m", "sharetrade", "backtest", "--device", "cpu", "--csv", str(csv),
                        "--trace-out", str(tmp_path / "tr")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["series"] == 1 and out["steps"] == out["days"] - H and out["backend"] == "torch"
    for k in ("policy", "buy_and_hold", "uniform_random"):
        assert math.isfinite(out[k]["mean"]) and out[k]["n"] == 1
    assert np.load(tmp_path / "tr" / "actions.npy").shape == (1, out["steps"])
    assert np.load(tmp_path / "tr" / "equity.npy").shape == (1, out["steps"])


def test_rollout_params_mirror_matches_the_struct():
    import build

    build.build_all()
    from sharetrade.ops import native

    fn = native.lib().st_abi_qrollout
    fn.argtypes, fn.restype = [C.POINTER(C.c_int), C.c_int], C.c_int
    out = (C.c_int * 1)()
    assert fn(out, 1) == 1
    assert out[0] == C.sizeof(RolloutParams)
