"""The risk ledger of the 2x128 backtest on the CPU: ``ledger_from_trace`` against an independent float64 walk
(``qrollout_ledger_refs.walk``) on inputs where every fp32 operation is exact, the walk's deliberate errors,
cut runs, ``report()`` on a hand-computed case, the torch backend of ``PolicyServer.backtest(ledger=True)`` and
the command line."""
import json
import math

import numpy as np
import pytest
import torch

import qrollout_ledger_refs as LR

E, STEPS = 70, 67
H, BUDGET = LR.H, LR.BUDGET
KW = dict(history=H, budget0=BUDGET, shares0=0)


@pytest.fixture(scope="module")
def exact():
    from sharetrade.serve.rollout import ledger_from_trace

    P, A = LR.exact_prices(E, STEPS), LR.random_actions(E, STEPS)
    return {"P": P, "A": A, "led": ledger_from_trace(P, A, **KW), "walk": LR.walk(P, A)}


def test_ledger_from_trace_equals_the_float64_walk_bit_for_bit(exact):
    led, w = exact["led"], exact["walk"]
    LR.same_as_walk(led, w, "exact inputs")
    # every branch of the ledger is reached
    print(f"[meas] refused buys {int(w['refused_buy'].sum())} in {int((w['refused_buy'] > 0).sum())} envs, refused "
          f"sells {int(w['refused_sell'].sum())}, flat days {int(w['flat_days'].sum())}, envs with a drawdown "
          f"{int((w['max_dd'] > 0).sum())}")
    assert int(w["refused_buy"].sum()) > 0 and int(w["refused_sell"].sum()) > 0 and int(w["flat_days"].sum()) > 0
    assert bool((w["max_dd"] > 0).all()) and int(w["dd_days"].max()) > 1 and int(w["max_shares"].max()) >= 3
    assert bool((w["peak"] > w["eq0"]).any()) and bool((w["run"] == 0).any()) and bool((w["run"] > 0).any())
    assert set(exact["A"].flatten().tolist()) == {0, 1, 2}
    assert led.sum_s.dtype == torch.int64 and led.days.dtype == torch.int32 and led.eq0.dtype == torch.float32
    assert bool((led.eq0 == BUDGET).all()) and torch.equal(led.v0, exact["P"][:, H - 1])


@pytest.mark.parametrize("mut", LR.MUTATIONS)
def test_every_mutation_of_the_walk_is_caught(exact, mut):
    """``peak_after_drawdown`` (the peak updated after the day's drawdown is taken) is an equivalent mutant, as it is
    for the GRU ledger (tests/test_gru_ledger.py): on a day that sets a new peak the stale peak gives a negative
    difference, which never raises ``max_dd`` >= 0, where the true order gives 0; on every other day the two peaks
    are equal; and ``eq < peak`` holds for neither on a new-peak day.  The test shows that its output is identical
    and relies on ``drawdown_before_equity`` for the order of the curve."""
    bad = LR.differs_from_walk(exact["led"], LR.walk(exact["P"], exact["A"], mut=mut))
    print(f"[meas] {mut}: differs in {bad}")
    if mut == "peak_after_drawdown":
        assert bad == [], "no longer an equivalent mutant"
        return
    want = {"drawdown_before_equity": "max_dd", "pnl_against_eq0": "sumsq", "position_before_trade": "sum_s",
            "refused_buy_as_executed": "refused_buy", "d_from_first_trade_price": "sum_d", "run_not_reset": "dd_days",
            "pad_rows_live": "curve"}[mut]
    assert want in bad


def test_given_holding_and_start_day(exact):
    """A run from day 5 with a holding of its own (continued episodes, no ledger carried): a fresh ledger whose eq0
    is that holding at the price before day 5."""
    from sharetrade.serve.rollout import ledger_from_trace

    P = LR.exact_prices(E, STEPS, extra=5)
    A = LR.random_actions(E, STEPS, start=5)
    b = torch.full((E,), 90.0) + torch.arange(E, dtype=torch.float32) * 0.25
    s = (torch.arange(E) % 3).to(torch.int32)
    led = ledger_from_trace(P, A, start=5, budget=b, shares=s, **KW)
    LR.same_as_walk(led, LR.walk(P, A, start=5, budget=b.tolist(), shares=s.tolist()), "start 5, given holding")
    assert torch.equal(led.eq0, b + s.float() * P[:, 5 + H - 1])


@pytest.mark.parametrize("cut", [32, 33])
def test_a_cut_run_ends_in_the_whole_runs_record(exact, cut):
    from sharetrade.serve.rollout import ledger_from_trace, simulate_actions

    P, A, whole = exact["P"], exact["A"], exact["led"]
    a = ledger_from_trace(P, A[:, :cut], **KW)
    mid = simulate_actions(P, A[:, :cut], compat=False, **KW)
    b = ledger_from_trace(P, A[:, cut:], start=cut, budget=mid["budget"], shares=mid["shares"], ledger_state=a.state,
                          **KW)
    LR.pieces_reproduce(whole, a, b, f"{cut} + {STEPS - cut}")
    assert a.curve.shape == (cut,) and b.curve.shape == (STEPS - cut,)
    with pytest.raises(ValueError):
        ledger_from_trace(P, A[:, cut:], start=cut, ledger_state=a.state[:, :8], **KW)


def test_report_of_a_hand_computed_case():
    """Two series, four days, history 2, budget 10, no shares.

    Series 0, prices 4 4 | 5 3 3 6, actions Buy Buy Sell Hold: holds 1, 2, 1, 1 shares, budget 5, 2, 5, 5, equity
    10, 8, 8, 11.  Series 1, prices 2 2 | 2 2 2 2, all Hold: equity 10 on every day."""
    from sharetrade.serve.rollout import BacktestResult, ledger_from_trace

    P = torch.tensor([[4.0, 4, 5, 3, 3, 6], [2, 2, 2, 2, 2, 2]])
    A = torch.tensor([[0, 0, 1, 2], [2, 2, 2, 2]], dtype=torch.int8)
    led = ledger_from_trace(P, A, history=2, budget0=10.0, shares0=0)
    assert led.eq_prev.tolist() == [11.0, 10.0] and led.peak.tolist() == [11.0, 10.0]
    assert led.max_dd.tolist() == [2.0, 0.0] and led.dd_days.tolist() == [2, 0] and led.run.tolist() == [0, 0]
    assert led.sumsq.tolist() == [0.0 + 4.0 + 0.0 + 9.0, 0.0]
    assert led.sum_d.tolist() == [1.0 - 1.0 - 1.0 + 2.0, 0.0] and led.sum_d2.tolist() == [7.0, 0.0]
    assert led.sum_sd.tolist() == [1.0 - 2.0 - 1.0 + 2.0, 0.0]
    assert led.sum_s.tolist() == [5, 0] and led.sum_s2.tolist() == [7, 0] and led.max_shares.tolist() == [2, 0]
    assert led.chose_buy.tolist() == [2, 0] and led.chose_sell.tolist() == [1, 0] and led.flat_days.tolist() == [0, 4]
    assert led.refused_buy.tolist() == [0, 0] and led.v_last.tolist() == [6.0, 2.0] and led.days.tolist() == [4, 4]
    assert led.curve.tolist() == [0.0, -2.0, -2.0, 1.0]
    z = torch.zeros(2)
    res = BacktestResult(budget=z, shares=z.int(), final_portfolio=z, buys=z.int(), sells=z.int(), budget0=10.0,
                         start=0, steps=4, ledger=led)
    rep = res.report(days_per_year=4.0)
    s, p = rep["series"], rep["portfolio"]
    assert s["n"] == 2 and s["ret_mean"] == 0.5 and s["ret_median"] == 0.0   # (median: an element of the sample)
    assert s["max_dd_mean"] == 1.0 and s["max_dd_worst"] == 2.0 and s["dd_days_longest"] == 2
    # series 0: mean day change 1/4, variance 13/4 - 1/16 = 51/16; series 1 has zero variance
    sharpe0 = 0.25 / math.sqrt(51.0 / 16.0) * 2.0
    assert s["sharpe_undefined"] == 1 and s["sharpe_mean"] == pytest.approx(sharpe0, rel=1e-15)
    assert s["sharpe_median"] == pytest.approx(sharpe0, rel=1e-15)
    assert s["shares_mean"] == 5 / 8 and s["flat_frac"] == 0.5
    assert (s["buy_frac"], s["sell_frac"], s["hold_frac"]) == (0.25, 0.125, 0.625)
    assert s["refused_buy_frac"] == 0.0 and s["refused_sell_frac"] == 0.0
    # exposure: mean position 5/4 times the price move 6 - 4; timing is the rest of the return 1
    assert s["exposure_mean"] == 1.25 and s["timing_mean"] == -0.75
    # correlation of series 0: cov 0 - 5 * 1 / 4, var_s 7 - 25 / 4, var_d 7 - 1 / 4; series 1 is constant
    assert s["corr_undefined"] == 1
    assert s["corr_median"] == pytest.approx(-1.25 / math.sqrt(0.75 * 6.75), rel=1e-15)
    # the book: curve / 2 = 0, -1, -1, 0.5; daily changes 0, -1, 0, 1.5
    assert p["total"] == 0.5 and p["max_dd"] == 1.0
    assert p["sharpe"] == pytest.approx(0.125 / math.sqrt(3.25 / 4 - 0.125 ** 2) * 2.0, rel=1e-15)
    # all Hold from nothing: every ratio with a zero denominator is None
    none = BacktestResult(budget=z, shares=z.int(), final_portfolio=z, buys=z.int(), sells=z.int(), budget0=10.0,
                          start=0, steps=4, ledger=ledger_from_trace(P[1:], A[1:], history=2, budget0=10.0, shares0=0,
                                                                     curve=False)).report()
    assert none["portfolio"] is None and none["series"]["sharpe_mean"] is None
    assert none["series"]["refused_buy_frac"] is None and none["series"]["corr_median"] is None
    with pytest.raises(ValueError):
        BacktestResult(budget=z, shares=z.int(), final_portfolio=z, buys=z.int(), sells=z.int(), budget0=10.0,
                       start=0, steps=4).report()


def _server(compat=False):
    from sharetrade.config import preset_config
    from sharetrade.serve import PolicyServer

    cfg = preset_config("flagship")
    cfg.env.budget = BUDGET
    cfg.env.compat_decisions = compat
    cfg.agent.epsilon, cfg.agent.seed = 0.0, LR.SEED
    return PolicyServer(cfg, device=torch.device("cpu"), backend="torch")


def test_policy_server_backtest_with_ledger_on_the_torch_backend(exact):
    """Epsilon 0 never exploits: the actions are the uniform draws, and the ledger is the walk's."""
    srv = _server()
    P, n = exact["P"][:17], 40
    res = srv.backtest(P, steps=n, greedy=False, trace=True, ledger=True)
    assert torch.equal(res.actions, LR.random_actions(17, n))
    LR.same_as_walk(res.ledger, LR.walk(P, res.actions), "torch backend")
    assert torch.equal(res.ledger.eq_prev, res.final_portfolio) and torch.equal(res.ledger.eq_prev, res.equity[:, -1])
    assert res.report()["series"]["n"] == 17
    plain = srv.backtest(P, steps=n, greedy=False)
    assert plain.ledger is None and torch.equal(plain.final_portfolio, res.final_portfolio)
    # pieces through the public interface
    a = srv.backtest(P, steps=32, greedy=False, ledger=True)
    b = srv.backtest(P, start=32, steps=n - 32, greedy=False, ledger=True, budget=a.budget, shares=a.shares,
                     ledger_state=a.ledger.state)
    LR.pieces_reproduce(res.ledger, a.ledger, b.ledger, "32 + 8")
    with pytest.raises(ValueError):
        srv.backtest(P, steps=n, ledger_state=a.ledger.state)


def test_compat_decisions_is_refused(exact):
    srv = _server(compat=True)
    with pytest.raises(ValueError, match="compat_decisions"):
        srv.backtest(exact["P"][:2], steps=3, ledger=True)
    assert srv.backtest(exact["P"][:2], steps=3).ledger is None


def _cli(capsys, *argv):
    from sharetrade.__main__ import main

    assert main(list(argv)) == 0
    return capsys.readouterr().out.strip().splitlines()[-1]


def test_command_line_report_and_curve(capsys, tmp_path):
    args = ("backtest", "--preset", "flagship", "--synthetic", "3", "--device", "cpu", "--set", "data.length=230")
    line = _cli(capsys, *args)
    base = json.loads(line)
    assert list(base) == ["series", "days", "steps", "budget", "backend", "weights", "policy", "buy_and_hold",
                          "uniform_random"]
    for k in ("policy", "buy_and_hold", "uniform_random"):
        assert list(base[k]) == ["n", "mean", "std", "median", "steps", "buys", "sells"]
    curve = tmp_path / "curve.npy"
    rep = json.loads(_cli(capsys, *args, "--report", "--curve-out", str(curve)))
    assert list(rep) == list(base)
    for k in ("policy", "buy_and_hold", "uniform_random"):
        assert list(rep[k]) == list(base[k]) + ["report"]
        assert {n: v for n, v in rep[k].items() if n != "report"} == base[k]
        r = rep[k]["report"]
        assert list(r) == ["days_per_year", "series", "portfolio"] and r["series"]["n"] == 3
        assert r["series"]["ret_mean"] == pytest.approx(base[k]["mean"], rel=1e-12)
        assert r["portfolio"]["total"] == pytest.approx(base[k]["mean"], rel=1e-12)
    bh = rep["buy_and_hold"]["report"]["series"]
    assert bh["buy_frac"] == 1.0 and bh["hold_frac"] == 0.0 and bh["refused_sell_frac"] is None
    c = np.load(curve)
    assert c.dtype == np.float64 and c.shape == (base["steps"],)
    assert c[-1] / 3 == pytest.approx(base["policy"]["mean"], rel=1e-12)
    # without the flags the line is what it was: the same bytes, with or without the ledger code in the way
    assert _cli(capsys, *args) == line
