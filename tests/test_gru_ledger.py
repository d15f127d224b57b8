"""The risk ledger's PyTorch form (``sharetrade/serve/gru_rollout.py::ledger_from_trace``, the oracle of the
kernel's ledger instance) on the CPU: against an independent float64 walk on hand-built runs with answers known
in closed form, cut in two, its report's empty cases, and three deliberate errors that the comparisons notice.

The hand-built runs use dyadic bar returns and cost 0.25, so float32 and float64 agree exactly."""
import math

import pytest
import torch

import gru_ledger_refs as LR

COST = 0.25
B, S, H = 0, 1, 2   # Buy, Sell, Hold


def _ledger(actions, ret, *, start, origin, ep_len, position=None, ledger_state=None, cost=COST):
    """simulate_minute_actions (the env mirror) -> ledger_from_trace."""
    from sharetrade.serve.gru_rollout import ledger_from_trace, simulate_minute_actions

    A = torch.tensor(actions, dtype=torch.int8)
    Rt = torch.tensor(ret, dtype=torch.float32)
    out = simulate_minute_actions(torch.ones_like(Rt), A, start=start, ep_len=ep_len, cost=cost, origin=origin,
                                  position=position, ret=Rt)
    led = ledger_from_trace(A, out["reward"], position=position, start=start, origin=origin, ep_len=ep_len,
                            ledger_state=ledger_state)
    return led, out


def _random_case(E, T, seed):
    g = torch.Generator().manual_seed(seed)
    ret = (torch.randint(-32, 33, (E, T), generator=g).float() / 8.0).tolist()
    return ret, g


RUNS = [  # (start, origin, ep_len, steps)
    (0, 0, 5, 20),     # whole episodes
    (5, 2, 4, 14),     # origin < start: the first column is one bar, the run ends inside an episode
    (3, 1, 13, 30),    # partial first and last columns
    (0, 0, 100, 17),   # one partial column
    (7, 7, 1, 6),      # every bar is an episode
]


@pytest.mark.parametrize("start,origin,ep_len,steps", RUNS)
def test_random_runs_equal_the_walk(start, origin, ep_len, steps):
    E, T = 37, start + steps + 1
    ret, g = _random_case(E, T, 5 + steps)
    actions = torch.randint(0, 3, (E, steps), generator=g).tolist()
    led, out = _ledger(actions, ret, start=start, origin=origin, ep_len=ep_len)
    w = LR.walk(actions, ret, COST, start=start, origin=origin, ep_len=ep_len)
    assert torch.equal(out["reward"].double(), torch.tensor(w["reward"], dtype=torch.float64))
    LR.check_against_walk(led, w)
    assert led.ep_ret.shape == (E, len(w["full"])) and int(led.trips.sum()) > 0


def test_known_peak_trough_and_drawdown_length():
    """Buy and hold over returns 1, 2, -1, -2, -0.5, 1, 3, -1: equity 0.75, 2.75, 1.75, -0.25, -0.75, 0.25, 3.25,
    2.25.  The peak 2.75 stands for 4 bars (2 .. 5), the trough -0.75 is 3.5 under it; the last bar is 1 under
    the new peak 3.25."""
    ret = [[1.0, 2.0, -1.0, -2.0, -0.5, 1.0, 3.0, -1.0, 0.0]]
    actions = [[B] + [H] * 7]
    led, _ = _ledger(actions, ret, start=0, origin=0, ep_len=100)
    assert led.max_dd.tolist() == [3.5] and led.dd_bars.tolist() == [4]
    assert led.state_field("peak").tolist() == [3.25] and led.state_field("cum").tolist() == [2.25]
    assert led.state_field("run").tolist() == [1]
    assert led.sumsq.tolist() == [0.75 ** 2 + 4 + 1 + 4 + 0.25 + 1 + 9 + 1]
    assert led.trips.tolist() == [0] and led.state_field("trip").tolist() == [2.25]   # the long is still open
    assert led.ep_ret.tolist() == [[2.25]] and led.ep_trades.tolist() == [[1]] and led.full == [False]
    LR.check_against_walk(led, LR.walk(actions, ret, COST, start=0, origin=0, ep_len=100))


def test_long_across_an_episode_end_closes_at_no_cost():
    """Episodes of 4 bars.  Env 0 buys at bar 1 and holds: the trip closes at bar 3 with 2 + 1 - 3 minus one cost
    (none at the forced flat); it is flat again at bar 4 and Hold keeps it flat.  Env 1 buys on the episode's last
    bar: a one-bar trip."""
    ret = [[9.0, 2.0, 1.0, -3.0, 5.0, 5.0, 5.0, 5.0, 0.0],
           [9.0, 9.0, 9.0, 0.5, 1.0, 1.0, 1.0, 1.0, 0.0]]
    actions = [[H, B, H, H, H, H, H, H],
               [H, H, H, B, H, H, B, S]]
    led, out = _ledger(actions, ret, start=0, origin=0, ep_len=4)
    assert led.trips.tolist() == [1, 2] and led.wins.tolist() == [0, 2]
    assert led.loss_sum.tolist() == [-0.25, 0.0] and led.win_sum.tolist() == [0.0, 0.25 + (0.75 - 0.25)]
    assert out["reward"][0].tolist() == [0.0, 1.75, 1.0, -3.0, 0.0, 0.0, 0.0, 0.0]
    assert led.ep_ret.tolist() == [[-0.25, 0.0], [0.25, 0.5]] and led.ep_trades.tolist() == [[1, 0], [1, 2]]
    assert led.full == [True, True] and led.curve.tolist() == [0.0, 1.75, 1.0, -2.75, 0.0, 0.0, 0.75, -0.25]
    LR.check_against_walk(led, LR.walk(actions, ret, COST, start=0, origin=0, ep_len=4))


def test_partial_first_column_and_run_ending_mid_episode():
    """origin 2, start 5, episodes of 4: bar 5 ends the episode 2 .. 5 (column 0, one bar), columns 1 and 2 are
    whole (6 .. 9, 10 .. 13), column 3 holds bars 14 .. 15 of an episode that goes on."""
    from sharetrade.serve.gru_rollout import episode_columns

    assert episode_columns(5, 11, 2, 4) == (2, 4, [False, True, True, False])
    ret = [[0.0] * 5 + [1.0, 0.5, 0.5, 0.5, 0.5, 2.0, 2.0, 2.0, 2.0, -1.0, -1.0, 0.0]]
    actions = [[B] * 11]
    pos = torch.tensor([1], dtype=torch.int32)     # long before bar 5: no trade, no cost on it
    led, _ = _ledger(actions, ret, start=5, origin=2, ep_len=4, position=pos)
    assert led.ep_ret.tolist() == [[1.0, 1.75, 7.75, -2.25]] and led.ep_trades.tolist() == [[0, 1, 1, 1]]
    assert led.state_field("ep").tolist() == [-2.25] and led.state_field("ep_tr").tolist() == [1]
    assert led.trips.tolist() == [3] and led.state_field("trip").tolist() == [-2.25]
    LR.check_against_walk(led, LR.walk(actions, ret, COST, start=5, origin=2, ep_len=4, position=[1]))


@pytest.mark.parametrize("cut", [20, 24, 5])
def test_two_pieces_reproduce_the_whole(cut):
    """37 series, bars 3 .. 63 of generated minute bars (real float32 rounding), random actions, episodes of 13
    from bar 1; cut after 20 bars (inside an episode), after 24 (on an episode's last bar, 26) and after 5 (inside the
    partial first column)."""
    import gru_backtest_refs as R
    from sharetrade.serve.gru_rollout import episode_columns, ledger_from_trace, simulate_minute_actions

    E, start, origin, ep_len, steps = 37, 3, 1, 13, 61
    close, _ = R.bars(E, 70)
    acts = R.random_actions(E, steps)
    kw = dict(ep_len=ep_len, cost=0.01, origin=origin)
    ow = simulate_minute_actions(close, acts, start=start, **kw)
    whole = ledger_from_trace(acts, ow["reward"], start=start, origin=origin, ep_len=ep_len)
    oa = simulate_minute_actions(close, acts[:, :cut], start=start, **kw)
    a = ledger_from_trace(acts[:, :cut], oa["reward"], start=start, origin=origin, ep_len=ep_len)
    ob = simulate_minute_actions(close, acts[:, cut:], start=start + cut, position=oa["position"],
                                 entry=oa["entry"], **kw)
    b = ledger_from_trace(acts[:, cut:], ob["reward"], position=oa["position"], start=start + cut, origin=origin,
                          ep_len=ep_len, ledger_state=a.state)
    assert torch.equal(torch.cat([oa["reward"], ob["reward"]], 1), ow["reward"])
    n_a = episode_columns(start, cut, origin, ep_len)[1]
    mid = (start + cut - origin) % ep_len != 0
    LR.pieces_reproduce(whole, a, b, n_a - (1 if mid else 0), label=f"cut {cut}")
    assert mid == (cut != 24) and int(whole.trips.sum()) > 0 and float(whole.max_dd.max()) > 0
    # cum is the float32 sum of the rewards in bar order
    s = torch.zeros(E)
    for i in range(steps):
        s = s + ow["reward"][:, i]
    assert torch.equal(s, whole.state_field("cum")) and torch.equal(s, ow["ret"])


def test_curve_is_within_the_fp32_summation_bound():
    """The butterfly and the chunk sum are an fp32 summation of E terms: |curve - exact| <= (E - 1) 2^-24 sum|r|."""
    import gru_backtest_refs as R
    from sharetrade.serve.gru_rollout import ledger_from_trace, simulate_minute_actions

    E, steps = 100, 30
    close, _ = R.bars(E, 40)
    acts = R.random_actions(E, steps)
    out = simulate_minute_actions(close, acts, ep_len=7)
    led = ledger_from_trace(acts, out["reward"], start=0, origin=0, ep_len=7)
    exact = out["reward"].double().sum(0)
    bound = (E - 1) * 2.0 ** -24 * out["reward"].double().abs().sum(0)
    assert bool(((led.curve.double() - exact).abs() <= bound).all())


def test_report_none_cases_and_values():
    from sharetrade.serve.gru_rollout import result_from

    # flat: no trips, no variance, and a run without a whole episode
    ret = [[1.0] * 9]
    led, out = _ledger([[S] * 6], ret, start=1, origin=0, ep_len=8)
    rep = result_from(out, 1, 6, 8, 0, "torch", False, led).report()
    s = rep["series"]
    assert s["hit_rate"] is None and s["profit_factor"] is None and s["trip_mean"] is None
    assert s["sharpe_mean"] is None and s["sharpe_median"] is None and s["trips"] == 0
    assert rep["episodes"] == {"n": 0, "mean": None, "std": None, "worst": None, "positive": None}
    assert rep["portfolio"]["sharpe"] is None and rep["portfolio"]["total"] == 0.0
    assert rep["bars_per_year"] == 252 * 8
    # only winning trips: the profit factor has no denominator
    led, out = _ledger([[B, S, B, S]], [[1.0, 0.0, 2.0, 0.0, 0.0]], start=0, origin=0, ep_len=2)
    rep = result_from(out, 0, 4, 2, 0, "torch", False, led).report(bars_per_year=4.0)
    s = rep["series"]
    assert s["hit_rate"] == 1.0 and s["profit_factor"] is None and s["trips"] == 2
    # rewards 0.75, -0.25, 1.75, -0.25: trips 0.5 and 1.5, episodes 0.5 and 1.5
    assert s["trip_mean"] == 1.0 and rep["episodes"]["mean"] == 1.0 and rep["episodes"]["std"] == 0.5
    assert rep["episodes"]["worst"] == 0.5 and rep["episodes"]["positive"] == 1.0 and rep["episodes"]["n"] == 2
    m, var = 2.0 / 4, (0.75 ** 2 + 0.25 ** 2 + 1.75 ** 2 + 0.25 ** 2) / 4 - 0.25
    assert s["sharpe_mean"] == pytest.approx(m / math.sqrt(var) * 2.0, rel=1e-12)
    p = rep["portfolio"]
    assert p["total"] == 2.0 and p["max_dd"] == 0.25 and p["episodes"] == [0.5, 1.5] and p["full"] == [True, True]
    assert p["sharpe"] == pytest.approx(s["sharpe_mean"], rel=1e-12)
    assert s["max_dd_worst"] == 0.25 and s["dd_bars_longest"] == 1 and s["ret_mean"] == 2.0
    # without a ledger there is nothing to report
    with pytest.raises(ValueError, match="ledger=True"):
        result_from(out, 0, 4, 2, 0, "torch", False).report()


def test_torch_backend_ledger_and_keyword_checks():
    import gru_backtest_refs as R
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import GruPolicy, ledger_from_trace

    close, feat = R.bars(5, 20)
    pol = GruPolicy(gq.init_params(3), device=torch.device("cpu"), seed=3)
    kw = dict(steps=12, ep_len=5, greedy=False, epsilon=0.5, backend="torch")
    plain = pol.backtest(close, feat, **kw)
    res = pol.backtest(close, feat, trace=True, ledger=True, **kw)
    assert plain.ledger is None and res.ledger is not None and res.ledger.curve.shape == (12,)
    want = ledger_from_trace(res.actions, res.reward, start=0, origin=0, ep_len=5)
    LR.same_ledger(res.ledger, want)
    assert torch.equal(res.ret, plain.ret) and torch.equal(res.ledger.state_field("cum"), res.ret)
    assert res.ledger.ep_ret.shape == (5, 3) and res.ledger.full == [True, True, False]
    with pytest.raises(ValueError, match="ledger=True"):
        pol.backtest(close, feat, ledger_state=res.ledger.state, **kw)


@pytest.mark.parametrize("mut", LR.MUTATIONS)
def test_mutations_are_caught(mut):
    """A ledger that takes the drawdown before the bar's reward is added, charges the cost at the forced flat, or
    lets the padding rows of the last chunk into the butterfly differs from the oracle on the hand-built runs:
    the comparison that passes against the true walk fails against the mutated one.

    ``peak_after_dd`` (the peak updated after the drawdown is taken) is an equivalent mutant: on a bar that sets a
    new peak the stale peak gives a negative difference, which never raises ``max_dd`` >= 0, where the true order
    gives 0; on every other bar the two peaks are equal; and ``cum < peak`` holds for neither on a new-peak bar.
    The test shows that its output is identical and relies on ``dd_before_cum`` for the order of the curve."""
    caught = 0
    for start, origin, ep_len, steps in RUNS:
        E, T = 37, start + steps + 1
        ret, g = _random_case(E, T, 5 + steps)
        actions = torch.randint(0, 3, (E, steps), generator=g).tolist()
        led, _ = _ledger(actions, ret, start=start, origin=origin, ep_len=ep_len)
        LR.check_against_walk(led, LR.walk(actions, ret, COST, start=start, origin=origin, ep_len=ep_len))
        try:
            LR.check_against_walk(led, LR.walk(actions, ret, COST, start=start, origin=origin, ep_len=ep_len, mut=mut))
        except AssertionError as exc:
            caught += 1
            print(f"[mutation] {mut}, run {(start, origin, ep_len, steps)}: first differing field {exc.args[0][0]}")
    if mut == "peak_after_dd":
        assert caught == 0, "no longer an equivalent mutant"
        print("[mutation] peak_after_dd: an equivalent mutant, every field identical on every run")
    else:
        assert caught >= 3, (mut, caught)
