"""The ledger instance of the episode rollout kernel (``csrc/qrollout.hip``: ``st_qrollout_ledger_launch``) against
``ledger_from_trace`` of its own action trace, the float64 walk of ``qrollout_ledger_refs``, the plain instance,
itself on one workgroup and itself cut in two.

The ledger depends on the net only through the actions and every comparison is made on the kernel's own action
trace, so all of them are bit for bit and no case is left out.  On ``exact_prices`` (a walk on quarters, budget 120)
every fp32 operation of the ledger is exact and the independent float64 walk must agree too; on the lognormal prices
of tests/test_gpu_backtest.py the comparison is the one against ``ledger_from_trace``.
"""
import ctypes as C

import pytest
import torch

import qrollout_ledger_refs as LR
from guard_band import Band

pytestmark = pytest.mark.gpu

H, BUDGET, SEED = LR.H, LR.BUDGET, LR.SEED
KW = dict(history=H, budget0=BUDGET, shares0=0)
PLAIN = ("budget", "shares", "portfolio", "buys", "sells")
TRACES = ("actions", "q", "equity")


def _cfg(features="relative", compat=False):
    from sharetrade.config import preset_config

    cfg = preset_config("flagship")
    cfg.env.features = features
    cfg.env.budget = BUDGET
    cfg.env.compat_decisions = compat
    cfg.agent.epsilon, cfg.agent.ramp = 0.0, 4.0   # epsilon 0 never exploits: greedy=False is uniform random
    if features == "raw":
        cfg.model.init_std = 0.01
        cfg.model.init = "normal"
    return cfg


class _Policy:
    """Weights of seed 3 (NumPy mirror: the same on every machine) behind a RolloutKernel."""

    def __init__(self, cfg):
        from sharetrade.env import trading as tr
        from sharetrade.models import qnet as qn
        from sharetrade.serve.rollout import RolloutKernel
        from sharetrade.utils import rng

        layout = qn.QNetLayout.from_config(cfg.model)
        self.dev = qn.init_params(layout, cfg.model, seed=SEED, host_mirror=True).cuda()
        self.dev_bf = self.dev.to(torch.bfloat16)
        self.kern = RolloutKernel(layout, self.dev, self.dev_bf, history=H, feat_mode=tr.FEATURES[cfg.env.features],
                                  output_relu=cfg.model.output_relu, budget0=cfg.env.budget, shares0=cfg.env.shares,
                                  compat=cfg.env.compat_decisions, epsilon=cfg.agent.epsilon, ramp=cfg.agent.ramp,
                                  key=rng.key_for(SEED, 0))

    def run(self, P, **kw):
        out = self.kern.run(P if P.is_cuda else P.cuda(), **kw)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}


def _ledger(out):
    from sharetrade.serve.rollout import QLedger

    return QLedger(state=out["ledger_state"], curve=out.get("curve"))


def _check(pol, P, steps, *, exact, label, start=0, budget=None, shares=None, **kw):
    """One traced ledger launch against the oracle on its own actions (and the walk on exact inputs)."""
    from sharetrade.serve.rollout import ledger_from_trace

    dev = {} if budget is None else {"budget": budget.cuda(), "shares": shares.cuda()}
    out = pol.run(P, start=start, steps=steps, trace=True, ledger=True, **dev, **kw)
    led = _ledger(out)
    E = P.shape[0]
    assert led.state.shape == (E, 24) and led.curve.shape == (steps,) and led.curve.dtype == torch.float64
    want = ledger_from_trace(P, out["actions"], start=start, budget=budget, shares=shares, **KW)
    LR.same_ledger(led, want, label)
    if exact:
        w = LR.walk(P, out["actions"], start=start, budget=None if budget is None else budget.tolist(),
                    shares=None if shares is None else shares.tolist())
        LR.same_as_walk(led, w, label)
    # the record agrees with the launch's plain outputs and its equity trace
    assert torch.equal(LR.bits(led.eq_prev), LR.bits(out["portfolio"])), label
    assert torch.equal(LR.bits(led.eq_prev), LR.bits(out["equity"][:, -1])), label
    assert torch.equal(led.days, torch.full((E,), steps, dtype=torch.int32)), label
    return out, led


@pytest.fixture(scope="module")
def pol(native_built):
    return _Policy(_cfg())


@pytest.mark.parametrize("E", [1, 15, 16, 17, 33, 70])
def test_uniform_random_on_exact_inputs(pol, E):
    """Lone rows, a half chunk, chunk and tile edges and three tiles, each over every path of the 32-day block
    loop; uniform random actions reach every branch of the ledger (refused trades, flat days, drawdowns)."""
    for steps in (1, 31, 32, 33, 67):
        start = 5 if steps in (31, 33) else 0
        P = LR.exact_prices(E, steps, extra=start)
        out, led = _check(pol, P, steps, exact=True, start=start, greedy=False, label=f"E {E} steps {steps}")
        assert torch.equal(out["actions"], LR.random_actions(E, steps, start=start)), (E, steps)
    if E == 70:
        assert int(led.refused_buy.sum()) > 0 and int(led.refused_sell.sum()) > 0 and int(led.flat_days.sum()) > 0
        assert bool((led.max_dd > 0).all()) and int(led.dd_days.max()) > 1


@pytest.mark.parametrize("features", ["relative", "raw"])
@pytest.mark.parametrize("greedy", [True, False])
def test_feature_modes_greedy_and_random(native_built, pol, features, greedy):
    p = pol if features == "relative" else _Policy(_cfg(features))
    _check(p, LR.exact_prices(33, 67), 67, exact=True, greedy=greedy, label=f"exact {features} greedy {greedy}")
    _check(p, LR.lognormal_prices(48, 40, extra=5), 40, exact=False, start=5, greedy=greedy,
           label=f"lognormal {features} greedy {greedy}")


def test_lognormal_prices_three_tiles(pol):
    out, led = _check(pol, LR.lognormal_prices(70, 67), 67, exact=False, greedy=False, label="lognormal 70 x 67")
    assert float(led.max_dd.max()) > 0 and int(led.max_shares.max()) >= 2


def test_given_budget_and_shares(pol):
    E, steps, start = 33, 40, 5
    b = torch.full((E,), 90.0) + torch.arange(E, dtype=torch.float32) * 0.25
    s = (torch.arange(E) % 3).to(torch.int32)
    P = LR.exact_prices(E, steps, extra=start)
    _, led = _check(pol, P, steps, exact=True, start=start, budget=b, shares=s, greedy=False, label="given holding")
    assert torch.equal(led.eq0, b + s.float() * P[:, start + H - 1])


def test_one_workgroup_walks_every_tile(pol):
    P = LR.exact_prices(70, 67)
    base, led = _check(pol, P, 67, exact=True, greedy=False, label="one workgroup per tile")
    for grid in (1, 2):
        out, g = _check(pol, P, 67, exact=True, greedy=False, grid=grid, label=f"grid {grid}")
        LR.same_ledger(g, led, f"grid {grid} vs one workgroup per tile")
        for k in PLAIN + TRACES:
            assert torch.equal(LR.bits(out[k]), LR.bits(base[k])), (grid, k)


@pytest.mark.parametrize("greedy", [True, False])
def test_plain_outputs_and_traces_equal_the_plain_launch(pol, greedy):
    P = LR.lognormal_prices(70, 67).cuda()
    plain = pol.run(P, steps=67, greedy=greedy, trace=True)
    traced = pol.run(P, steps=67, greedy=greedy, trace=True, ledger=True)
    quiet = pol.run(P, steps=67, greedy=greedy, ledger=True)
    nocurve = pol.run(P, steps=67, greedy=greedy, ledger=True, curve=False)
    assert "ledger_state" not in plain and "actions" not in quiet and "curve" not in nocurve
    for k in PLAIN + TRACES:
        assert torch.equal(LR.bits(traced[k]), LR.bits(plain[k])), k
    for k in PLAIN:
        assert torch.equal(LR.bits(quiet[k]), LR.bits(plain[k])), k
    LR.same_ledger(_ledger(quiet), _ledger(traced), "with and without the trace")
    assert torch.equal(nocurve["ledger_state"], traced["ledger_state"])


@pytest.mark.parametrize("cut", [32, 33])
def test_pieces_reproduce_the_whole(pol, cut):
    P = LR.lognormal_prices(70, 67).cuda()
    whole = pol.run(P, steps=67, greedy=False, ledger=True)
    a = pol.kern.run(P, steps=cut, greedy=False, ledger=True)
    b = pol.kern.run(P, start=cut, steps=67 - cut, greedy=False, ledger=True, budget=a["budget"], shares=a["shares"],
                     ledger_state=a["ledger_state"])
    torch.cuda.synchronize()
    LR.pieces_reproduce(_ledger(whole), _ledger(a), _ledger(b), f"{cut} + {67 - cut}")
    for k in ("budget", "shares", "portfolio"):
        assert torch.equal(LR.bits(b[k].cpu()), LR.bits(whole[k])), k


def test_policy_server_backtest_with_ledger(native_built):
    from sharetrade.serve import PolicyServer

    srv = PolicyServer(_cfg(), device=torch.device("cuda", 0), backend="native", seed=SEED)
    P = LR.exact_prices(17, 40)
    res = srv.backtest(P, greedy=False, trace=True, ledger=True)
    torch.cuda.synchronize()
    LR.same_as_walk(res.ledger, LR.walk(P, res.actions.cpu()), "PolicyServer.backtest")
    assert res.report()["series"]["n"] == 17 and res.report()["portfolio"] is not None
    with pytest.raises(ValueError, match="compat_decisions"):
        PolicyServer(_cfg(compat=True), device=torch.device("cuda", 0), backend="native").backtest(P, ledger=True)
    with pytest.raises(ValueError, match="compat_decisions"):
        _Policy(_cfg(compat=True)).kern.run(P.cuda(), ledger=True)


E_G, STEPS_G, STRIDE_G = 17, 33, 64   # guard-band shape: a tile with 15 dead rows, a chunk with one live row


def _banded_args(pol, P):
    """A RolloutLedger whose every output lies in a guard band: the kernel's parameter block as a ledger run of
    the same shape left it, with the output pointers replaced."""
    from sharetrade.serve.rollout import RolloutLedger

    pol.kern.run(P, steps=STEPS_G, greedy=False, trace=True, ledger=True)
    torch.cuda.synchronize()
    i32, f32 = torch.int32, torch.float32
    n = E_G * STEPS_G
    bands = {"out_budget": Band(E_G, f32, -7.0), "out_shares": Band(E_G, i32, -7),
             "out_portfolio": Band(E_G, f32, -7.0), "out_buys": Band(E_G, i32, -7), "out_sells": Band(E_G, i32, -7), "tr_actions": Band(n, torch.int8, -7),
             "tr_q": Band(3 * n, f32, -7.0), "tr_equity": Band(n, f32, -7.0),
             "state_out": Band(E_G * 24, i32, -7), "part": Band(2 * STRIDE_G, f32, -7.0),
             "curve": Band(STEPS_G, torch.float64, -7.0)}
    q = RolloutLedger()
    q.r = pol.kern.p
    for k, b in bands.items():
        setattr(q.l if hasattr(q.l, k) else q.r, k, b.ptr())
    q.l.state_in, q.l.part_stride = None, STRIDE_G
    return q, bands


def test_every_output_stays_inside_its_buffer(pol):
    from sharetrade.ops import native
    from sharetrade.serve.rollout import _lib

    P = LR.exact_prices(E_G, STEPS_G).cuda()
    want = pol.run(P, steps=STEPS_G, greedy=False, trace=True, ledger=True)
    q, bands = _banded_args(pol, P)
    assert _lib().st_qrollout_ledger_launch(C.byref(q), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    for k, b in bands.items():
        assert b.guards_intact(), k
    for k, name in (("out_budget", "budget"), ("out_shares", "shares"), ("out_portfolio", "portfolio"),
                    ("out_buys", "buys"), ("out_sells", "sells"), ("tr_actions", "actions"), ("tr_q", "q"),
                    ("tr_equity", "equity"), ("state_out", "ledger_state"), ("curve", "curve")):
        assert torch.equal(LR.bits(bands[k].cpu()), LR.bits(want[name].reshape(-1))), k
    part = bands["part"].cpu().view(2, STRIDE_G)
    assert bool((part[:, STEPS_G:] == -7.0).all()) and not bool((part[:, :STEPS_G] == -7.0).any())
    assert torch.equal(part[:, :STEPS_G].double().sum(0), want["curve"])


def test_launcher_refuses_bad_ledger_arguments(pol):
    """Return codes only: hipErrorInvalidValue before anything is launched."""
    from sharetrade.ops import native
    from sharetrade.serve.rollout import _lib

    q, bands = _banded_args(pol, LR.exact_prices(E_G, STEPS_G).cuda())
    snaps = {k: b.snap() for k, b in bands.items()}
    INVALID = 1
    for where, over in (("l", dict(curve=None)), ("l", dict(part=None)), ("l", dict(part_stride=STEPS_G)),
                        ("l", dict(part_stride=STRIDE_G + 32)), ("l", dict(state_out=None)),
                        ("r", dict(compat_env=1)), ("r", dict(steps=0)), ("r", dict(out_budget=None))):
        old = {k: getattr(getattr(q, where), k) for k in over}
        for k, v in over.items():
            setattr(getattr(q, where), k, v)
        assert _lib().st_qrollout_ledger_launch(C.byref(q), 0, native.stream_handle()) == INVALID, over
        for k, v in old.items():
            setattr(getattr(q, where), k, v)
    torch.cuda.synchronize()
    for k, b in bands.items():
        assert b.same(snaps[k]), k   # nothing ran
    # the ledger without a curve is a launch of its own
    q.l.part, q.l.curve = None, None
    assert _lib().st_qrollout_ledger_launch(C.byref(q), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert bands["curve"].same(snaps["curve"]) and bands["part"].same(snaps["part"])
    assert not bool((bands["state_out"].cpu() == -7).all()) and bands["state_out"].guards_intact()
