"""The episode rollout kernel (``csrc/qrollout.hip``) against its PyTorch oracle and against the engine.

A rollout feeds its own actions back into its inputs, so one near-tie flips a trajectory for good.  The tests
therefore teacher-force: the kernel's own action trace is replayed through ``reference_rollout(forced_actions=
...)`` on the CPU, which visits the same states.  Everything downstream of the actions (budget, shares, counts,
equity) is then exact arithmetic and must be bit-equal; the Q rows differ only in the fp32 summation order
(tolerance of tests/test_gpu_serve.py), and the kernel's action must be the oracle's argmax wherever the
oracle's top-two margin is not a near-tie.  The epsilon-greedy draws are recomputed from the Philox mirror.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 201
BUDGET = 120.0
SEED = 3


def _prices(E, steps, extra=0):
    g = np.random.default_rng(3)
    p = 50.0 * np.exp(np.cumsum(g.normal(0, 0.02, size=(E, H + steps + extra)), axis=1))
    return torch.from_numpy(p.astype(np.float32))


def _cfg(features="relative", output_relu=False, compat=False):
    from sharetrade.config import preset_config

    cfg = preset_config("flagship")
    cfg.env.features = features
    cfg.env.budget = BUDGET
    cfg.env.compat_decisions = compat
    cfg.model.output_relu = output_relu
    cfg.agent.epsilon, cfg.agent.ramp = 0.9, 4.0
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

        self.cfg = cfg
        self.layout = qn.QNetLayout.from_config(cfg.model)
        self.params = qn.init_params(self.layout, cfg.model, seed=SEED, host_mirror=True)
        self.dev = self.params.cuda()
        self.dev_bf = self.dev.to(torch.bfloat16)
        self.kern = RolloutKernel(self.layout, self.dev, self.dev_bf, history=H,
                                  feat_mode=tr.FEATURES[cfg.env.features], output_relu=cfg.model.output_relu,
                                  budget0=cfg.env.budget, shares0=cfg.env.shares, compat=cfg.env.compat_decisions,
                                  epsilon=cfg.agent.epsilon, ramp=cfg.agent.ramp, key=rng.key_for(SEED, 0))

    def run(self, P, **kw):
        out = self.kern.run(P if P.is_cuda else P.cuda(), trace=True, **kw)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    def replay(self, P, actions, *, greedy=True, start=0, steps=None, budget=None, shares=None, env_offset=0,
               output_relu=None):
        from sharetrade.serve.rollout import reference_rollout

        c = self.cfg
        return reference_rollout(self.params, self.layout, P, history=H, feat_mode=c.env.features,
                                 output_relu=c.model.output_relu if output_relu is None else output_relu,
                                 budget0=c.env.budget, shares0=c.env.shares,
                                 compat=c.env.compat_decisions, epsilon=math.inf if greedy else c.agent.epsilon,
                                 ramp=c.agent.ramp, key_seed=SEED, start=start, steps=steps, budget=budget,
                                 shares=shares, env_offset=env_offset, forced_actions=actions)


def _clear(q_ref):
    """Rule (c): (env, day) pairs whose oracle top-two margin is not a near-tie."""
    top2 = q_ref.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) > 1e-3 * (q_ref.abs().max(-1).values + 1e-3)


def _clamped(pol, P, out, q_ref, **kw):
    """With an output ReLU a row whose three Q values are all negative is clamped to exactly (0, 0, 0): a tie
    that rule (c) excludes, though the action is determined (the first max: 0).  Such a row is clear when the
    oracle's largest pre-ReLU value is below 0 by rule (c)'s margin, 1e-3 * (max|q_pre| + 1e-3); the pre-ReLU
    rows come from a second replay of the same actions without the output ReLU."""
    if not pol.cfg.model.output_relu:
        return torch.zeros(q_ref.shape[:2], dtype=torch.bool)
    pre = pol.replay(P, out["actions"], output_relu=False, **kw)["q"]
    return (q_ref == 0).all(-1) & (pre.max(-1).values < -1e-3 * (pre.abs().max(-1).values + 1e-3))


def _check(pol, P, steps, *, greedy=True, env_offset=0, start=0):
    from sharetrade.utils import rng

    out = pol.run(P, start=start, steps=steps, greedy=greedy, env_offset=env_offset)
    ref = pol.replay(P, out["actions"], greedy=greedy, start=start, steps=steps, env_offset=env_offset)
    E = P.shape[0]
    assert out["actions"].shape == (E, steps) and int(out["actions"].min()) >= 0 and int(out["actions"].max()) <= 2
    # (a) everything downstream of the actions is exact
    for k in ("budget", "shares", "portfolio", "buys", "sells", "equity"):
        assert torch.equal(out[k], ref[k]), k
    # (b) Q rows: fp32 summation order only
    q, q_ref = out["q"], ref["q"]
    rel = float((q - q_ref).norm() / (q_ref.norm() + 1e-12))
    print(f"[meas] E={E} steps={steps} greedy={greedy}: rel q error {rel:.3e}")
    assert rel < 2e-3, rel
    # (c) the action is the oracle's argmax off the near-ties (of the exploiting envs)
    clamped = _clamped(pol, P, out, q_ref, greedy=greedy, start=start, steps=steps, env_offset=env_offset)
    clear = _clear(q_ref) | clamped
    acts = out["actions"].long()
    want = q_ref.argmax(-1)   # (0 on a clamped row)
    assert bool((want[clamped] == 0).all())
    if greedy:
        exploit = torch.ones_like(clear)
    else:
        c = pol.cfg.agent
        ids = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset)).astype(np.uint32)
        exploit = torch.empty_like(clear)
        for i in range(steps):
            t = start + i
            u1, u2 = rng.uniforms(SEED, 0, ids, t, stream=4)
            thr = np.minimum(np.float32(c.epsilon), np.float32(t) * np.float32(1.0 / c.ramp))
            ex = torch.from_numpy(u1 < thr)
            rnd = torch.from_numpy(np.minimum((u2 * np.float32(3)).astype(np.int64), 2))
            exploit[:, i] = ex
            assert torch.equal(acts[:, i][~ex], rnd[~ex]), f"random actions of day {t}"
    sel = clear & exploit
    assert torch.equal(acts[sel], want[sel])
    # (d) few near-ties
    excluded = float((~clear).float().mean())
    print(f"[meas] excluded (env, day) pairs: {excluded:.4%}")
    assert excluded < 0.02, excluded
    return out


@pytest.fixture(scope="module")
def pol(native_built):
    return _Policy(_cfg())


def _shapes():
    from sharetrade.serve.rollout import day_block

    D = day_block()
    return [(1, 1), (17, 40), (48, 40), (48, 2 * D + 3), (1000, 8)]


@pytest.mark.parametrize("case", range(5))
def test_rollout_teacher_forced(pol, case):
    E, steps = _shapes()[case]
    out = _check(pol, _prices(E, steps), steps)
    if (E, steps) == (48, 40):   # this input's trajectory takes every action and executes both trades
        assert {0, 1, 2} <= set(out["actions"].unique().tolist())
        assert int(out["buys"].sum()) > 0 and int(out["sells"].sum()) > 0


@pytest.mark.parametrize("E,steps,env_offset,start", [(48, 40, 0, 0), (17, 40, 1 << 20, 0), (48, 40, 5, 3)])
def test_rollout_epsilon_greedy(pol, E, steps, env_offset, start):
    _check(pol, _prices(E, steps, extra=start), steps, greedy=False, env_offset=env_offset, start=start)


@pytest.mark.parametrize("features,output_relu", [("raw", True), ("relative", True)])
def test_rollout_feature_modes(native_built, features, output_relu):
    pol = _Policy(_cfg(features, output_relu))
    out = _check(pol, _prices(48, 40), 40)
    if features == "raw":
        # greedy, the raw net of this seed holds on every day of this input (no trade, budget and shares constant):
        # the epsilon-greedy draws move the budget / shares inputs and execute both trades
        assert int(out["buys"].sum()) == 0 and int(out["sells"].sum()) == 0
        out = _check(pol, _prices(48, 40), 40, greedy=False)
        assert int(out["buys"].sum()) > 0 and int(out["sells"].sum()) > 0


def test_rollout_chained_launches_equal_one(pol):
    P = _prices(48, 40).cuda()
    whole = pol.run(P, steps=40)
    a = pol.kern.run(P, start=0, steps=20, trace=True)
    b = pol.kern.run(P, start=20, steps=20, budget=a["budget"], shares=a["shares"], trace=True)
    torch.cuda.synchronize()
    for k in ("budget", "shares", "portfolio"):
        assert torch.equal(b[k].cpu(), whole[k]), k
    for k in ("buys", "sells"):
        assert torch.equal((a[k] + b[k]).cpu(), whole[k]), k
    for k in ("actions", "q", "equity"):
        assert torch.equal(torch.cat([a[k], b[k]], dim=1).cpu(), whole[k]), k


def test_rollout_grid_stride_over_tiles(pol):
    """Fewer workgroups than 32-env tiles: a workgroup re-initialises its env state, price ring and feature
    staging for every further tile (one workgroup walks all four tiles, the last one partial)."""
    from sharetrade.serve.rollout import day_block

    steps = day_block() + 3
    P = _prices(100, steps)
    base = pol.run(P, steps=steps)
    for grid in (1, 3):
        out = pol.run(P, steps=steps, grid=grid)
        for k in base:
            assert torch.equal(out[k], base[k]), (grid, k)
    _check(pol, P, steps)


def test_rollout_compat_env_trades_from_the_start_state(native_built):
    pol = _Policy(_cfg(compat=True))
    P = _prices(48, 40)
    out = pol.run(P, steps=40)
    ref = pol.replay(P, out["actions"], steps=40)
    for k in ("budget", "shares", "portfolio", "buys", "sells", "equity"):
        assert torch.equal(out[k], ref[k]), k
    # every day starts from (b0, s0 = 0): at most one share, and the budget is b0 or b0 - price
    assert int(out["shares"].max()) <= 1 and int(out["sells"].sum()) == 0
    bought = out["shares"] == 1
    assert torch.equal(out["budget"][~bought], torch.full_like(out["budget"][~bought], BUDGET))
    assert torch.equal(out["budget"][bought], (BUDGET - P[:, -1])[bought])


def test_rollout_matches_engine_greedy_episode(native_built):
    """One greedy episode of the training engine (lr 0) and the backtest of its weights on its own bank end
    with the same portfolios, wherever the rollout met no near-tie."""
    from sharetrade.config import preset_config
    from sharetrade.serve import PolicyServer
    from sharetrade.trainer import benchkit
    from sharetrade.trainer.engine import VectorEngine

    cfg = preset_config("flagship")
    cfg.data.length = H + 40
    eng = VectorEngine(cfg, device=torch.device("cuda", 0), envs=64)
    ep0 = benchkit.reset_episodes(eng)
    with eng.policy_overrides(epsilon=math.inf, lr=0.0):
        eng.run(eng.T - eng.H)
        eng.synchronize()
    assert bool((eng.state.episodes > ep0).all())
    fin = eng.state.last_final.cpu()
    srv = PolicyServer(cfg, params=eng.params, device=eng.device, backend="native")
    res = srv.backtest(eng.prices, trace=True)
    torch.cuda.synchronize()
    assert res.steps == 40
    from sharetrade.serve.rollout import reference_rollout

    e = cfg.env
    ref = reference_rollout(eng.params.cpu(), srv.layout, eng.prices.cpu(), history=H, feat_mode=e.features,
                            output_relu=cfg.model.output_relu, budget0=e.budget, shares0=e.shares,
                            compat=e.compat_decisions, epsilon=math.inf, ramp=cfg.agent.ramp, key_seed=0,
                            forced_actions=res.actions.cpu())
    ok = _clear(ref["q"]).all(dim=1)
    print(f"[meas] envs compared with the engine: {int(ok.sum())} of {ok.numel()}")
    assert float(ok.float().mean()) >= 0.8
    assert torch.equal(res.final_portfolio.cpu()[ok], fin[ok])
    # the engine-level summary is the same launch reduced like greedy_episode_returns
    summ = benchkit.backtest_returns(eng)
    want = res.summary()
    assert summ["n"] == 64 and summ["steps"] == 40 and summ["complete_frac"] == 1.0
    assert summ["mean"] == want["mean"] and summ["median"] == want["median"] and abs(summ["std"] - want["std"]) < 1e-9


def test_rollout_strided_series_and_stream(pol):
    P = _prices(48, 40)
    base = pol.run(P, steps=40)
    wide = torch.zeros(48, P.shape[1] + 37)
    wide[:, : P.shape[1]] = P
    dev_wide = wide.cuda()
    out = pol.kern.run(dev_wide[:, : P.shape[1]], steps=40, trace=True)   # ld > T
    torch.cuda.synchronize()
    for k in base:
        assert torch.equal(out[k].cpu(), base[k]), k
    st = torch.cuda.Stream()
    Pd = P.cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        out2 = pol.kern.run(Pd, steps=40, trace=True)
    st.synchronize()
    for k in base:
        assert torch.equal(out2[k].cpu(), base[k]), k
