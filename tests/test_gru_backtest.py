"""The GRU backtest's oracle and host side on the CPU: the oracle's env against ``env/minute.py``, the three rules
the GPU test holds a kernel trace to (they must reject perturbed traces), ``summary()`` and the command line."""
import json
import math

import numpy as np
import pytest
import torch

import gru_backtest_refs as R

E, STEPS, EP = 33, 23, 5


def test_oracle_env_is_the_minute_env_bar_by_bar():
    """Random actions from bar 3 with episodes counted from bar 1: rewards, returns, positions, entries and the
    env columns of the x row equal a per-series loop over env/minute.py (restart draws replaced by the next bar)."""
    from sharetrade.data import minute_bars as mb
    from sharetrade.env import minute as me
    from sharetrade.serve.gru_rollout import _Env, simulate_minute_actions

    close, feat = R.bars(7, STEPS + 8)
    acts = R.random_actions(7, STEPS)
    start, origin, cost = 3, 1, 0.01
    out = simulate_minute_actions(close, acts, start=start, ep_len=EP, cost=cost, origin=origin)
    c_np, f_np = close.numpy(), feat.float().numpy()
    ret = mb.bar_returns(c_np)
    T = c_np.shape[1]
    env = _Env(7, cost, None, None, torch.device("cpu"))
    es0 = origin + (start - origin) // EP * EP
    states = [me.MinuteEnvState(start, es0) for _ in range(7)]
    sums = np.zeros(7, np.float32)
    for i in range(STEPS):
        t = start + i
        xe = env.x_env(close[:, t], t - states[0].es, np.float32(1.0 / EP)).numpy()
        for e, st in enumerate(states):
            assert st.t == t
            assert np.array_equal(xe[e], me.obs(f_np[e, t], c_np[e, t], st, EP)[8:12]), (e, t)
            rew, done, _ = me.step(st, int(acts[e, i]), c_np[e], ret[e], T, EP, cost, 0.0)
            assert np.float32(rew) == out["reward"][e, i].numpy(), (e, t)
            sums[e] = sums[e] + np.float32(rew)
            assert done == ((t + 1 - origin) % EP == 0)
            if done:   # no random restart: the next episode starts at the next bar, entry cleared
                st.t, st.es, st.entry = t + 1, t + 1, 0.0
        env.step(acts[:, i], close[:, t], torch.from_numpy(ret[:, t]), (t + 1 - origin) % EP == 0)
    assert np.array_equal(out["ret"].numpy(), sums)
    assert np.array_equal(out["position"].numpy(), np.array([st.pz for st in states]))
    assert np.array_equal(out["entry"].numpy(), np.array([st.entry for st in states], np.float32))
    assert int(out["trades"].sum()) > 0 and int(out["long"].sum()) > 0


@pytest.fixture(scope="module")
def case():
    close, feat = R.bars(E, STEPS + 8)
    p = R.centred_params(3, E, STEPS, EP)
    kw = dict(steps=STEPS, ep_len=EP)
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    # a stand-in for the kernel: the oracle in float32 arithmetic, greedy
    out = reference_gru_rollout(p, close, feat, dtype=torch.float32, **kw)
    bound, ref = R.q_bound(p, close, feat, out["actions"], **kw)
    return p, close, feat, kw, out, bound, ref


def test_centred_head_uses_every_action(case):
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    p, close, feat, kw, _, _, _ = case
    sh = R.action_shares(reference_gru_rollout(p, close, feat, **kw)["actions"])
    assert min(sh) >= 0.10, sh


def test_rules_accept_the_float32_oracle(case):
    _, _, _, _, out, bound, ref = case
    rel = R.check_trace(out, ref, bound, label="float32 oracle")
    assert 1e-3 < 4 * bound < 5e-2, bound   # the quantisation effect itself: percent level
    assert rel < bound / 3


def test_rules_reject_a_flipped_action(case):
    """The trace claims another action on one bar than the one its rewards came from."""
    p, close, feat, kw, out, bound, _ = case
    bad = {k: v.clone() for k, v in out.items()}
    e, i = 5, 7
    bad["actions"][e, i] = (int(bad["actions"][e, i]) + 1) % 3
    ref = R.replay(p, close, feat, bad["actions"], **kw)
    with pytest.raises(AssertionError):
        R.check_trace(bad, ref, bound, label="flipped")


@pytest.mark.parametrize("emulate", [("x", "w_ih", "w_hh", "h"), False], ids=["plain-q-head", "plain-gru"])
def test_rules_reject_a_missing_rounding_point(case, emulate):
    """A net that skips the Q head's bf16 rounding, or every rounding: its own greedy trace is self-consistent
    (rules a, b) but its Q rows are off by more than the bound."""
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    p, close, feat, kw, _, _, _ = case
    out = reference_gru_rollout(p, close, feat, emulate=emulate, **kw)
    bound, ref = R.q_bound(p, close, feat, out["actions"], **kw)
    for k in R.EXACT:
        assert torch.equal(out[k], ref[k]), k
    with pytest.raises(AssertionError):
        R.check_trace(out, ref, bound, label=str(emulate))
    rel = float((out["q"].double() - ref["q"].double()).norm() / ref["q"].double().norm())
    assert rel > bound, (rel, bound)


def test_pieces_equal_the_whole_on_the_oracle(case):
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    p, close, feat, _, _, _, _ = case
    whole = reference_gru_rollout(p, close, feat, steps=STEPS, ep_len=7)
    a = reference_gru_rollout(p, close, feat, steps=9, ep_len=7)
    b = reference_gru_rollout(p, close, feat, start=9, steps=STEPS - 9, ep_len=7, origin=0, h0=a["h"],
                              position=a["position"], entry=a["entry"])
    for k in ("actions", "q", "reward"):
        assert torch.equal(torch.cat([a[k], b[k]], dim=1), whole[k]), k
    for k in ("position", "entry", "h"):
        assert torch.equal(b[k], whole[k]), k
    assert torch.equal(a["trades"] + b["trades"], whole["trades"]) and torch.equal(a["long"] + b["long"], whole["long"])


def test_summary_arithmetic():
    from sharetrade.serve.gru_rollout import GruBacktestResult

    ret = torch.tensor([1.0, -2.0, 0.5, 4.5])
    z = torch.zeros(4, dtype=torch.int32)
    s = GruBacktestResult(ret=ret, trades=z + 3, long=torch.tensor([10, 0, 5, 5], dtype=torch.int32), position=z,
                          entry=ret * 0, start=2, steps=20, ep_len=10, origin=0).summary()
    assert s["n"] == 4 and s["steps"] == 20 and s["trades"] == 12
    assert s["mean"] == 1.0 and s["median"] == 0.5
    assert math.isclose(s["std"], math.sqrt((0.0 + 9.0 + 0.25 + 12.25) / 4))
    assert s["per_episode"] == 0.5 and s["long_frac"] == 0.25


def test_policy_from_checkpoint_on_the_cpu(tmp_path):
    """A checkpoint file, its directory and a data-parallel run's directory (rank 0) give the saved nets; another
    run's checkpoint is refused by its kind."""
    from sharetrade.models import gru_qnet as gq
    from sharetrade.persist import checkpoint as ck
    from sharetrade.serve.gru_rollout import PARAM_NAMES, GruPolicy, checkpoint_kind

    p = gq.init_params(4)
    flat = torch.cat([p[n].flatten() for n in PARAM_NAMES])
    run = tmp_path / "run" / "rank0"
    run.mkdir(parents=True)
    mgr = ck.CheckpointManager(str(run), interval=1)
    meta = {"kind": "recurrent", "config": {"agent": {"seed": 9, "epsilon": 0.8}}}
    mgr.save(1, {"flat": flat * 3, "tflat": flat}, meta)
    path = mgr.save(2, {"flat": flat, "tflat": flat * 2}, meta)
    for where in (path, str(run), str(tmp_path / "run")):
        assert checkpoint_kind(where) == "recurrent"
        pol = GruPolicy.from_checkpoint(where, device="cpu")
        assert pol.seed == 9 and pol.epsilon == 0.8 and pol.packed is None
        for n in PARAM_NAMES:
            assert torch.equal(pol.params[n], p[n]), n
    tg = GruPolicy.from_checkpoint(path, net="target", device="cpu")
    assert torch.equal(tg.params["w_hh"], 2 * p["w_hh"])
    other = str(tmp_path / "deep.stck")
    ck.save(other, {"flat": flat}, {"kind": "deep"})
    assert checkpoint_kind(other) == "deep" and checkpoint_kind(str(tmp_path)) is None
    with pytest.raises(ValueError, match="'deep' run"):
        GruPolicy.from_checkpoint(other, device="cpu")
    close, feat = R.bars(3, 20)
    res = pol.backtest(close, feat, ep_len=6, trace=True)
    assert res.backend == "torch" and res.steps == 19 and res.actions.shape == (3, 19)
    with pytest.raises(RuntimeError, match="GPU"):
        pol.backtest(close, feat, backend="hip")


def _cli(capsys, *argv):
    from sharetrade.__main__ import main

    assert main(list(argv)) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_command_line_gru_path_on_the_cpu(capsys, tmp_path):
    out = _cli(capsys, "backtest", "--policy", "gru", "--synthetic", "4", "--bars", "60", "--ep-len", "20",
               "--device", "cpu", "--trace-out", str(tmp_path / "tr"))
    assert out["policy_kind"] == "gru" and out["backend"] == "torch" and out["series"] == 4
    assert out["bars"] == 60 and out["steps"] == 59 and out["weights"] == "init"
    for k in ("policy", "always_long", "uniform_random", "flat"):
        assert math.isfinite(out[k]["mean"]) and out[k]["n"] == 4
    assert out["flat"]["mean"] == 0.0 and out["flat"]["trades"] == 0 and out["flat"]["long_frac"] == 0.0
    assert out["always_long"]["long_frac"] == 1.0
    assert np.load(tmp_path / "tr" / "actions.npy").shape == (4, 59)
    assert np.load(tmp_path / "tr" / "reward.npy").shape == (4, 59)


def test_command_line_refuses_csv_on_the_gru_path(tmp_path):
    from sharetrade.__main__ import main

    with pytest.raises(SystemExit) as ei:
        main(["backtest", "--policy", "gru", "--csv", str(tmp_path / "x.csv"), "--device", "cpu"])
    assert ei.value.code == 2


def test_command_line_mlp_path_is_unchanged(capsys):
    """A non-recurrent invocation prints what it printed before the GRU path existed: the keys and values of
    the MLP backtest (policy vs buy-and-hold vs uniform random), with or without ``--policy mlp``."""
    from sharetrade.config import preset_config
    from sharetrade.serve import PolicyServer

    args = ("backtest", "--preset", "flagship", "--synthetic", "2", "--device", "cpu", "--set", "data.length=230")
    out = _cli(capsys, *args)
    assert list(out) == ["series", "days", "steps", "budget", "backend", "weights", "policy", "buy_and_hold",
                         "uniform_random"]
    assert out == _cli(capsys, *args, "--policy", "mlp")
    cfg = preset_config("flagship")
    cfg.override(["data.length=230"])
    from sharetrade.data import prices as dp

    d = cfg.data
    P = torch.from_numpy(np.ascontiguousarray(
        dp.random_walk(d.length, d.start_price, d.volatility, d.seed, n_series=2), dtype=np.float32))
    res = PolicyServer(cfg, device=torch.device("cpu")).backtest(P)
    assert out["policy"] == res.summary() and out["series"] == 2 and out["days"] == 230
    assert out["steps"] == res.steps and out["weights"] == "init"
