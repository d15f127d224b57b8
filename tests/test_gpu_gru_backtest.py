"""The GRU episode rollout kernel (``csrc/gru_rollout.hip``) against its PyTorch oracle, the env mirror, itself
cut in pieces, and the actor it shares its per-bar arithmetic with.

A rollout feeds its own actions back into its inputs, so one near-tie flips a trajectory for good.  The tests
therefore teacher-force: the kernel's own action trace is replayed through ``reference_gru_rollout(
forced_actions=...)`` on the CPU, which visits the same states.  Three rules (tests/gru_backtest_refs.py,
shown to reject perturbed traces in tests/test_gru_backtest.py):

(a) everything downstream of the actions -- return, trades, bars long, position, entry, the reward trace -- is
    exact float32 arithmetic and must be bit-equal;
(b) the traced action is the first maximum of the kernel's own traced Q row on every exploiting pair, and the
    Philox mirror's random action on every exploring pair, with no near-tie exclusion;
(c) ``||q - q_ref|| / ||q_ref||`` stays under a bound computed on the CPU for the test's own inputs: a quarter
    of the relative norm of the quantisation effect (oracle with every rounding point emulated minus the plain
    GRU on the same forced actions).  The effect is 1.3e-2 to 1.8e-2 here, the bound 3.4e-3 to 4.5e-3; the oracle
    in float32 against float64 stays at or under 1.2e-3.  Measured on an MI355X (profiles/gru_backtest.md): 2.9e-6
    on one bar, 2.5e-4 to 6.6e-4 with episodes of 4 or 5 bars, 2.1e-3 and 2.3e-3 over 40 and 70 unbroken bars.
"""
import ctypes as C
import math

import pytest
import torch

import gru_backtest_refs as R

pytestmark = pytest.mark.gpu

SEED = 3
EXACT_OUT = ("ret", "trades", "long", "position", "entry")
TRACES = ("actions", "q", "reward")


def _policy(params, seed=SEED):
    from sharetrade.serve.gru_rollout import GruPolicy

    return GruPolicy(params, device=torch.device("cuda", 0), seed=seed)


def _run(pol, close, feat, **kw):
    res = pol.backtest(close.cuda(), feat.cuda(), trace=True, **kw)
    torch.cuda.synchronize()
    out = {k: getattr(res, k).cpu() for k in EXACT_OUT + TRACES + ("h",)}
    assert out["actions"].dtype == torch.int8 and int(out["actions"].min()) >= 0 and int(out["actions"].max()) <= 2
    return out


def _same(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if x.is_floating_point():
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def _forced_check(E, steps, ep_len, wseed, *, centre=None, shares=True, **kw):
    """Kernel run -> its action trace replayed through the oracle -> rules (a), (b), (c)."""
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    close, feat = R.bars(E, steps + 8)
    params = R.centred_params(wseed, *(centre or (E, steps, ep_len)))
    if shares:   # the oracle alone: the greedy policy of these weights uses every action
        sh = R.action_shares(reference_gru_rollout(params, close, feat, steps=steps, ep_len=ep_len)["actions"])
        print(f"[meas] E={E} steps={steps} ep_len={ep_len}: oracle action shares {sh}")
        assert min(sh) >= 0.10, sh
    out = _run(_policy(params), close, feat, steps=steps, ep_len=ep_len, **kw)
    bound, ref = R.q_bound(params, close, feat, out["actions"], steps=steps, ep_len=ep_len)
    R.check_trace(out, ref, bound, label=f"E={E} steps={steps} ep_len={ep_len} seed={wseed} {kw}")
    return out


@pytest.mark.parametrize("E,steps,ep_len,wseed", [
    (1, 1, 390, 3),        # one env, one bar (weights centred on the 48 x 40 case: one bar cannot centre a head)
    (33, 23, 5, 3),        # a partial second chunk, four resets, a partial last episode
    (48, 40, 1000, 3),
    (48, 70, 1000, 1),     # more than 64 bars
])
def test_greedy_rollout_teacher_forced(native_built, E, steps, ep_len, wseed):
    from sharetrade.ops import gru as G

    one = E == 1
    _forced_check(E, steps, ep_len, wseed, centre=(48, 40, 1000) if one else None, shares=not one)
    blk = int(G.lib().st_gru_rollout_block())
    assert blk >= 0
    if blk and steps == 70:   # a kernel that stages bars per block: two blocks and a tail
        _forced_check(48, 2 * blk + 3, 1000, wseed)


def test_grid_strides_over_chunks(native_built):
    """100 envs = 4 chunks (the last partial) on 1 and 3 workgroups: bit-equal to one workgroup per chunk."""
    base = _forced_check(100, 9, 4, 3)
    close, feat = R.bars(100, 9 + 8)
    pol = _policy(R.centred_params(3, 100, 9, 4))
    for grid in (1, 3):
        out = _run(pol, close, feat, steps=9, ep_len=4, grid=grid)
        _same(out, base, EXACT_OUT + TRACES + ("h",))


@pytest.mark.parametrize("env_offset,start,origin", [(0, 0, None), (1000, 0, None), (0, 4, 2)])
def test_random_policy_is_the_env_mirror(native_built, env_offset, start, origin):
    """epsilon = 0: every action is the Philox mirror's, so every output equals the env alone bit for bit."""
    from sharetrade.serve.gru_rollout import simulate_minute_actions

    E, steps, ep_len = 33, 23, 5
    close, feat = R.bars(E, start + steps + 8)
    out = _run(_policy(R.centred_params(3, E, steps, ep_len)), close, feat, start=start, steps=steps, ep_len=ep_len,
               origin=origin, greedy=False, epsilon=0.0, env_offset=env_offset)
    ex, rnd = R.mirror_draws(SEED, E, start, steps, 0.0, env_offset)
    assert not bool(ex.any())
    assert torch.equal(out["actions"].long(), rnd)
    want = simulate_minute_actions(close, rnd.to(torch.int8), start=start, ep_len=ep_len, origin=origin)
    _same(out, want, EXACT_OUT + ("reward",))
    assert len(set(rnd.flatten().tolist())) == 3


def test_epsilon_greedy_teacher_forced(native_built):
    """epsilon = 0.6: exploiting pairs take the first maximum of their own Q row, exploring pairs the mirror's draw."""
    E, steps, ep_len, eps = 33, 23, 5, 0.6
    close, feat = R.bars(E, steps + 8)
    params = R.centred_params(3, E, steps, ep_len)
    out = _run(_policy(params), close, feat, steps=steps, ep_len=ep_len, greedy=False, epsilon=eps)
    ex, rnd = R.mirror_draws(SEED, E, 0, steps, eps)
    assert 0.3 < float(ex.float().mean()) < 0.9
    bound, ref = R.q_bound(params, close, feat, out["actions"], steps=steps, ep_len=ep_len)
    R.check_trace(out, ref, bound, exploit=ex, rnd=rnd, label="epsilon 0.6")


def test_pieces_reproduce_the_whole(native_built):
    """48 envs x 40 bars, episodes of 7: bars 0..16 then 17..39 with the same origin against one launch."""
    E, steps, ep_len, cut = 48, 40, 7, 17
    close, feat = R.bars(E, steps + 8)
    pol = _policy(R.centred_params(3, 48, 40, 1000))
    whole = _run(pol, close, feat, steps=steps, ep_len=ep_len)
    a = _run(pol, close, feat, steps=cut, ep_len=ep_len)
    b = _run(pol, close, feat, start=cut, steps=steps - cut, ep_len=ep_len, origin=0, h0=a["h"].cuda(),
             position=a["position"].cuda(), entry=a["entry"].cuda())
    both = {k: torch.cat([a[k], b[k]], dim=1) for k in TRACES}
    _same(both, whole, TRACES)
    _same(b, whole, ("position", "entry", "h"))
    assert torch.equal(a["trades"] + b["trades"], whole["trades"]) and torch.equal(a["long"] + b["long"], whole["long"])
    # the return is the float32 sum of the rewards in bar order, of the whole and of each piece
    for o in (whole, a, b):
        s = torch.zeros(E)
        for i in range(o["reward"].shape[1]):
            s = s + o["reward"][:, i]
        assert torch.equal(s, o["ret"])
    assert int(whole["trades"].sum()) > 0 and len(set(whole["actions"].flatten().tolist())) == 3


def test_rollout_agrees_with_the_actor(native_built):
    """One greedy actor launch (4 bars from a shared start bar, no update) and a 4-bar rollout of the learner's
    weights on the learner's own bank: the last bar's Q row and action, positions, episode returns and the
    recurrent state are equal bit for bit on every env whose rollout met no near-tie."""
    from sharetrade.config import preset_config
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.trainer.recurrent import RecurrentDQN

    cfg = preset_config("recurrent")
    cfg.agent.epsilon, cfg.agent.ramp = math.inf, 1.0
    d = RecurrentDQN(cfg, torch.device("cuda", 0), envs=64, seq=4, burn_in=1, bars=600, ep_len=390, batch=128,
                     replay_segments=1024, actor_kernel="single")
    d.P["w_q"].mul_(30.0)            # a Q head wide enough that near-ties are rare
    d.pack("on", into=0)
    d.pack("on", into=1)
    t0 = 100
    d.pos.fill_(t0)
    d.ep_start.fill_(t0)
    d.ctrl.fill_(1)                  # launch counter 1: global steps 4 .. 7, past the exploit ramp of 1 step
    q_out = torch.zeros(d.E, 4, device="cuda")
    d._act.q_out = q_out.data_ptr()
    pol = GruPolicy.from_learner(d)
    res = pol.backtest(d.close, d.feat, start=t0, steps=d.S, ep_len=d.ep_len, cost=d.cost, origin=t0, trace=True,
                       h0=d.h.clone(), position=d.position.clone(), entry=d.entry.clone())
    d.act()
    torch.cuda.synchronize()
    q = res.q.cpu()
    top2 = q.topk(2, dim=-1).values
    ok = ((top2[..., 0] - top2[..., 1]) > 1e-3 * (q.abs().max(-1).values + 1e-3)).all(dim=1)
    print(f"[meas] envs compared with the actor: {int(ok.sum())} of {ok.numel()}")
    assert float(ok.float().mean()) >= 0.8
    qo = q_out.cpu()
    assert torch.equal(qo[:, :3][ok].view(torch.int32), q[:, -1][ok].view(torch.int32))
    assert torch.equal(qo[:, 3][ok].long(), res.actions.cpu()[:, -1][ok].long())
    assert torch.equal(d.position.cpu()[ok], res.position.cpu()[ok])
    assert torch.equal(d.ep_ret.cpu()[ok].view(torch.int32), res.ret.cpu()[ok].view(torch.int32))
    assert torch.equal(d.h.cpu()[ok].view(torch.int32), res.h.cpu()[ok].view(torch.int32))
    assert int(d.pos[0]) == t0 + d.S and len(set(res.actions.cpu().flatten().tolist())) >= 2


def test_checkpoint_policy_equals_the_learners(native_built, tmp_path):
    from sharetrade.config import preset_config
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.trainer import runs
    from sharetrade.trainer.recurrent import RecurrentDQN

    cfg = preset_config("recurrent")
    dev = torch.device("cuda", 0)
    d = RecurrentDQN(cfg, dev, envs=64, seq=4, burn_in=1, bars=600, ep_len=5, batch=128, replay_segments=1024)
    w0 = d.flat.clone()
    runs.run("recurrent", cfg, 2, device=dev, ckpt_dir=str(tmp_path), ckpt_every=2, graph=False, learner=d,
             log_every=0)
    assert not torch.equal(w0, d.flat)
    a = GruPolicy.from_checkpoint(str(tmp_path), device=dev)
    b = GruPolicy.from_learner(d)
    assert a.seed == b.seed
    for n in a.params:
        assert torch.equal(a.params[n], b.params[n]), n
    close, feat = R.bars(40, 31)
    ra = a.backtest(close.cuda(), feat.cuda(), ep_len=7, trace=True)
    rb = b.backtest(close.cuda(), feat.cuda(), ep_len=7, trace=True)
    held = d.backtest(envs=64, bars=31, ep_len=7)   # the learner's wrapper: held-out bars, nothing of its state
    torch.cuda.synchronize()
    for k in EXACT_OUT + TRACES + ("h",):
        assert torch.equal(getattr(ra, k), getattr(rb, k)), k
    assert held.steps == 30 and held.ret.shape == (64,) and bool(torch.isfinite(held.ret).all())
    from sharetrade.persist import checkpoint as ck

    ck.save(str(tmp_path / "other.stck"), {"flat": d.flat.cpu()}, {"kind": "deep"})
    with pytest.raises(ValueError, match="recurrent"):
        GruPolicy.from_checkpoint(str(tmp_path / "other.stck"), device=dev)


def test_stream_and_strides(native_built):
    E, steps, ep_len = 48, 40, 7
    close, feat = R.bars(E, steps + 8)
    pol = _policy(R.centred_params(3, 48, 40, 1000))
    base = _run(pol, close, feat, steps=steps, ep_len=ep_len)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = _run(pol, close, feat, steps=steps, ep_len=ep_len)
    _same(out, base, EXACT_OUT + TRACES + ("h",))
    wide_c = torch.zeros(E, close.shape[1] + 5).cuda()
    wide_f = torch.zeros(E, close.shape[1] + 5, 8, dtype=torch.bfloat16).cuda()
    with pytest.raises(ValueError, match="contiguous"):
        pol.backtest(wide_c[:, :close.shape[1]], feat.cuda(), steps=steps, ep_len=ep_len)
    with pytest.raises(ValueError, match="contiguous"):
        pol.backtest(close.cuda(), wide_f[:, :close.shape[1]], steps=steps, ep_len=ep_len)


def test_launcher_refuses_bad_bounds(native_built):
    """Return codes only: hipErrorInvalidValue before anything is launched."""
    from sharetrade.ops import gru as G
    from sharetrade.ops import native

    E, T = 8, 20
    close, feat = R.bars(E, T)
    close, feat = close.cuda(), feat.cuda()
    pol = _policy(R.centred_params(3, 48, 40, 1000))
    ret = torch.zeros(E, T, device="cuda")
    outs = {k: torch.full((E,), -7, dtype=dt, device="cuda") for k, dt in
            (("out_ret", torch.float32), ("out_trades", torch.int32), ("out_long", torch.int32),
             ("out_position", torch.int32), ("out_entry", torch.float32))}

    def args(**over):
        a = G.RolloutArgs()
        for n, t in pol.packed.items():
            setattr(a, n, t.data_ptr())
        a.feat, a.close, a.ret = feat.data_ptr(), close.data_ptr(), ret.data_ptr()
        for k, t in outs.items():
            setattr(a, k, t.data_ptr())
        a.E, a.T, a.start, a.steps, a.origin, a.ep_len = E, T, 0, 5, 0, 5
        a.eps, a.cost, a.inv_ep_len = math.inf, 0.01, 0.2
        for k, v in over.items():
            setattr(a, k, v)
        return a

    L = G.lib()
    INVALID = 1
    bad = [dict(E=0), dict(steps=0), dict(ep_len=0), dict(origin=1), dict(start=-1, origin=-1),
           dict(start=T - 5, origin=0), dict(steps=T), dict(out_ret=None), dict(close=None), dict(whh8=None)]
    for over in bad:
        assert L.st_gru_rollout_launch(C.byref(args(**over)), 0, native.stream_handle()) == INVALID, over
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == -7).all()), k   # nothing ran
    assert L.st_gru_rollout_launch(C.byref(args(steps=T - 1)), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert bool((outs["out_trades"] >= 0).all())
