"""Shared inputs of the GRU backtest tests (tests/test_gru_backtest.py on the CPU, tests/test_gpu_gru_backtest.py
on the GPU): bars, weights whose greedy policy uses all three actions, and the three rules a kernel trace is
held to.  Everything here runs on the CPU; nothing is cached on disk.

Weights: plain random-init weights are useless for a policy test (the greedy policy takes one action on almost
every bar, |q| <= 0.034), so the Q head is widened (``30 * w_q``) and centred: ``b_q`` is minus the per-action
mean of Q over one oracle pass with uniformly random forced actions.
"""
import functools

import numpy as np
import torch


@functools.lru_cache(maxsize=None)
def bars(E, T, seed=3):
    """(close [E, T] fp32, feat [E, T, 8] bf16) from the NumPy mirror of the bar generator."""
    from sharetrade.data import minute_bars as mb

    c, f = mb.generate_numpy(E, T, seed=seed)
    return torch.from_numpy(c), torch.from_numpy(f).to(torch.bfloat16)


def random_actions(E, steps, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 3, (E, steps), generator=g).to(torch.int8)


@functools.lru_cache(maxsize=None)
def _centred(seed, E, steps, ep_len):
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    close, feat = bars(E, steps + 8)
    p = gq.init_params(seed)
    p["w_q"] = 30.0 * p["w_q"]
    out = reference_gru_rollout(p, close, feat, steps=steps, ep_len=ep_len, forced_actions=random_actions(E, steps))
    p["b_q"] = -out["q"].double().mean(dim=(0, 1)).float()
    return p


def centred_params(seed, E, steps, ep_len):
    """Fresh copies of the centred-head weights for bars(E, steps + 8)."""
    return {n: t.clone() for n, t in _centred(seed, E, steps, ep_len).items()}


def action_shares(actions):
    a = actions.long().flatten()
    return [float((a == k).float().mean()) for k in range(3)]


def replay(params, close, feat, actions, **kw):
    """Teacher-forced oracle pass (float64, every rounding point emulated unless ``emulate`` says otherwise)."""
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    return reference_gru_rollout(params, close, feat, forced_actions=actions, **kw)


def q_bound(params, close, feat, actions, **kw):
    """Rule (c)'s bound for these inputs: a quarter of the relative norm of the quantisation effect, oracle with
    every rounding point emulated minus the plain GRU on the same forced actions.  An error at any quantisation
    point (a wrong scale, a skipped rounding) is at least the size of that effect; summation order and rare fp8
    boundary flips are far below it.  Returns (bound, emulated oracle pass)."""
    ref = replay(params, close, feat, actions, **kw)
    plain = replay(params, close, feat, actions, emulate=False, **kw)
    effect = float((ref["q"].double() - plain["q"].double()).norm() / plain["q"].double().norm())
    return 0.25 * effect, ref


EXACT = ("ret", "trades", "long", "position", "entry", "reward")


def check_trace(out, ref, bound, *, exploit=None, rnd=None, label=""):
    """The three rules of the teacher-forced check.  ``out``: the trace under test (CPU tensors), ``ref``: the
    oracle's pass forced to ``out['actions']``, ``exploit`` [E, steps] bool (None: greedy, all exploit) and
    ``rnd`` [E, steps] the Philox mirror's random actions.  Returns the measured relative Q error."""
    # (a) everything downstream of the actions is exact arithmetic
    for k in EXACT:
        assert out[k].dtype == ref[k].dtype and torch.equal(out[k], ref[k]), f"{label} {k}"
    # (b) the action is the first maximum of the trace's own Q row (no near-tie exclusion: it is its own Q)
    acts = out["actions"].long()
    own = out["q"].argmax(-1)
    if exploit is None:
        exploit = torch.ones_like(acts, dtype=torch.bool)
    assert torch.equal(acts[exploit], own[exploit]), f"{label} exploiting actions"
    if rnd is not None:
        assert torch.equal(acts[~exploit], rnd.long()[~exploit]), f"{label} random actions"
    # (c) the Q rows against the oracle's
    q, q_ref = out["q"].double(), ref["q"].double()
    rel = float((q - q_ref).norm() / q_ref.norm())
    print(f"[meas] {label}: rel q error {rel:.3e} (bound {bound:.3e})")
    assert rel < bound, (label, rel, bound)
    return rel


def mirror_draws(seed, E, start, steps, epsilon, env_offset=0):
    """(exploit [E, steps] bool, random action [E, steps]) of the backtest's Philox draws."""
    from sharetrade.serve.gru_rollout import draws

    ids = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset)).astype(np.uint32)
    ex = torch.empty(E, steps, dtype=torch.bool)
    rnd = torch.empty(E, steps, dtype=torch.int64)
    for i in range(steps):
        u0, u1 = draws(seed, ids, start + i)
        ex[:, i] = torch.from_numpy(u0 < np.float32(epsilon))
        rnd[:, i] = torch.from_numpy(np.minimum((u1 * np.float32(3)).astype(np.int64), 2))
    return ex, rnd
