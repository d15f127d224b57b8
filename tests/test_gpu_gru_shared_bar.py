"""The GRU bar against recorded outputs of the kernels before they shared one definition of it.

The other GRU tests compare the four kernels (single actor, pair actor, rollout, server) with each other and,
teacher-forced, with the oracle; an error common to all four could slip through both.  This one pins the rollout
and the pair actor to ``tests/golden/gru_bar_parent_seeded.npz``: outputs recorded once on an MI355X from this
project's own commit f5527cf (the last one with the bar written out in each kernel), from seeded inputs, by
``tools/record_gru_bar_golden.py`` -- its docstring has the command and what each array is.  ``h`` is compared
through the SHA-256 of its bytes and, for a readable failure, every 16th env's row; everything else in full.
The rollout's bars and ``b_q`` come from the fixture (the rest of its weights from ``init_params(3)``); the
actor's inputs are the learner's own GPU-generated bank and initial weights, whose sums are checked first.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_bar_parent_seeded.npz")


def _sha(t):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).digest(), dtype=np.uint8)


def _same_h(h, g, pre):
    h = h.cpu()
    assert torch.equal(_bits(h[::16]), _bits(g[pre + "_h_rows"])), f"{pre} h rows"
    assert np.array_equal(_sha(h), g[pre + "_h_sha256"]), f"{pre} h"


def _bits(x):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return t.view(torch.int32) if t.is_floating_point() else t


def test_rollout_and_pair_actor_equal_the_recorded_parent(native_built):
    from sharetrade.config import preset_config
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.trainer.recurrent import RecurrentDQN

    g = np.load(GOLDEN)
    dev = torch.device("cuda", 0)
    # ---- the rollout
    E, steps, ep_len = 96, 9, 7
    close = torch.from_numpy(g["ro_close"])
    feat = torch.from_numpy(g["ro_feat"]).view(torch.bfloat16)
    assert close.shape == (E, steps + 2) and feat.shape == (E, steps + 2, 8)
    params = gq.init_params(3)
    params["w_q"] = 30.0 * params["w_q"]
    params["b_q"] = torch.from_numpy(g["ro_b_q"])
    res = GruPolicy(params, device=dev, seed=3).backtest(close.cuda(), feat.cuda(), steps=steps, ep_len=ep_len,
                                                         trace=True)
    torch.cuda.synchronize()
    assert len(set(g["ro_actions"].flatten().tolist())) == 3
    for k in ("actions", "position", "ret"):
        got, want = getattr(res, k).cpu(), g["ro_" + k]
        assert got.numpy().dtype == want.dtype and torch.equal(_bits(got), _bits(want)), f"rollout {k}"
    _same_h(res.h, g, "ro")
    # ---- one pair-actor launch
    cfg = preset_config("recurrent")
    cfg.agent.epsilon, cfg.agent.ramp = 0.9, 1.0
    d = RecurrentDQN(cfg, dev, envs=96, seq=4, burn_in=1, bars=600, ep_len=5, batch=128, replay_segments=1024,
                     actor_kernel="pair")
    d.P["w_q"].mul_(30.0)
    d.pack("on", into=0)
    d.pack("on", into=1)
    d.ctrl.fill_(1)                  # launch counter 1: global steps 4 .. 7, past the exploit ramp of 1 step
    q_out = torch.zeros(d.E, 4, device="cuda")
    d._act.q_out = q_out.data_ptr()
    d.act()
    torch.cuda.synchronize()
    in_sum = np.array([float(t.double().sum()) for t in (d.close, d.feat, d.flat, d.pos)])   # (pos: after the launch)
    assert np.array_equal(in_sum, g["act_in_sum"]), "the actor's seeded inputs were not reproduced"
    for k, t in (("ep_ret", d.ep_ret), ("position", d.position), ("q_out", q_out)):
        want = g["act_" + k]
        assert t.cpu().numpy().dtype == want.dtype and torch.equal(_bits(t.cpu()), _bits(want)), f"actor {k}"
    _same_h(d.h, g, "act")
