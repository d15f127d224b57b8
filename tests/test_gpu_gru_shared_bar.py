"""The GRU bar against recorded outputs of the kernels before they shared one definition of it.

The other GRU tests compare the four kernels (single actor, pair actor, rollout, server) with each other and,
teacher-forced, with the oracle; an error common to all four could slip through both.  This one pins the rollout
and the pair actor to ``tests/golden/gru_bar_parent_seeded.npz``: outputs recorded once on an MI355X from this
project's own commit f5527cf (the last one with the bar written out in each kernel), from seeded inputs, by
``tools/record_gru_bar_golden.py`` -- its docstring has the command and what each array is.  ``h`` is compared
through the SHA-256 of its bytes and, for a readable failure, every 16th env's row; everything else in full.
The rollout's bars and ``b_q`` come from the fixture (the rest of its weights from ``init_params(3)``); the
actor's inputs are the learner's own GPU-generated bank and initial weights, whose sums are checked first.

The learner's forward (``gru_seq_fwd_kernel``) joined the shared bar later and has its own fixture and test below,
and one cross-kernel check: its Q of a first step equals the backtest's for the same bar.
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


def _tool():
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import record_gru_seq_fwd_golden as rec

    return rec


def test_seq_fwd_equals_the_recorded_parent(native_built):
    """The learner's forward on the shared bar against ``tests/golden/gru_seq_fwd_parent_seeded.npz``: one
    st_gru_seq_fwd launch (B = 96, S = 3, mixed resets; online and target net) recorded on an MI355X from commit
    78d3a1e, the last one whose ``gru_seq_fwd_kernel`` carried its own copy of the prologue, the tile and the Q row,
    by ``tools/record_gru_seq_fwd_golden.py``, whose ``run_case`` is what runs here.  The saves, ``HT``, ``Q`` and
    ``Qt`` are compared bit for bit: the SHA-256 of each and, for a readable failure, every 16th row first."""
    import gru_learn_refs as R
    import test_gpu_gru_learn_kernels as T

    rec = _tool()
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "gru_seq_fwd_parent_seeded.npz"))
    in_sum, out = rec.run_case(T, R)
    assert np.array_equal(in_sum, g["in_sum"]), "the seeded inputs and packed weights were not reproduced"
    for name, v in out.items():
        r = rec.rows(name, v)
        want = g[name + "_rows"]
        assert r.dtype == want.dtype and torch.equal(_bits(r[rec.ROWS]), _bits(want)), f"{name} rows"
        assert np.array_equal(rec.sha(r), g[name + "_sha256"]), name


def test_seq_fwd_first_step_q_equals_the_rollouts(native_built):
    """One function for the learner and the actors: from h = 0, on the same packed weights and the same x rows, Q
    of step 0 of st_gru_seq_fwd (online net) equals the Q the backtest traces for its first bar, bit for bit
    (B = 32: one workgroup each; so it was before the learner's forward included the shared bar)."""
    import ctypes as C
    import math

    import gru_learn_refs as R
    import test_gpu_gru_learn_kernels as T
    from sharetrade.ops import native

    G, k = T._k()
    on, tg = T._packed(11), T._packed(12)
    B, S = 32, 1
    inp = R.fwd_inputs(B, S, "ones", seed=77)
    # the x row of a flat env at bar 0 of its episode: 8 features, then position 0, unrealised 0, elapsed 0, 1
    inp["x"][0, :, 8:] = 0.0
    inp["x"][0, :, 11] = 1.0
    inp["h0"][:] = 0.0
    rc, _, _, Q, _ = T._fwd_launch(G, k, inp, on, tg, B, S)
    assert rc == 0
    feat = torch.zeros(B, 2, 8, dtype=torch.bfloat16)
    feat[:, 0] = torch.from_numpy(np.ascontiguousarray(inp["x"][0, :, :8], dtype=np.float32)).to(torch.bfloat16)
    assert np.array_equal(feat[:, 0].float().numpy(), inp["x"][0, :, :8])   # (the inputs are bf16 values)
    dev = dict(device="cuda")
    feat, close, ret = feat.cuda(), torch.full((B, 2), 100.0, **dev), torch.zeros(B, 2, **dev)
    i32 = torch.int32
    outs = {"out_ret": torch.empty(B, **dev), "out_trades": torch.empty(B, dtype=i32, **dev),
            "out_long": torch.empty(B, dtype=i32, **dev), "out_position": torch.empty(B, dtype=i32, **dev),
            "out_entry": torch.empty(B, **dev), "tr_q": torch.full((B, 1, 3), float("nan"), **dev)}
    a = G.RolloutArgs()
    G.set_netw(a, {n: band.v for n, band in on["b"].items()})
    a.feat, a.close, a.ret = feat.data_ptr(), close.data_ptr(), ret.data_ptr()
    for n, t in outs.items():
        setattr(a, n, t.data_ptr())
    a.E, a.T, a.start, a.steps, a.origin, a.ep_len = B, 2, 0, 1, 0, 5
    a.eps, a.cost, a.inv_ep_len = math.inf, 0.01, 0.2
    assert G.lib().st_gru_rollout_launch(C.byref(a), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    q_learn = np.ascontiguousarray(Q.reshape(S + 1, B, 4)[0, :, :3])
    q_roll = outs["tr_q"].cpu().numpy()[:, 0]
    assert len(np.unique(q_roll)) > B and np.isfinite(q_roll).all()
    assert np.array_equal(q_learn.view(np.int32), q_roll.view(np.int32))
