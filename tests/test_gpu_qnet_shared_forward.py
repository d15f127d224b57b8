"""The 2x128 Q-net forward of the serve and backtest kernels against recorded outputs of the kernels before
they shared one definition of it.

``tests/test_gpu_serve.py`` and ``tests/test_gpu_backtest.py`` compare each kernel with a PyTorch oracle at 2e-3;
an error in the shared forward (``csrc/qnet_*.h``) that stayed under that tolerance would pass both.  This test
pins every output bit of both kernels to ``tests/golden/qnet_forward_parent_seeded.npz``: recorded once on an
MI355X from this project's own commit f2f298c (the last one where ``csrc/qserve.hip`` and ``csrc/qrollout.hip``
each carried a copy of the forward) by ``tools/record_qnet_forward_golden.py``, which runs :func:`run_cases` of
this file on that commit's kernels.  The fixture holds the inputs too (request rows, steps, prices); the weights
are the NumPy-mirror ``init_params`` of seed 3, the same on every machine.

Cases (:func:`run_cases`): serve at 130 rows with ``grid=2`` (three 64-row tiles, one workgroup walks tiles 0 and
2, the last with 2 live rows) from a stride-204 buffer (STREAM build, one m-tile per wave) and a stride-203 buffer
(register gather, two m-tiles per wave), greedy and epsilon-greedy, plus stride 204 with raw features and the
output ReLU; the rollout at 40 envs with ``grid=1`` (two 32-env tiles, the second with 8 live envs), ``start=5``,
``day_block() + 3`` days (two price blocks, the last partial), traced: greedy, epsilon-greedy, raw + output ReLU.

Every greedy run must take all three actions, so that the argmax is exercised.  The raw nets of this seed hold on
every row (b2 = 0.1 dominates W2 h at ``init_std`` 0.01, and W2 h is negative for all three actions on these
inputs), so the raw cases scale the three action rows of W2 by ``RAW_W2_SCALE``: negative factors lift every output
above the output ReLU's clamp (no row of either raw run is (0, 0, 0)), and their ratio spreads the argmax over Buy,
Sell and Hold in the serve run and in the rollout.
"""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qnet_forward_parent_seeded.npz")
H, SEED = 201, 3
B, E, START = 130, 40, 5
BUDGET = 120.0          # the rollout's (tests/test_gpu_backtest.py); serve keeps the preset's
RAW_W2_SCALE = (-1.0, -3.0, -10.0)   # W2 rows of Buy, Sell, Hold
# (name, features, output_relu, row stride, epsilon-greedy)
SERVE_CASES = [("sv204_greedy", "relative", False, 204, False), ("sv204_eps", "relative", False, 204, True),
               ("sv203_greedy", "relative", False, 203, False), ("sv203_eps", "relative", False, 203, True),
               ("sv204_raw_greedy", "raw", True, 204, False)]
# (name, features, output_relu, greedy)
ROLLOUT_CASES = [("ro_greedy", "relative", False, True), ("ro_eps", "relative", False, False),
                 ("ro_raw_greedy", "raw", True, True)]
ROLLOUT_FIELDS = ("budget", "shares", "portfolio", "buys", "sells", "actions", "q", "equity")


def _weights(features, output_relu, budget=None):
    from sharetrade.config import preset_config
    from sharetrade.models import qnet as qn

    cfg = preset_config("flagship")
    cfg.env.features, cfg.model.output_relu = features, output_relu
    if budget is not None:
        cfg.env.budget = budget
    if features == "raw":
        cfg.model.init_std, cfg.model.init = 0.01, "normal"
    layout = qn.QNetLayout.from_config(cfg.model)
    w = qn.init_params(layout, cfg.model, seed=SEED, host_mirror=True)
    if features == "raw":
        layout.w(w, 2)[:3] *= torch.tensor(RAW_W2_SCALE)[:, None]
    dev = w.cuda()
    return cfg, layout, dev, dev.to(torch.bfloat16)


def run_cases(rows, steps, prices):
    """Every case on the GPU: ``rows`` [B, 203], ``steps`` [B], ``prices`` [E, >= START + days + H] fp32 host
    tensors -> {"<case>_<output>": host array}."""
    from sharetrade.env import trading as tr
    from sharetrade.serve.kernel import ServeKernel
    from sharetrade.serve.rollout import RolloutKernel, day_block
    from sharetrade.utils import rng

    out = {}
    key = rng.key_for(SEED, 0)
    for name, features, relu, ld, eps in SERVE_CASES:
        cfg, layout, w, wbf = _weights(features, relu)
        kern = ServeKernel(layout, w, wbf, history=H, feat_mode=tr.FEATURES[features], output_relu=relu,
                           budget0=cfg.env.budget, epsilon=cfg.agent.epsilon, ramp=cfg.agent.ramp, key=key)
        buf = torch.zeros(B, ld, device="cuda")
        buf[:, : H + 2] = rows.cuda()
        x = buf[:, : H + 2]
        assert x.stride(0) == ld and x.data_ptr() % 16 == 0
        acts = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        q = torch.zeros(B, 3, device="cuda")
        kern.launch(x, acts, q, steps.cuda() if eps else None, seq=1 if eps else 0, grid=2)
        torch.cuda.synchronize()
        out[name + "_actions"], out[name + "_q"] = acts.cpu().numpy(), q.cpu().numpy()
    days = day_block() + 3
    assert prices.shape == (E, START + days + H)
    P = prices.cuda()
    for name, features, relu, greedy in ROLLOUT_CASES:
        cfg, layout, w, wbf = _weights(features, relu, BUDGET)
        kern = RolloutKernel(layout, w, wbf, history=H, feat_mode=tr.FEATURES[features], output_relu=relu,
                             budget0=BUDGET, shares0=cfg.env.shares, compat=False, epsilon=0.9, ramp=4.0, key=key)
        res = kern.run(P, start=START, steps=days, greedy=greedy, trace=True, env_offset=0 if greedy else 7, grid=1)
        torch.cuda.synchronize()
        for k in ROLLOUT_FIELDS:
            out[f"{name}_{k}"] = res[k].cpu().numpy()
    return out


def _bits(x):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return t.view(torch.int32) if t.is_floating_point() else t


@pytest.mark.gpu
def test_serve_and_rollout_equal_the_recorded_parent(native_built):
    g = np.load(GOLDEN)
    for name, features, *_ in SERVE_CASES + ROLLOUT_CASES:
        if "greedy" in name:
            assert set(g[name + "_actions"].flatten().tolist()) == {0, 1, 2}, name
    got = run_cases(torch.from_numpy(g["in_rows"]), torch.from_numpy(g["in_steps"]), torch.from_numpy(g["in_prices"]))
    keys = sorted(k for k in g.files if not k.startswith("in_"))
    assert keys == sorted(got)
    for k in keys:
        assert got[k].dtype == g[k].dtype and got[k].shape == g[k].shape, k
        assert torch.equal(_bits(got[k]), _bits(g[k])), k
