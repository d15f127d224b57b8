"""The ws step kernel's latency items (csrc/qstep_ws.hip: WS_L2NPRE, WS_GW1PRE, WS_TICK_RCP, WS_EARLY_LOADS) change
when work is issued, never what is computed.

* Bit-identity with the kernel before them: ``tests/golden/ws_latency_{tick,f32}.npz`` hold what that kernel
  computed in 6 eager flagship steps -- parameters, budget, shares, value, position, actions, rewards and the
  statistics accumulator -- on the 16-bit tick bank and on fp32 windows, at 192 envs on grid 2 (uneven rounds: 2
  chunks and 1 chunk per workgroup, so the loop, the last tile and the values carried over the back edge all run)
  and at 64 envs on grid 1 (one tile per data wave, one slot pair: the prologue order and the pre-reads have no
  steady state to hide in).  The fixtures were written by ``python tests/test_gpu_ws_latency_items.py DIR`` on
  that kernel.  This build must reproduce every bit.
* The tick reciprocal (csrc/qstep.h ``tick_rcp``) equals the IEEE division 1 / x for every tick 1 .. 65,535.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(192, 2), (64, 1)]
STEPS = 6
KEYS = ("params", "budget", "shares", "value", "pos", "actions", "rewards", "stat_acc")


def _run(E, grid, tick16):
    from sharetrade.config import preset_config
    from sharetrade.data.prices import random_walk, tick16_quantize
    from sharetrade.trainer.engine import VectorEngine

    cfg = preset_config("flagship")
    cfg.engine.step_kernel = "ws"
    cfg.engine.step_variant = os.environ.get("SHARETRADE_WS_VARIANT", "")
    cfg.engine.grid = grid
    cfg.agent.epsilon = 0.5
    p = random_walk(400, 50.0, 0.02, 17, n_series=E).astype(np.float32)
    prices = torch.from_numpy(tick16_quantize(p) if tick16 else p)
    dev = torch.device("cuda", 0)
    eng = VectorEngine(cfg, prices=prices, device=dev, envs=E)
    assert eng.step_kernel == "ws" and eng.grid == grid
    assert (eng.ticks is not None) == tick16 and (eng.prices4 is None) == tick16
    # odd and even window starts in every tile; some envs finish their episode (T - H = 199) inside the 6 steps
    eng.state.pos.copy_(torch.arange(E, dtype=torch.int32, device=dev) * 7 % 198)
    eng.state.shares.copy_(torch.arange(E, dtype=torch.int32, device=dev) % 3)
    for _ in range(STEPS):
        eng.step()
        torch.cuda.synchronize()
        eng.check_kernel_err()
    out = {"params": eng.params.detach(), "budget": eng.state.budget, "shares": eng.state.shares,
           "value": eng.state.value, "pos": eng.state.pos, "actions": eng.actions_out, "rewards": eng.rewards_out,
           "stat_acc": eng.stat_acc}
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.mark.parametrize("E,grid", SHAPES)
@pytest.mark.parametrize("bank", ["tick", "f32"])
def test_ws_bit_identical_to_kernel_before_latency_items(native_built, bank, E, grid):
    gold = np.load(os.path.join(GOLDEN, f"ws_latency_{bank}.npz"))
    got = _run(E, grid, bank == "tick")
    for k in KEYS:
        want = gold[f"E{E}_g{grid}_{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        diff = int((_bits(got[k]) != _bits(want)).sum())
        print(f"[meas] ws latency items bank={bank} E={E} grid={grid} {k}: {diff} of {want.size} words differ")
        assert diff == 0, (bank, E, grid, k, diff)
    assert int((gold[f"E{E}_g{grid}_pos"] & 1).sum()) > 0, "no window starts at an odd tick"


def test_tick_rcp_equals_ieee_division_for_every_tick(native_built):
    """csrc/diag.hip tick_rcp_table: the bits of __fdiv_rn(1, x) and of tick_rcp(x) for x = 1 .. 65,535."""
    div, rcp = native_built.tick_rcp_table(torch.device("cuda", 0))
    div, rcp = div.cpu().numpy().view(np.uint32), rcp.cpu().numpy().view(np.uint32)
    assert div.shape == rcp.shape == (65535,)
    x = np.arange(1, 65536, dtype=np.float64)
    assert np.array_equal(div, (1.0 / x).astype(np.float32).view(np.uint32)), "the division itself is not 1 / x"
    bad = np.nonzero(div != rcp)[0]
    print(f"[meas] tick_rcp: {bad.size} of 65535 ticks differ from the IEEE division" +
          (f", first x = {int(bad[0]) + 1}" if bad.size else ""))
    assert bad.size == 0, (bad[:8] + 1).tolist()


if __name__ == "__main__":   # write the fixtures (run on the kernel the later builds have to reproduce)
    out_dir = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.makedirs(out_dir, exist_ok=True)
    for bank in ("tick", "f32"):
        arrs = {}
        for E, grid in SHAPES:
            for k, v in _run(E, grid, bank == "tick").items():
                arrs[f"E{E}_g{grid}_{k}"] = v
        np.savez_compressed(os.path.join(out_dir, f"ws_latency_{bank}.npz"), **arrs)
        print(bank, {k: (v.dtype.str, v.shape) for k, v in arrs.items()})
