#!/usr/bin/env python3
"""Record tests/golden/learner_driver_parent_seeded.npz, the fixture of
tests/test_gpu_learner_driver_golden.py (1x MI355X).

The fixture pins what ``capture(iters_per_graph=4); iterations(9); iteration(2)`` leaves behind in DeepDQN
(config 4) and RecurrentDQN (config 5) to what it left at commit 9a7cd56, the last one at which each learner
carried its own copy of the graph-replay driver.  It was recorded from a built checkout of that commit:

    git worktree add /tmp/parent 9a7cd56 && (cd /tmp/parent && python build.py)
    python tools/record_learner_driver_golden.py --root /tmp/parent tests/golden/learner_driver_parent_seeded.npz

``--root`` is the checkout whose package and kernels run (default: this one; recording from a later commit pins
that commit instead).  Only the learners' surface that is the same before and after the change is used.

The runs, at the small shapes of the k-graph tests in tests/test_gpu_deep.py and tests/test_gpu_gru.py, with
``agent.epsilon = 0`` (actions then come from the Philox draws alone, so env, replay and counters do not depend on
Q and are exact) and ``target_every = 6``: deep E = 256, B = 256, hidden [256, 256], replay capacity 1024, six
eager act steps; recurrent E = 256, S = 8, batch 256, 1024 replay segments, two eager actor launches; both
``overlap_act``.  The warm-up, 9 iterations and one 2-update iteration make 12 updates and 11 act steps: the
warm-up (update 1), a 4-iteration graph (2..5), a single iteration up to the target copy at 6, a second graph
(7..10), one overlapped iteration (11) and a plain update (12, the second target copy).

Stored per learner (keys ``deep_*`` / ``gru_*``): the counters (``updates``, ``acts``, and ``par``, the GRU's
current online weight set), every integer and exact-float tensor of ``state_dict()`` that
tests/test_gpu_learners_dp.py compares bit for bit (NaN as -7; without the GRU's large replay features ``rx``
and hidden states ``rh0``), and ``norm_<name>``, the float64 L2 norm of each parameter tensor (online and
target), which depend on the order of float atomics and are compared to rtol 1e-4.
"""
import argparse
import os
import sys

import numpy as np

TARGET_EVERY, K, N, LAST = 6, 4, 9, 2
# weight-dependent entries of state_dict() (reduction-order noise): by norm or not at all
DEEP_APPROX = ("W", "b", "Wm", "Wv", "bm", "bv", "Wt", "bt", "loss", "stats")
GRU_APPROX = ("flat", "mflat", "vflat", "tflat", "h", "rh0", "loss", "stats")
GRU_LARGE = ("rx",)


def _drive(d):
    import torch

    d.capture(iters_per_graph=K)
    d.iterations(N)
    d.iteration(LAST)
    torch.cuda.synchronize()


def _exact(st, skip, per_layer=False):
    out = {}
    for k, v in st.items():
        if (k.rstrip("0123456789") if per_layer else k) in skip:
            continue
        v = v.float().nan_to_num(-7.0) if v.is_floating_point() else v
        out[k] = v.numpy()
    return out


def _norm(t) -> np.ndarray:
    return np.array(float(t.detach().double().norm().cpu()))


def make_deep():
    import torch

    from sharetrade.config import preset_config
    from sharetrade.data.prices import random_walk
    from sharetrade.trainer.deep import DeepDQN

    cfg = preset_config("flagship")
    cfg.model.hidden = [256, 256]
    cfg.agent.lr, cfg.agent.epsilon, cfg.agent.ramp = 1e-4, 0.0, 2.0
    E = 256
    prices = torch.from_numpy(random_walk(400, 50.0, 0.02, 4, n_series=E).astype(np.float32))
    d = DeepDQN(cfg, torch.device("cuda", 0), envs=E, batch=256, replay_capacity=1024, prices=prices,
                dw_gemm="hip", overlap_act=True, target_every=TARGET_EVERY)
    for _ in range(6):
        d.act_step()
    return d


def run_deep():
    d = make_deep()
    _drive(d)
    rec = _exact(d.state_dict(), DEEP_APPROX, per_layer=True)
    rec.update(updates=np.array(d.updates), acts=np.array(d.env_steps), par=np.array(0))
    for l in range(d.L):
        for name, lst in (("W", d.W), ("b", d.b), ("Wt", d.Wt), ("bt", d.bt)):
            rec[f"norm_{name}{l}"] = _norm(lst[l])
    return rec


def make_gru():
    import torch

    from sharetrade.config import preset_config
    from sharetrade.trainer.recurrent import RecurrentDQN

    cfg = preset_config("recurrent")
    cfg.agent.epsilon = 0.0
    d = RecurrentDQN(cfg, torch.device("cuda", 0), envs=256, seq=8, batch=256, bars=600, ep_len=5,
                     replay_segments=1024, burn_in=1, overlap_act=True)
    d.target_every = TARGET_EVERY
    for _ in range(2):
        d.act()
    return d


def run_gru():
    d = make_gru()
    _drive(d)
    rec = _exact(d.state_dict(), GRU_APPROX + GRU_LARGE)
    rec.update(updates=np.array(d.updates), acts=np.array(d.launches), par=np.array(d._par))
    for name in d.P:
        rec[f"norm_{name}"], rec[f"norm_t_{name}"] = _norm(d.P[name]), _norm(d.T_P[name])
    return rec


def run_cases():
    """{"deep_<key>" / "gru_<key>": array} of both runs."""
    out = {}
    for pre, fn in (("deep", run_deep), ("gru", run_gru)):
        out.update({f"{pre}_{k}": np.asarray(v) for k, v in fn().items()})
    return out


def is_exact(key: str) -> bool:
    return "_norm_" not in key


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import sharetrade
    assert os.path.abspath(sharetrade.__file__).startswith(root + os.sep), sharetrade.__file__

    rec = run_cases()
    for k, v in rec.items():
        print(k, v.dtype, v.shape, v if v.ndim == 0 else "")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
