#!/usr/bin/env python3
"""Record tests/golden/gru_bar_parent_seeded.npz, the fixture of tests/test_gpu_gru_shared_bar.py (1x MI355X).

The fixture pins the GRU(256) bar to what the kernels computed at commit f5527cf, the last one at which each of
the four kernels carried its own copy of the bar.  It was recorded from a built checkout of that commit:

    git worktree add /tmp/parent f5527cf && (cd /tmp/parent && python build.py)
    python tools/record_gru_bar_golden.py --root /tmp/parent tests/golden/gru_bar_parent_seeded.npz

``--root`` is the checkout whose package and kernels run (default: this one; recording from a later commit pins
that commit instead).  What is stored:

* ``ro_*``: a greedy 96-env, 9-bar rollout with ``ep_len`` 7 (three chunks, an episode end inside the run) of
  ``gru_backtest_refs.centred_params(3, 96, 9, 7)`` on the first 11 bars of ``gru_backtest_refs.bars(96, 17)``.
  Inputs kept: the bars and ``b_q`` (the rest of the weights is ``init_params(3)`` with ``w_q`` x 30).  Outputs:
  ``ret``, ``position``, actions, and of ``h`` every 16th env's row and the SHA-256 of the whole array's bytes;
* ``act_*``: one pair-actor launch at 96 envs, S = 4, of a ``RecurrentDQN`` (Q head x 30, epsilon 0.9, launch
  counter 1 = past the 1-step ramp): ``ep_ret``, ``position``, ``q_out``, ``h`` as above, and ``act_in_sum``, sums of
  the GPU-generated inputs (bank, weights, bar positions after the launch).
"""
import argparse
import hashlib
import os
import sys

import numpy as np

E, STEPS, EP_LEN, T = 96, 9, 7, 11
H_ROWS = slice(0, None, 16)


def sha(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch

    import gru_backtest_refs as R
    import sharetrade
    assert os.path.abspath(sharetrade.__file__).startswith(root), sharetrade.__file__
    from sharetrade.config import preset_config
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.trainer.recurrent import RecurrentDQN

    dev = torch.device("cuda", 0)
    rec = {}
    close, feat = R.bars(E, STEPS + 8)
    close, feat = close[:, :T].contiguous(), feat[:, :T].contiguous()
    params = R.centred_params(3, E, STEPS, EP_LEN)
    res = GruPolicy(params, device=dev, seed=3).backtest(close.cuda(), feat.cuda(), steps=STEPS, ep_len=EP_LEN,
                                                         trace=True)
    torch.cuda.synchronize()
    rec["ro_close"], rec["ro_feat"] = close.numpy(), feat.view(torch.int16).numpy()
    rec["ro_b_q"] = params["b_q"].numpy()
    h = res.h.cpu().numpy()
    rec["ro_ret"], rec["ro_position"] = res.ret.cpu().numpy(), res.position.cpu().numpy()
    rec["ro_actions"], rec["ro_h_rows"], rec["ro_h_sha256"] = res.actions.cpu().numpy(), h[H_ROWS].copy(), sha(h)
    print("rollout action shares", R.action_shares(res.actions.cpu()), "trades", int(res.trades.sum()))

    cfg = preset_config("recurrent")
    cfg.agent.epsilon, cfg.agent.ramp = 0.9, 1.0
    d = RecurrentDQN(cfg, dev, envs=E, seq=4, burn_in=1, bars=600, ep_len=5, batch=128, replay_segments=1024,
                     actor_kernel="pair")
    d.P["w_q"].mul_(30.0)
    d.pack("on", into=0)
    d.pack("on", into=1)
    d.ctrl.fill_(1)
    q_out = torch.zeros(d.E, 4, device="cuda")
    d._act.q_out = q_out.data_ptr()
    d.act()
    torch.cuda.synchronize()
    h = d.h.cpu().numpy()
    rec["act_h_rows"], rec["act_h_sha256"] = h[H_ROWS].copy(), sha(h)
    rec["act_ep_ret"], rec["act_position"] = d.ep_ret.cpu().numpy(), d.position.cpu().numpy()
    rec["act_q_out"] = q_out.cpu().numpy()
    rec["act_in_sum"] = np.array([float(t.double().sum()) for t in (d.close, d.feat, d.flat, d.pos)])
    print("actor: positions", int(d.position.sum()), "actions", sorted(set(q_out[:, 3].cpu().long().tolist())))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
