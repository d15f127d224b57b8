#!/usr/bin/env python3
"""Does the config-5 learner learn?  GRU(256) DQN on synthetic minute bars (AR(1) + GARCH returns,
trading cost per position change): the trained run vs the same run with a frozen random network
(lr = 0; identical envs, draws and epsilon schedule), reward per env-step over windows of
iterations.  Prints a markdown table (GPU).  ``--heldout`` adds, per window, the greedy return of the frozen
current net per full episode on held-out bars (``RecurrentDQN.backtest``: one rollout launch, learner state
untouched), trained vs frozen."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def curve(lr: float, iters: int, window: int, envs: int, seed: int, heldout: int = 0):
    from sharetrade.config import preset_config
    from sharetrade.trainer.recurrent import RecurrentDQN

    cfg = preset_config("recurrent")
    d = RecurrentDQN(cfg, torch.device("cuda", 0), envs=envs, lr=lr, seed=seed, overlap_act=True)
    out = []
    prev_r, prev_steps, prev_ep, prev_fin = 0.0, 0, 0.0, 0.0
    d.capture()
    done = 1
    while done < iters:
        d.iteration(1)
        done += 1
        if done % window == 0:
            st = d.stats.detach().cpu().numpy().astype(np.float64)
            steps = d.env_steps
            r = (st[0] - prev_r) / max(1, steps - prev_steps)
            ep = st[2] - prev_ep
            ret = (st[3] - prev_fin) / ep if ep > 0 else float("nan")
            held = d.backtest(envs=heldout).summary()["per_episode"] if heldout else float("nan")
            out.append((done, r, ret, 1.0 - (st[1] - 0) / max(1, steps), held))
            prev_r, prev_steps, prev_ep, prev_fin = st[0], steps, st[2], st[3]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--window", type=int, default=250)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--heldout", action="store_true",
                    help="add the greedy held-out return per episode of the current net (trained vs frozen)")
    ap.add_argument("--heldout-envs", type=int, default=4096)
    a = ap.parse_args()
    import build

    build.build_all()
    held = a.heldout_envs if a.heldout else 0
    learned = curve(3e-4, a.iters, a.window, a.envs, a.seed, held)
    frozen = curve(0.0, a.iters, a.window, a.envs, a.seed, held)
    lines = ["# Config 5 learning check: GRU(256) DQN on AR(1)+GARCH minute bars (1x MI355X)", "",
             f"{a.envs} envs x 16 bars per iteration, one update (1,024 segments) per iteration; the frozen run "
             "has lr = 0 (random-init network, same envs / draws / epsilon schedule).", "",
             "| iterations | reward / env-step (trained) | reward / env-step (frozen) | episode return (trained) | "
             "episode return (frozen) |", "|---|---|---|---|---|"]
    if a.heldout:
        lines[2] += (f"  Held-out: the net after the window's last iteration, greedy, over 4 episodes of "
                     f"{a.heldout_envs} series the run never saw (return per episode).")
        lines[-2] += " greedy held-out return (trained) | greedy held-out return (frozen) |"
        lines[-1] += "---|---|"
    for (i, r1, e1, _, h1), (_, r2, e2, _, h2) in zip(learned, frozen):
        row = f"| {i - a.window + 1}-{i} | {r1:.3e} | {r2:.3e} | {e1:.4f} | {e2:.4f} |"
        lines.append(row + (f" {h1:.4f} | {h2:.4f} |" if a.heldout else ""))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
