#!/usr/bin/env python3
"""Record tests/golden/qnet_forward_parent_seeded.npz, the fixture of tests/test_gpu_qnet_shared_forward.py
(1x MI355X).

The fixture pins the serve and backtest kernels of the 2x128 Q-net to what they computed at commit f2f298c, the
last one at which ``csrc/qserve.hip`` and ``csrc/qrollout.hip`` each carried a copy of the forward.  It was
recorded from a built checkout of that commit:

    git worktree add /tmp/parent f2f298c && (cd /tmp/parent && python build.py)
    python tools/record_qnet_forward_golden.py --root /tmp/parent tests/golden/qnet_forward_parent_seeded.npz

``--root`` is the checkout whose package and kernels run (default: this one; recording from a later commit pins
that commit instead).  The cases are ``run_cases`` of this checkout's test file, whatever ``--root`` is; its
docstring describes them.  What is stored:

* ``in_rows`` [130, 203]: request rows as ``tests/test_gpu_serve.py::_rows(130)``; ``in_steps`` [130]: the
  epsilon-greedy runs' steps, uniform in 0 .. 2000; ``in_prices`` [40, 241]: series as
  ``tests/test_gpu_backtest.py::_prices(40, day_block() + 3, extra=5)``;
* ``sv*_actions`` / ``sv*_q``: the five serve runs; ``ro*_<field>``: the five per-env fields and the three traces
  of the three rollouts.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, root)
    import torch

    import sharetrade
    assert os.path.abspath(sharetrade.__file__).startswith(root + os.sep), sharetrade.__file__
    import test_gpu_backtest as tb
    import test_gpu_qnet_shared_forward as T
    import test_gpu_serve as ts
    from sharetrade.serve.rollout import day_block

    rows = ts._rows(T.B)
    steps = torch.from_numpy(np.random.default_rng(T.B).uniform(0, 2000, size=T.B).astype(np.float32))
    prices = tb._prices(T.E, day_block() + 3, extra=T.START)
    rec = {"in_rows": rows.numpy(), "in_steps": steps.numpy(), "in_prices": prices.numpy()}
    rec.update(T.run_cases(rows, steps, prices))
    for k in sorted(rec):
        if k.endswith("_actions"):
            print(k, np.bincount(rec[k].flatten().astype(np.int64), minlength=3).tolist())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
