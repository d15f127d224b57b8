"""bench.py driver contract on one GPU: one JSON line with the required keys, whole-job value =
envs x steps / elapsed, and the flagship config it claims (BASELINE.json metric)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract(native_built):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--envs", "8192", "--steps", "40",
                          "--warmup", "4", "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"]
    for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 4 and d["dtype"] == "bf16"
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    c = d["config"]
    assert c["global_batch"] == 8192 and c["parallelism"] == "dp1" and c["seq_len"] == 201
    # value is the whole-job rate implied by ms_per_step
    assert abs(d["value"] - 8192 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    # the untimed evaluations: the plain learner's episodes and the stabilised learner's greedy episode
    er = d["episode_return"]
    for k in ("greedy_median", "random_median", "buy_hold_median"):
        assert k in er, k
    sl = er["stable_learner"]
    assert "error" not in sl, sl
    # trained for as many steps as the plain learner before its evaluation (graph priming + warm-up + timed)
    assert sl["preset"] == "flagship_stable" and 44 <= sl["train_steps"] <= d["graph_prime_steps"] + 44 + 64
    assert "greedy_median" in sl


def test_plain_run_is_lean_and_dumps_outputs(native_built, tmp_path):
    """Without --full the bench only times its steps: no evaluation blocks in the result line.  --dump-outputs
    writes what the last timed step computed, float32 / float64, within the 64 MB budget."""
    import numpy as np

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "8192", "--steps", "21",
                          "--warmup", "3", "--dump-outputs", str(tmp_path / "o")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 21 and d["warmup"] == 3 and d["ms_per_step"] > 0 and d["dtype"] == "bf16"
    assert d["unit"] == "env_steps/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 8192 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    assert "episode_return" not in d and "allreduce_ms_per_step" not in d
    arrs = {f[:-4]: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert set(arrs) == {"params", "actions", "rewards", "budget", "shares", "value", "portfolios", "stat_acc"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64_000_000
    for k in ("actions", "rewards", "budget", "shares", "value", "portfolios"):
        assert arrs[k].shape == (8192,) and np.isfinite(arrs[k]).all(), k
    assert set(np.unique(arrs["actions"])) <= {0.0, 1.0, 2.0}
    assert np.allclose(arrs["portfolios"], arrs["budget"] + arrs["shares"] * arrs["value"], rtol=1e-6)
    assert np.isfinite(arrs["params"]).all() and np.abs(arrs["params"]).max() > 0
