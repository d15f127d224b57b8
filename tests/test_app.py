"""End-to-end ShareTradeHelper runs (CPU): price service -> router -> workers -> learner.

The MSFT series comes from ``config.default_csv_path()``: the reference checkout's CSV when present,
else the bundled parsed copy (``sharetrade/data/msft_prices.npz``), so these parity runs never skip.
The reference's CSV itself is stored as ``tests/golden/MSFT-stock-prices-revised.txt``: the bundled copy
is re-derived from it on every machine."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from sharetrade.config import BUNDLED_SERIES, default_csv_path, preset_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CSV = os.path.join(ROOT, "tests", "golden", "MSFT-stock-prices-revised.txt")


def _cfg(max_ok=True):
    cfg = preset_config("test")
    cfg.router.poll_interval_s = 0.1
    cfg.env.progress_every = 0
    return cfg


def test_bundled_series_is_the_reference_csv():
    """The bundled series is exactly what the CSV parser keeps from the reference's file."""
    from sharetrade.data.prices import load_csv

    z = np.load(BUNDLED_SERIES)
    assert len(z["days"]) == 6047 and np.all(np.diff(z["days"]) > 0)
    ref = load_csv(GOLDEN_CSV)
    dates = sorted(ref)
    assert [d.toordinal() for d in dates] == z["days"].tolist()
    assert np.array_equal(np.asarray([ref[d] for d in dates]), z["prices"])
    import hashlib

    assert hashlib.sha256(open(GOLDEN_CSV, "rb").read()).hexdigest() == str(z["source_sha256"])


@pytest.mark.parametrize("engine", ["actors", "vector"])
def test_compat_run_reproduces_reference_avg_std(engine):
    """Reference semantics (quirk Q1): every worker ends at its initial budget -> 2400.0 / 0.0."""
    from sharetrade.app import run

    res = run(_cfg(), engine=engine, device="cpu", max_prices=260, quiet=True)
    assert res["completed"] == 1.0
    assert res["avg"] == 2400.0 and res["std"] == 0.0


def test_full_length_compat_run_vector_engine():
    """The reference's own run at full length (`ShareTradeHelper.scala:20-48`): 10 workers x the whole
    6,047-price MSFT series = 5,846 steps each (`TrainerChildActor.scala:64-71`), reference_compat
    semantics, vector engine on the CPU -> exactly avg 2400.0, std 0.0 (reward is identically 0 under
    quirk Q1, `TrainerChildActor.scala:118-123`)."""
    from sharetrade.app import run

    cfg = _cfg()
    cfg.router.poll_interval_s = 1.0     # 201 polls span 201 s: room for a loaded CPU (the run alone takes ~40 s)
    t0 = time.perf_counter()
    res = run(cfg, engine="vector", device="cpu", quiet=True)
    assert res["completed"] == 1.0, res
    assert res["avg"] == 2400.0 and res["std"] == 0.0, res
    assert time.perf_counter() - t0 < 600


@pytest.mark.slow
@pytest.mark.timeout(1200)
def test_full_length_compat_run_actors_engine():
    """Message-level parity at full length: the `actors` engine runs the reference app exactly as
    `ShareTradeHelper.scala:20-48` wires it -- 10 TrainerChildActor FSMs, each asking ONE shared
    QDecisionPolicyActor `SelectionAction` and `UpdateQ` per step (`TrainerChildActor.scala:87-102`), over
    the whole MSFT series (5,846 steps each: 116,920 round trips) -- and ends at exactly avg 2400.0,
    std 0.0 (quirk Q1)."""
    from sharetrade.app import run

    cfg = _cfg()
    cfg.router.poll_interval_s = 5.0     # the reference's own poll (ShareTradeHelper.scala:33): 201 polls span 1,005 s
    t0 = time.perf_counter()
    res = run(cfg, engine="actors", device="cpu", quiet=True)
    assert res["completed"] == 1.0, res
    assert res["avg"] == 2400.0 and res["std"] == 0.0, res
    assert time.perf_counter() - t0 < 1100


def test_intended_semantics_trade():
    from sharetrade.app import run

    cfg = preset_config("intended")
    cfg.persist.journal_plugin = "inmemory"
    cfg.router.poll_interval_s = 0.1
    cfg.env.progress_every = 0
    cfg.agent.ramp = 10.0
    res = run(cfg, engine="vector", device="cpu", max_prices=320, quiet=True)
    assert res["completed"] == 1.0
    assert res["avg"] != 2400.0        # the fixed env actually trades


def test_cli_config_and_engine():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "sharetrade", "config", "--preset", "flagship",
                          "--set", "model.hidden=[64,64]"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    cfg = json.loads(out.stdout)
    assert cfg["model"]["hidden"] == [64, 64] and cfg["agent"]["optimizer"] == "adam"
    out = subprocess.run([sys.executable, "-m", "sharetrade", "engine", "--preset", "intended", "--steps", "3",
                          "--envs", "4", "--device", "cpu", "--set", "data.source=random_walk",
                          "--set", "data.length=300"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["backend"] == "torch" and res["envs"] == 4


def test_config_file_roundtrip(tmp_path):
    from sharetrade.config import Config

    cfg = preset_config("flagship")
    p = tmp_path / "c.json"
    p.write_text(cfg.to_json())
    back = Config.load(str(p), "reference_compat")
    assert back.to_dict() == cfg.to_dict()
    t = tmp_path / "c.toml"
    t.write_text('[agent]\noptimizer = "sgd"\nlr = 0.5\n[model]\nhidden = [32]\n')
    c2 = Config.load(str(t))
    assert c2.agent.optimizer == "sgd" and c2.agent.lr == 0.5 and c2.model.hidden == [32]
    with pytest.raises(KeyError):
        cfg.override(["agent.nope=1"])
