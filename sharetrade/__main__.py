"""Command line: ``python -m sharetrade <command>``.

Commands
--------
``train``   run the ShareTradeHelper application (`ShareTradeHelper.scala`):
            price service -> router -> workers -> learner; prints avg/std.
``engine``  run the vectorised engine directly for N steps and print metrics.
``deep``    train the 4x1024-MLP replay DQN (BASELINE config 4) for N iterations.
``recurrent`` train the GRU(256) minute-bar DQN (BASELINE config 5) for N iterations; with ``--bars-file F`` on the
            first ``--train-frac`` of every series of a file of raw OHLCV minute bars (``data.ohlcv``).
``serve``   serve SelectionAction over HTTP from the batched GPU kernel (weights from an
            engine checkpoint or random init).  With a checkpoint of a ``recurrent`` run (or ``--policy gru``):
            stateful GRU(256) sessions, one minute bar per request (``/session`` routes).
``backtest`` what a policy (engine checkpoint or random init) would have done over a price history: a CSV
            series or N synthetic ones, one rollout launch; prints policy vs buy-and-hold vs uniform random.
            With a checkpoint of a ``recurrent`` run (or ``--policy gru``): the GRU(256) policy, greedy, on N
            held-out synthetic minute-bar series, or (``--bars-file F [--held-out]``) on the raw OHLCV minute bars of
            a file; prints policy vs always-long vs uniform random vs flat.
``config``  print the resolved configuration (JSON).

Common flags: ``--preset {reference_compat,intended,flagship,flagship_stable,test}``,
``--config file.{json,toml}``, ``--set section.key=value`` (repeatable).
"""
from __future__ import annotations

import argparse
import json
import logging
import sys

from .config import Config, preset_config


def _cfg(a) -> Config:
    cfg = Config.load(a.config, a.preset) if a.config else preset_config(a.preset)
    if a.set:
        cfg.override(a.set)
    return cfg


def _backtest(a, cfg: Config) -> dict:
    """``backtest``: the policy, buy-and-hold (Buy at every step, as benchkit.buy_and_hold_returns) and a uniform
    random policy over the same series, each as mean / std / median of final portfolio - budget and trade counts.
    ``--report`` adds the risk report of each (drawdown, Sharpe, position, action mix, exposure / timing split,
    position / price correlation and portfolio figures: ``BacktestResult.report``), ``--curve-out`` saves the
    policy's portfolio curve; the policy's ledger rides along in its one launch."""
    import os

    import numpy as np
    import torch

    from .data import prices as dp
    from .serve import PolicyServer
    from .serve.http import load_checkpoint_params
    from .serve.rollout import ledger_from_trace, result_from, simulate_actions
    from .trainer.engine import resolve_device

    if a.csv:
        _, series = dp.sorted_series(dp.load_csv(a.csv))
        P = series[None, :]
    else:
        d = cfg.data
        P = dp.random_walk(d.length, d.start_price, d.volatility, d.seed, n_series=a.synthetic)
    P = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float32))
    params = load_checkpoint_params(a.ckpt, averaged=a.weights == "average") if a.ckpt else None
    srv = PolicyServer(cfg, params=params, device=resolve_device(a.device))
    res = srv.backtest(P, trace=bool(a.trace_out), ledger=bool(a.report or a.curve_out))
    e, H = cfg.env, cfg.model.history
    steps = res.steps
    g = torch.Generator().manual_seed(int(cfg.agent.seed))
    base, reports = {}, ({"policy": res.report()} if a.report else {})
    for name, acts in (("buy_and_hold", torch.zeros(P.shape[0], steps, dtype=torch.int8)),
                       ("uniform_random", torch.randint(0, 3, (P.shape[0], steps), generator=g).to(torch.int8))):
        out = simulate_actions(P, acts, history=H, budget0=e.budget, shares0=e.shares, compat=e.compat_decisions)
        base[name] = result_from(out, e.budget, 0, steps, False).summary()
        if a.report:
            led = ledger_from_trace(P, acts, history=H, budget0=e.budget, shares0=e.shares)
            reports[name] = result_from(out, e.budget, 0, steps, False, led).report()
    if a.trace_out:
        os.makedirs(a.trace_out, exist_ok=True)
        np.save(os.path.join(a.trace_out, "actions.npy"), res.actions.cpu().numpy())
        np.save(os.path.join(a.trace_out, "equity.npy"), res.equity.cpu().numpy())
    if a.curve_out:
        np.save(a.curve_out, res.ledger.curve.cpu().numpy())
    out = {"series": int(P.shape[0]), "days": int(P.shape[1]), "steps": int(steps), "budget": float(e.budget),
           "backend": srv.backend, "weights": (a.weights if a.ckpt else "init"), "policy": res.summary(), **base}
    for name, rep in reports.items():   # (--report: a `report` block in the policy's and every baseline's entry)
        out[name] = {**out[name], "report": rep}
    return out


def _gru_path(a) -> bool:
    """``backtest`` and ``serve`` take the GRU path with ``--policy gru`` or (``--policy auto``) a ``recurrent``
    checkpoint."""
    if a.policy != "auto":
        return a.policy == "gru"
    if not a.ckpt:
        return False
    from .serve.gru_rollout import checkpoint_kind

    return checkpoint_kind(a.ckpt) == "recurrent"


def _first_session(bars) -> int:
    """Bars of the first session of series 0 (to the first later bar with minute 0)."""
    N, T = bars.shape
    if bars.minute is None:
        return T
    import numpy as np

    m = np.asarray(bars.minute)
    m = m[0] if m.ndim == 2 else m
    later = np.nonzero(m[1:] == 0)[0]
    return int(later[0]) + 1 if later.size else T


def _file_bars(a, dev, meta):
    """``--bars-file``: the file's bars featurised with the checkpoint's parameters (``meta["bar_features"]``), or
    with ones fitted on the file's first session.  Returns (close, feat, info)."""
    import numpy as np
    import torch

    from .data import ohlcv as ov

    bars = ov.load_bars(a.bars_file)
    N, T = bars.shape
    bf = (meta or {}).get("bar_features")
    if bf:
        fp = ov.FeatureParams.from_meta(bf)
        if fp.sigma.shape[0] != N:
            raise ValueError(f"the checkpoint holds feature parameters of {fp.sigma.shape[0]} series, "
                             f"{a.bars_file} has {N}")
        source = "checkpoint"
    else:
        upto = _first_session(bars)
        fp = ov.fit_feature_params(bars, upto=upto)
        source = "first_session"
        print(f"warning: no feature parameters in a checkpoint; fitted on the first {upto} bars of {a.bars_file}",
              file=sys.stderr)
    start = 0
    if a.held_out:
        frac = float(bf["train_frac"]) if bf else float(a.train_frac)
        start = int(T * frac)
        if T - start < 2:
            raise ValueError(f"no held-out bars after train_frac={frac}")
    # the filter runs from the first bar on, so the held-out part starts with the state the training part left
    if dev.type == "cuda":
        r = ov.featurise_gpu(bars, fp, dev)
        close, feat = r.close[:, start:].contiguous(), r.feat[:, start:].contiguous()
    else:
        r = ov.featurise_numpy(bars, fp)
        close = torch.from_numpy(np.ascontiguousarray(r.close[:, start:]))
        feat = torch.from_numpy(np.ascontiguousarray(r.feat[:, start:])).to(torch.bfloat16)
    return close, feat, {"bars_file": a.bars_file, "held_out": bool(a.held_out), "first_bar": start,
                         "feature_params": source}


def _recurrent_bank(a, cfg: Config, ctx, kw: dict) -> dict:
    """``recurrent --bars-file``: featurise the first ``--train-frac`` of every series with parameters fitted on
    that part, cut this rank's windows (``seed + rank``) into ``kw["bank"]``; returns the checkpoint meta entry."""
    from .data import ohlcv as ov

    if not 0.0 < a.train_frac <= 1.0:
        raise ValueError("--train-frac must be in (0, 1]")
    bars = ov.load_bars(a.bars_file)
    N, T = bars.shape
    upto = int(T * a.train_frac)
    fp = ov.fit_feature_params(bars, upto=upto)
    r = ov.featurise_gpu(bars.piece(0, upto), fp, ctx.device)
    E = int(kw.get("envs", 65536))
    kw["bars"] = min(4096, upto)
    kw["bank"] = ov.window_bank(r.close, r.feat, E, kw["bars"], seed=int(cfg.agent.seed) + int(ctx.rank))
    return {"bar_features": {**fp.to_meta(bars.names_or_default()), "crc32c": ov.file_crc32c(a.bars_file),
                             "train_frac": float(a.train_frac), "file": a.bars_file}}


def _backtest_gru(a, cfg: Config) -> dict:
    """``backtest`` of a GRU(256) policy on N held-out synthetic minute-bar series (or the bars of ``--bars-file``):
    the greedy policy, always long (Buy on every bar), uniform random and flat, each as mean / std / median of the
    per-series return.  ``--report`` adds the risk report of each (drawdown, Sharpe, round trips, per-episode and
    portfolio figures: ``GruBacktestResult.report``), ``--curve-out`` saves the policy's portfolio curve."""
    import os

    import numpy as np
    import torch

    from .data import minute_bars as mb
    from .models import gru_qnet as gq
    from .serve.gru_rollout import GruPolicy, ledger_from_trace, result_from, simulate_minute_actions
    from .trainer.engine import resolve_device

    dev = resolve_device(a.device)
    if a.ckpt:
        pol = GruPolicy.from_checkpoint(a.ckpt, device=dev)
    else:
        pol = GruPolicy(gq.init_params(cfg.agent.seed), device=dev, seed=cfg.agent.seed)
    ep_len = int(a.ep_len)
    info = {}
    if a.bars_file:
        from .serve.gru_rollout import checkpoint_meta

        close, feat, info = _file_bars(a, dev, checkpoint_meta(a.ckpt) if a.ckpt else None)
        N, T = (int(v) for v in close.shape)
        bars_seed = None
    else:
        N = int(a.synthetic)
        T = int(a.bars) if a.bars else 4 * ep_len + 1
        bars_seed = pol.seed + 1000 if a.bars_seed is None else int(a.bars_seed)
        if dev.type == "cuda":
            close, feat = mb.generate_gpu(N, T, dev, seed=bars_seed)
        else:
            c, f = mb.generate_numpy(N, T, seed=bars_seed)
            close, feat = torch.from_numpy(c), torch.from_numpy(f).to(torch.bfloat16)
    kw = dict(ep_len=ep_len, cost=float(a.cost))
    led = bool(a.report or a.curve_out)   # the risk ledger rides along in the same launch
    res = pol.backtest(close, feat, trace=bool(a.trace_out), ledger=led, **kw)
    steps = res.steps
    rnd = pol.backtest(close, feat, greedy=False, epsilon=0.0, ledger=bool(a.report), **kw)
    base = {"uniform_random": rnd.summary()}
    reports = {"policy": res.report(), "uniform_random": rnd.report()} if a.report else {}
    for name, act in (("always_long", 0), ("flat", 1)):
        acts = torch.full((N, steps), act, dtype=torch.int8, device=close.device)
        out = simulate_minute_actions(close, acts, **kw)
        bl = ledger_from_trace(acts, out["reward"], start=0, origin=0, ep_len=ep_len) if a.report else None
        r = result_from(out, 0, steps, ep_len, 0, res.backend, False, bl)
        base[name] = r.summary()
        if a.report:
            reports[name] = r.report()
    if a.trace_out:
        os.makedirs(a.trace_out, exist_ok=True)
        np.save(os.path.join(a.trace_out, "actions.npy"), res.actions.cpu().numpy())
        np.save(os.path.join(a.trace_out, "reward.npy"), res.reward.cpu().numpy())
    if a.curve_out:
        np.save(a.curve_out, res.ledger.curve.cpu().numpy())
    return {"policy_kind": "gru", "series": N, "bars": T, "steps": int(steps), "ep_len": ep_len, "cost": float(a.cost),
            "bars_seed": bars_seed, "backend": res.backend, "weights": "checkpoint" if a.ckpt else "init",
            "policy": res.summary(), **base, **info, **({"report": reports} if a.report else {})}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="sharetrade")
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("train", "engine", "deep", "recurrent", "serve", "backtest", "config"):
        p = sub.add_parser(name)
        p.add_argument("--preset", default={"deep": "flagship", "recurrent": "recurrent",
                                            "serve": "flagship", "backtest": "flagship"}.get(name, "reference_compat"))
        p.add_argument("--config", default=None)
        p.add_argument("--set", action="append", default=[])
        if name == "train":
            p.add_argument("--engine", choices=["actors", "vector"], default="actors")
            p.add_argument("--device", default=None)
            p.add_argument("--max-prices", type=int, default=None, help="truncate the series (smoke runs)")
            p.add_argument("--gpus", type=int, default=1,
                           help="--engine vector: N > 1 makes the router's N routees the ranks of a data-parallel "
                                "group, one process per GPU (RCCL), with rank death -> replacement -> resume")
            p.add_argument("--envs-per-rank", type=int, default=None, help="envs of each rank (--gpus > 1)")
            p.add_argument("--dist-backend", default=None, help="nccl (= RCCL, GPUs) | gloo")
            p.add_argument("--ckpt-dir", default=None, help="--gpus > 1: sharded checkpoints of the episode")
            p.add_argument("--ckpt-every", type=int, default=0)
            p.add_argument("--same-device", action="store_true", help="--gpus > 1: every rank on cuda:0 (rehearsal)")
        if name == "engine":
            p.add_argument("--steps", type=int, default=100)
            p.add_argument("--envs", type=int, default=None)
            p.add_argument("--device", default="auto")
            p.add_argument("--metrics", default=None, help="JSONL metrics output path")
            p.add_argument("--log-every", type=int, default=100)
            p.add_argument("--ckpt-dir", default=None)
            p.add_argument("--ckpt-every", type=int, default=0)
            p.add_argument("--resume", action="store_true")
            p.add_argument("--trace", default=None, help="Chrome trace output path (torch.profiler)")
            p.add_argument("--no-graph", action="store_true")
        if name in ("engine", "deep", "recurrent"):
            p.add_argument("--elastic", type=int, default=0,
                           help="N > 0: run N rank processes under the elastic launcher (heartbeat + progress "
                                "watchdog, whole-generation respawn, resume from committed checkpoints)")
            p.add_argument("--max-restarts", type=int, default=3)
            p.add_argument("--stall-timeout", type=float, default=120.0, help="--elastic: seconds without progress")
            p.add_argument("--pg-timeout", type=float, default=120.0, help="--elastic: collective timeout (s)")
            p.add_argument("--final-dir", default=None, help="each rank writes its final state here")
            p.add_argument("--same-device", action="store_true", help="--elastic: every rank on cuda:0 (rehearsal)")
            if name == "engine":
                p.add_argument("--dist-backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
        if name in ("deep", "recurrent"):
            p.add_argument("--iterations", type=int, default=200)
            p.add_argument("--envs", type=int, default=None)
            p.add_argument("--batch", type=int, default=None)
            if name == "deep":
                p.add_argument("--hidden", default="1024,1024,1024,1024", help="hidden widths (config 4: 4x1024)")
            p.add_argument("--metrics", default=None, help="JSONL metrics output path")
            p.add_argument("--log-every", type=int, default=50)
            p.add_argument("--ckpt-dir", default=None)
            p.add_argument("--ckpt-every", type=int, default=0)
            p.add_argument("--resume", action="store_true")
            p.add_argument("--no-graph", action="store_true")
            p.add_argument("--dist-backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
            p.add_argument("--trace", default=None, help="Chrome trace output path (torch.profiler)")
            if name == "recurrent":
                p.add_argument("--bars-file", default=None, metavar="F",
                               help="train on raw OHLCV minute bars: an .npz of [N, T] planes or a one-series .csv "
                                    "(data.ohlcv.load_bars) instead of the synthetic generator's")
                p.add_argument("--train-frac", type=float, default=0.8,
                               help="--bars-file: the leading part of every series that is trained on")
        if name == "serve":
            p.add_argument("--ckpt", default=None, help="engine checkpoint file or directory (default: random init)")
            p.add_argument("--ckpt-root", default=None,
                           help="directory POST /load may read checkpoints from (default: the --ckpt directory; "
                                "without either, /load is disabled)")
            p.add_argument("--host", default="127.0.0.1")
            p.add_argument("--port", type=int, default=8000)
            p.add_argument("--device", default="auto")
            p.add_argument("--max-batch", type=int, default=4096)
            p.add_argument("--max-delay-us", type=float, default=200.0)
            p.add_argument("--weights", choices=["average", "live"], default="average",
                           help="with a checkpoint that keeps a Polyak average (engine.ema_decay): serve it or the "
                                "live weights (profiles/r2_serve_eval.md: evaluate both)")
            p.add_argument("--policy", choices=["auto", "mlp", "gru"], default="auto",
                           help="auto: GRU(256) sessions for a checkpoint of a `recurrent` run, else the MLP routes")
            p.add_argument("--max-sessions", type=int, default=65536, help="GRU policy: slots of the session table")
            p.add_argument("--ep-len", type=int, default=390, help="GRU policy: bars per episode")
            p.add_argument("--cost", type=float, default=0.01, help="GRU policy: cost per position change")
        if name == "backtest":
            p.add_argument("--ckpt", default=None, help="engine checkpoint file or directory (default: random init)")
            p.add_argument("--weights", choices=["average", "live"], default="average",
                           help="with a checkpoint that keeps a Polyak average: backtest it or the live weights")
            src = p.add_mutually_exclusive_group(required=True)
            src.add_argument("--csv", default=None, help="one series: `price, yyyy-MM-dd` rows (or a parsed .npz)")
            src.add_argument("--synthetic", type=int, default=None, metavar="N",
                             help="N random-walk series of data.length days (data.* of the config)")
            src.add_argument("--bars-file", default=None, metavar="F",
                             help="GRU policy: raw OHLCV minute bars, an .npz of [N, T] planes or a one-series .csv of "
                                  "`yyyy-MM-dd HH:mm,open,high,low,close,volume` rows")
            p.add_argument("--held-out", action="store_true",
                           help="--bars-file: only the bars after the checkpoint's train_frac")
            p.add_argument("--train-frac", type=float, default=0.8,
                           help="--bars-file --held-out without a checkpoint that records one")
            p.add_argument("--device", default="auto")
            p.add_argument("--trace-out", default=None, metavar="DIR",
                           help="write actions.npy and equity.npy (GRU policy: reward.npy) here")
            p.add_argument("--policy", choices=["auto", "mlp", "gru"], default="auto",
                           help="auto: the GRU(256) path for a checkpoint of a `recurrent` run, else the MLP path")
            p.add_argument("--bars", type=int, default=None, metavar="T",
                           help="GRU policy: bars per synthetic series (default 4 episodes + 1)")
            p.add_argument("--bars-seed", type=int, default=None, metavar="S",
                           help="GRU policy: seed of the synthetic bars (default: the policy's seed + 1000, held out)")
            p.add_argument("--ep-len", type=int, default=390, help="GRU policy: bars per episode")
            p.add_argument("--cost", type=float, default=0.01, help="GRU policy: cost per position change")
            p.add_argument("--report", action="store_true",
                           help="add a `report` block (drawdown, Sharpe and portfolio figures; GRU policy: hit rate "
                                "and per-episode figures; MLP policy: position, action mix, exposure / timing) for "
                                "the policy and every baseline")
            p.add_argument("--curve-out", default=None, metavar="F.npy",
                           help="write the portfolio curve here (GRU policy: per-bar sum of the series' rewards; MLP "
                                "policy: per-day sum of the series' gains, float64)")
    a = ap.parse_args(argv)
    cfg = _cfg(a)
    logging.basicConfig(level=getattr(logging, cfg.log.loglevel, logging.INFO),
                        format="%(asctime)s %(levelname)s %(name)s %(message)s")
    if a.cmd == "config":
        print(cfg.to_json())
        return 0
    if a.cmd == "train":
        from .app import run

        dp = None
        if a.gpus > 1:
            dev = a.device or "cuda"
            dp = dict(device="cpu" if dev.startswith("cpu") else "cuda", backend=a.dist_backend,
                      envs_per_rank=a.envs_per_rank or cfg.engine.envs_per_rank, ckpt_dir=a.ckpt_dir,
                      ckpt_every=a.ckpt_every, same_device=a.same_device)
        res = run(cfg, engine=a.engine, device=a.device, max_prices=a.max_prices, gpus=a.gpus, dp=dp)
        print(json.dumps(res, default=str))
        return 0 if res.get("completed") else 1
    if a.cmd == "recurrent" and a.bars_file and a.elastic:
        ap.error("--bars-file is not supported under --elastic")
    if a.cmd in ("engine", "deep", "recurrent") and a.elastic:
        # the launcher never touches the GPU: one fresh process per rank (parallel/elastic_cli.py)
        from .parallel.elastic_cli import run_elastic

        dev = getattr(a, "device", None) or "cuda"
        dev = "cpu" if dev.startswith("cpu") else "cuda"
        kw = dict(device=dev, backend=a.dist_backend, metrics=a.metrics, log_every=a.log_every, ckpt_dir=a.ckpt_dir,
                  ckpt_every=a.ckpt_every, graph=not a.no_graph, final_dir=a.final_dir, pg_timeout_s=a.pg_timeout,
                  same_device=a.same_device)
        if a.cmd == "engine":
            kw.update(steps=a.steps, envs=a.envs)
        else:
            lk = {}
            if a.cmd == "deep":
                lk["hidden"] = [int(x) for x in a.hidden.split(",")]
            if a.envs:
                lk["envs"] = a.envs
            if a.batch:
                lk["batch"] = a.batch
            kw.update(steps=a.iterations, learner_kw=lk)
        import os
        import tempfile

        fd, kw["result_path"] = tempfile.mkstemp(suffix=".json")
        os.close(fd)
        r = run_elastic(a.cmd, cfg, a.elastic, kw, max_restarts=a.max_restarts, stall_timeout_s=a.stall_timeout)
        out = {"ok": r.ok, "restarts": r.restarts, "flagged": r.flagged,
               "generations": [{"generation": g.generation, "exitcodes": g.exitcodes, "ok": g.ok,
                                "seconds": round(g.seconds, 2)} for g in r.generations]}
        try:
            with open(kw["result_path"]) as f:
                out["result"] = json.loads(f.read() or "null")
        except (OSError, ValueError):
            pass
        os.unlink(kw["result_path"])
        print(json.dumps(out, default=str))
        return 0 if r.ok else 1
    if a.cmd in ("deep", "recurrent"):
        import torch

        from .trainer.runs import run as run_learner

        kw = {}
        if a.cmd == "deep":
            kw["hidden"] = [int(x) for x in a.hidden.split(",")]
        if a.envs:
            kw["envs"] = a.envs
        if a.batch:
            kw["batch"] = a.batch
        from .parallel import dist as D

        # under torch.distributed.run: one rank per GPU, synchronous data parallel over RCCL
        ctx = D.init(backend=a.dist_backend, device="cuda")
        if a.cmd == "recurrent" and a.bars_file:
            kw["extra_meta"] = _recurrent_bank(a, cfg, ctx, kw)
        res = run_learner(a.cmd, cfg, a.iterations, device=ctx.device, metrics_path=a.metrics,
                          log_every=a.log_every, ckpt_dir=a.ckpt_dir, ckpt_every=a.ckpt_every, resume=a.resume,
                          graph=not a.no_graph, ctx=ctx, trace_path=a.trace, **kw)
        if ctx.is_main:
            print(json.dumps(res, default=float))
        D.shutdown(ctx)
        return 0
    if a.cmd == "serve":
        import uvicorn

        from .serve import DynamicBatcher, PolicyServer
        from .serve.http import load_checkpoint_params, make_app
        from .trainer.engine import resolve_device

        if _gru_path(a):
            from .models import gru_qnet as gq
            from .serve.gru_rollout import GruPolicy
            from .serve.gru_serve import GruBatcher, GruSessionServer
            from .serve.http import make_gru_app

            dev = resolve_device(a.device)
            pol = GruPolicy.from_checkpoint(a.ckpt, device=dev) if a.ckpt else \
                GruPolicy(gq.init_params(cfg.agent.seed), device=dev, seed=cfg.agent.seed)
            gsrv = GruSessionServer(pol, a.max_sessions, ep_len=a.ep_len, cost=a.cost)
            gbat = GruBatcher(gsrv, max_batch=a.max_batch, max_delay_us=a.max_delay_us)
            try:
                uvicorn.run(make_gru_app(gsrv, gbat), host=a.host, port=a.port, log_level="warning")
            finally:
                gbat.close()
            return 0
        params = load_checkpoint_params(a.ckpt, averaged=a.weights == "average") if a.ckpt else None
        srv = PolicyServer(cfg, params=params, device=resolve_device(a.device))
        bat = DynamicBatcher(srv, max_batch=a.max_batch, max_delay_us=a.max_delay_us)
        try:
            import os

            root = a.ckpt_root or (None if not a.ckpt else
                                   a.ckpt if os.path.isdir(a.ckpt) else os.path.dirname(os.path.abspath(a.ckpt)))
            uvicorn.run(make_app(srv, bat, ckpt_root=root), host=a.host, port=a.port, log_level="warning")
        finally:
            bat.close()
        return 0
    if a.cmd == "backtest":
        if _gru_path(a):
            if a.csv:
                ap.error("backtest of a GRU policy: --csv holds daily prices, not minute bars; use --bars-file F "
                         "(raw OHLCV minute bars) or --synthetic N")
            print(json.dumps(_backtest_gru(a, cfg)))
            return 0
        if a.bars_file:
            ap.error("--bars-file is for a GRU policy (--policy gru or a checkpoint of a `recurrent` run)")
        print(json.dumps(_backtest(a, cfg)))
        return 0
    if a.cmd == "engine":
        from .parallel import dist as D
        from .trainer.engine import resolve_device
        from .trainer.loop import train

        ctx = D.init(backend=a.dist_backend, device=None if a.device == "auto" else a.device)
        dev = ctx.device if ctx.is_distributed or a.device == "auto" else resolve_device(a.device)
        res = train(cfg, a.steps, device=dev, envs=a.envs, metrics_path=a.metrics, log_every=a.log_every,
                    ckpt_dir=a.ckpt_dir, ckpt_every=a.ckpt_every, resume=a.resume, trace_path=a.trace,
                    graph=not a.no_graph, rank=ctx.rank, world_size=ctx.world_size, group=ctx.group)
        if ctx.is_main:
            print(json.dumps(res))
        D.shutdown(ctx)
        return 0
    return 2


if __name__ == "__main__":
    sys.exit(main())
