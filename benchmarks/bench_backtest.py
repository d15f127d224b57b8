#!/usr/bin/env python3
"""Backtest benchmark (1x MI355X): one episode of every env, four ways, one JSON line.

* ``rollout``: the episode rollout kernel (``csrc/qrollout.hip``, one launch) on a ``VectorEngine``'s bank;
* ``greedy``: ``benchkit.greedy_episode_returns`` on the same engine (one learning step per day at lr 0, on a
  snapshot that is restored) -- the path the rollout replaces for evaluation;
* ``loop``: ``tools/serve_eval.py``'s per-day loop for one served policy (one ``qserve`` launch, a
  ``torch.cat`` of request rows and the env transition in torch per day);
* ``serve_rollout``: the same policy through ``PolicyServer.backtest`` (what ``serve_eval.py --rollout`` runs).

``--ledger`` adds, on the bank and shape of ``rollout``: ``rollout_ledger`` (the kernel's ledger instance with the
portfolio curve, no trace), ``trace_only`` (``trace=True``) and ``trace_then_ledger`` (``trace=True``, then
``ledger_from_trace`` on the device tensors: the path the ledger launch replaces), and asserts that the ledger
launch's final portfolios equal the plain launch's bit for bit.

Every run is warm (one untimed repeat first) and timed with HIP events around the whole episode; reported are
the median, min and max over ``--repeats`` and env-days/s from the median.

    python benchmarks/bench_backtest.py --envs 65536 --eval-envs 8192
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, repeats):
    """Milliseconds of ``repeats`` warm runs of ``fn`` (HIP events, one untimed run first)."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return ms


def report(ms, env_days):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "repeats": len(ms),
            "env_days_per_s": round(env_days / (med * 1e-3), 1)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536, help="rollout / greedy: envs of the engine")
    ap.add_argument("--eval-envs", type=int, default=8192, help="loop / serve_rollout: series traded")
    ap.add_argument("--length", type=int, default=None, help="days per series (default: data.length of the preset)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--what", default="rollout,greedy,loop,serve_rollout")
    ap.add_argument("--ledger", action="store_true",
                    help="with rollout: also time rollout_ledger, trace_only and trace_then_ledger")
    args = ap.parse_args()
    what = set(args.what.split(","))

    import build

    build.build_all()
    from sharetrade.config import preset_config
    from sharetrade.serve import PolicyServer
    from sharetrade.serve.rollout import _lib, day_block
    from sharetrade.trainer import benchkit
    from sharetrade.trainer.engine import VectorEngine, make_price_bank

    dev = torch.device("cuda", 0)
    cfg = preset_config("flagship")
    if args.length:
        cfg.data.length = args.length
    H = cfg.model.history
    out = {"bench": "backtest", "device": torch.cuda.get_device_name(0), "history": H, "days": cfg.data.length - H,
           "day_block": day_block(), "lds_bytes": int(_lib().st_qrollout_lds_bytes())}

    if what & {"rollout", "greedy"}:
        eng = VectorEngine(cfg, device=dev, envs=args.envs)
        env_days = args.envs * (eng.T - eng.H)
        out["envs"] = args.envs
        if "rollout" in what:
            srv = PolicyServer(cfg, params=eng.params, device=dev, backend="native")
            out["rollout"] = report(timed(lambda: srv.backtest(eng.prices), args.repeats), env_days)
            out["rollout_summary"] = benchkit.backtest_returns(eng)
            if args.ledger:
                from sharetrade.serve.rollout import ledger_from_trace

                e = cfg.env

                def trace_then_ledger():
                    res = srv.backtest(eng.prices, trace=True)
                    return ledger_from_trace(eng.prices, res.actions, history=H, budget0=e.budget, shares0=e.shares)

                out["rollout_ledger"] = report(timed(lambda: srv.backtest(eng.prices, ledger=True), args.repeats),
                                               env_days)
                out["trace_only"] = report(timed(lambda: srv.backtest(eng.prices, trace=True), args.repeats), env_days)
                out["trace_then_ledger"] = report(timed(trace_then_ledger, max(1, min(args.repeats, 2))), env_days)
                a, b = srv.backtest(eng.prices), srv.backtest(eng.prices, ledger=True)
                torch.cuda.synchronize()
                assert torch.equal(a.final_portfolio.view(torch.int32), b.final_portfolio.view(torch.int32)), \
                    "the ledger launch's final portfolios differ from the plain launch's"
                out["ledger_final_portfolio_equal"] = True
        if "greedy" in what:
            res = {}
            out["greedy"] = report(timed(lambda: res.update(benchkit.greedy_episode_returns(eng)), args.repeats), env_days)
            out["greedy_summary"] = res
        del eng
        torch.cuda.empty_cache()

    if what & {"loop", "serve_rollout"}:
        from serve_eval import trade

        test = make_price_bank(cfg, args.eval_envs, dev, seed=101)
        srv = PolicyServer(cfg, device=dev, backend="native")
        env_days = args.eval_envs * (test.shape[1] - H)
        out["eval_envs"] = args.eval_envs
        fin = {}
        if "loop" in what:
            run = lambda: fin.__setitem__("loop", trade(test, H, cfg.env.budget, lambda rows, t: srv.infer(rows).long()))  # noqa: E731
            out["loop"] = report(timed(run, args.repeats), env_days)
        if "serve_rollout" in what:
            run = lambda: fin.__setitem__("roll", srv.backtest(test).final_portfolio.double())  # noqa: E731
            out["serve_rollout"] = report(timed(run, args.repeats), env_days)
        if len(fin) == 2:   # the two paths trade alike except where a near-tie flips a trajectory
            out["same_final_frac"] = float((fin["loop"] == fin["roll"]).double().mean())
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
