#!/usr/bin/env python3
"""GRU backtest benchmark (1x MI355X): the same env-bars three ways, one JSON line.

* ``rollout``: ``csrc/gru_rollout.hip`` through ``GruPolicy.backtest`` -- ``--bars`` bars of every env of a
  ``RecurrentDQN``'s bank in one launch (greedy, no trace, the learner's precomputed bar returns);
* ``actor_single`` / ``actor_pair``: the only other way to step a GRU policy, ``RecurrentDQN.act()`` with the
  single-chunk and the two-chunk actor kernel: ``bars / seq`` launches covering the same env-bars (they also
  explore, write replay segments and round-trip ``h`` through HBM every ``seq`` bars);
* ``rollout_small``: the rollout on the first ``--small-envs`` envs (8,192 = one workgroup per CU);
* with ``--ledger``: ``rollout_ledger``, the same run through the kernel's ledger instance (``ledger=True``: risk
  ledger and portfolio curve kept on the chip), and ``trace_then_ledger``, the path it replaces: a ``trace=True``
  launch followed by ``ledger_from_trace`` on the traced GPU tensors (``trace_only`` is its launch alone).

Every run is warm (one untimed run first) and timed with HIP events around the whole run; reported are the
median, min and max over ``--repeats`` and ns per env-bar from the median, plus the ratios rollout / actor.

    python benchmarks/bench_gru_backtest.py --envs 65536 --bars 384
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


def report(ms, env_bars):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "repeats": len(ms),
            "ns_per_env_bar": round(med * 1e6 / env_bars, 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--small-envs", type=int, default=8192)
    ap.add_argument("--bars", type=int, default=384, help="bars per env (a multiple of --seq)")
    ap.add_argument("--seq", type=int, default=16, help="bars per actor launch")
    ap.add_argument("--bank-bars", type=int, default=4096, help="bars of the learner's bank")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ledger", action="store_true",
                    help="also time the ledger launch and the trace launch + ledger_from_trace it replaces")
    ap.add_argument("--no-actors", action="store_true", help="skip the actor runs")
    args = ap.parse_args()
    if args.bars % args.seq:
        ap.error("--bars must be a multiple of --seq")

    import build

    build.build_all()
    from sharetrade.config import preset_config
    from sharetrade.ops import gru as G
    from sharetrade.serve.gru_rollout import GruPolicy, ledger_from_trace
    from sharetrade.trainer.recurrent import RecurrentDQN

    dev = torch.device("cuda", 0)
    cfg = preset_config("recurrent")
    d = RecurrentDQN(cfg, dev, envs=args.envs, seq=args.seq, bars=args.bank_bars, actor_kernel="single")
    pol = GruPolicy.from_learner(d)
    env_bars = args.envs * args.bars
    launches = args.bars // args.seq
    out = {"bench": "gru_backtest", "device": torch.cuda.get_device_name(0), "envs": args.envs, "bars": args.bars,
           "seq": args.seq, "actor_launches": launches, "lds_bytes": int(G.lib().st_gru_rollout_lds_bytes()),
           "block": int(G.lib().st_gru_rollout_block()), "grid": pol._auto_grid(args.envs)}

    def rollout(n):
        return lambda: pol.backtest(d.close[:n], d.feat[:n], steps=args.bars, ep_len=d.ep_len, cost=d.cost,
                                    ret=d.ret[:n])

    out["rollout"] = report(timed(rollout(args.envs), args.repeats), env_bars)
    n = min(args.small_envs, args.envs)
    out["rollout_small"] = dict(report(timed(rollout(n), args.repeats), n * args.bars), envs=n,
                                grid=pol._auto_grid(n))
    res = pol.backtest(d.close, d.feat, steps=args.bars, ep_len=d.ep_len, cost=d.cost, ret=d.ret)
    out["rollout_summary"] = res.summary()

    if args.ledger:
        kw = dict(steps=args.bars, ep_len=d.ep_len, cost=d.cost, ret=d.ret)

        def traced(then_ledger):
            def run():
                r = pol.backtest(d.close, d.feat, trace=True, **kw)
                if then_ledger:
                    ledger_from_trace(r.actions, r.reward, start=0, origin=0, ep_len=d.ep_len)
            return run

        out["rollout_ledger"] = report(timed(lambda: pol.backtest(d.close, d.feat, ledger=True, **kw), args.repeats),
                                       env_bars)
        out["trace_only"] = report(timed(traced(False), args.repeats), env_bars)
        out["trace_then_ledger"] = report(timed(traced(True), max(1, args.repeats // 2)), env_bars)
        out["ledger_over_plain"] = round(out["rollout_ledger"]["ms_median"] / out["rollout"]["ms_median"], 4)
        out["ledger_over_trace_then_ledger"] = round(out["rollout_ledger"]["ms_median"] /
                                                     out["trace_then_ledger"]["ms_median"], 4)
        led = pol.backtest(d.close, d.feat, ledger=True, **kw)
        assert torch.equal(led.ret, res.ret), "the ledger launch's returns differ from the plain launch's"
        out["ledger_report"] = {k: v for k, v in led.report()["series"].items()}

    def act():
        for _ in range(launches):
            d.act()

    for kernel in () if args.no_actors else ("single", "pair"):
        d.actor_kernel = kernel
        d.grid = d._auto_grid(dev)
        out[f"actor_{kernel}"] = dict(report(timed(act, args.repeats), env_bars), grid=d.grid)
        out[f"rollout_over_{kernel}"] = round(out["rollout"]["ms_median"] / out[f"actor_{kernel}"]["ms_median"], 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
