#!/usr/bin/env python3
"""GRU serving benchmark (1x MI355X): one bar for B sessions per launch, one JSON line.

For every batch size B (default 1, 32, 1,024, 8,192, 65,536) and two slot patterns -- ``contiguous`` (slots
0 .. B - 1 of a table of B) and ``random`` (B distinct random slots of a table of 4 B):

* ``serve``: ``GruSessionServer.step_into`` (``csrc/gru_serve.hip``) on preallocated device tensors, launches
  back to back on one stream;

and two comparison lines on code older than the serving kernel, for B envs:

* ``backtest_loop``: the one-bar ``GruPolicy.backtest(start=t, steps=1, h0=..., position=..., entry=...)`` loop
  with the state passed through tensors (the precomputed bar returns handed in);
* ``rollout_floor``: one ``csrc/gru_rollout.hip`` launch over ``--bars`` bars divided by the bars: the per-bar
  cost when nothing leaves the chip.

Every window is primed (replayed until two successive windows agree within 5 %, at most 8 times) and timed with
HIP events around the whole window; reported are microseconds per launch (median, min, max over ``--repeats``
windows) and bars per second from the median, plus serve / backtest_loop and serve / rollout_floor.

    python benchmarks/bench_gru_serve.py
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def timed(fn, repeats):
    """Milliseconds of ``repeats`` windows of ``fn`` after priming."""
    last = window_ms(fn)
    for _ in range(8):
        cur = window_ms(fn)
        settled = abs(cur - last) <= 0.05 * max(cur, last)
        last = cur
        if settled:
            break
    return [window_ms(fn) for _ in range(repeats)]


def report(ms, launches, rows):
    us = [m * 1e3 / launches for m in ms]
    med = statistics.median(us)
    return {"us_per_launch": round(med, 3), "us_min": round(min(us), 3), "us_max": round(max(us), 3),
            "launches": launches, "bars_per_s": round(rows / (med * 1e-6), 1)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32,1024,8192,65536")
    ap.add_argument("--bars", type=int, default=64, help="bars of the comparison runs")
    ap.add_argument("--launches", type=int, default=200, help="serve launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ep-len", type=int, default=390)
    args = ap.parse_args()

    import build

    build.build_all()
    from sharetrade.data import minute_bars as mb
    from sharetrade.models import gru_qnet as gq
    from sharetrade.ops import gru as G
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.serve.gru_serve import GruSessionServer

    dev = torch.device("cuda", 0)
    pol = GruPolicy(gq.init_params(0), device=dev, seed=0)
    out = {"bench": "gru_serve", "device": torch.cuda.get_device_name(0), "ep_len": args.ep_len,
           "lds_bytes": int(G.lib().st_gru_serve_lds_bytes()), "sizes": []}
    g = torch.Generator().manual_seed(1)
    for B in (int(v) for v in args.batches.split(",")):
        T = args.bars + 2
        close, feat = mb.generate_gpu(B, T, dev, seed=7)
        ret = mb.bar_returns(close)
        row = {"B": B}
        # ------------------------------------------------ the serving kernel
        launches = args.launches if B <= 8192 else max(20, args.launches // 4)
        for mode in ("contiguous", "random"):
            S = B if mode == "contiguous" else 4 * B
            srv = GruSessionServer(pol, S, ep_len=args.ep_len)
            opened = srv.open(S)
            pick = torch.arange(B) if mode == "contiguous" else torch.randperm(S, generator=g)[:B]
            slots = torch.tensor(opened, dtype=torch.int32)[pick].to(dev)
            f, c = feat[:, 0].contiguous(), close[:, 0].contiguous()
            acts = torch.empty(B, dtype=torch.int8, device=dev)
            pos = torch.empty(B, dtype=torch.int32, device=dev)
            rew = torch.empty(B, device=dev)

            def serve():
                for _ in range(launches):
                    srv.step_into(slots, f, c, None, acts, pos, rew)

            row[f"serve_{mode}"] = dict(report(timed(serve, args.repeats), launches, B), table=S)
            del srv
        # ------------------------------------------------ the one-bar backtest loop, state through tensors
        state = {"h0": torch.zeros(B, G.HID, device=dev), "position": torch.zeros(B, dtype=torch.int32, device=dev),
                 "entry": torch.zeros(B, device=dev)}

        def loop():
            for t in range(args.bars):
                r = pol.backtest(close, feat, start=t, steps=1, ep_len=args.ep_len, origin=0, ret=ret, **state)
                state["h0"], state["position"], state["entry"] = r.h, r.position, r.entry

        row["backtest_loop"] = report(timed(loop, args.repeats), args.bars, B)

        # ------------------------------------------------ one rollout launch over the same bars
        def rollout():
            pol.backtest(close, feat, steps=args.bars, ep_len=args.ep_len, ret=ret)

        row["rollout_floor"] = report(timed(rollout, args.repeats), args.bars, B)
        for mode in ("contiguous", "random"):
            us = row[f"serve_{mode}"]["us_per_launch"]
            row[f"serve_{mode}_over_loop"] = round(us / row["backtest_loop"]["us_per_launch"], 4)
            row[f"serve_{mode}_over_floor"] = round(us / row["rollout_floor"]["us_per_launch"], 4)
        out["sizes"].append(row)
        del close, feat, ret
    out["serve_faster_than_loop_everywhere"] = all(
        r[f"serve_{m}_over_loop"] < 1.0 for r in out["sizes"] for m in ("contiguous", "random"))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
