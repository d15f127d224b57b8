#!/usr/bin/env python3
"""Raw-bar featurisation benchmark (1x MI355X), one JSON line.

* ``history``: ``csrc/bar_features.hip`` on N series of T bars (default 4,096 x 4,096), the tiled kernel (8 waves own
  64 series, 64-bar tiles through LDS) against the one-thread-per-series kernel, on device-resident planes: bars per
  second and the bytes moved per second (26 read + 20 written per bar).
* ``serve``: ``GruSessionServer.step_raw_into`` (the sessions featurise launch + the serve launch) against
  ``step_into`` on precomputed features (the serve launch alone: the code as it was before raw bars) for
  B = 1, 256, 4,096, 65,536 sessions, launches back to back on one stream.

Every window is primed (replayed until two successive windows agree within 5 %, at most 8 times) and timed with HIP
events around the whole window; reported are the median, min and max over ``--repeats`` windows.

    python benchmarks/bench_bar_features.py
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--bars", type=int, default=4096)
    ap.add_argument("--batches", default="1,256,4096,65536")
    ap.add_argument("--launches", type=int, default=200, help="serve launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import build

    build.build_all()
    from sharetrade.data import minute_bars as mb
    from sharetrade.data import ohlcv as ov
    from sharetrade.models import gru_qnet as gq
    from sharetrade.ops import bar_features as BF
    from sharetrade.ops import native
    from sharetrade.serve.gru_rollout import GruPolicy
    from sharetrade.serve.gru_serve import GruSessionServer

    dev = torch.device("cuda", 0)
    out = {"bench": "bar_features", "device": torch.cuda.get_device_name(0),
           "lds_bytes": int(BF.lib().st_bar_features_lds_bytes())}
    # ---------------------------------------------------------------- whole histories
    N, T = args.series, args.bars
    bp = mb.BarParams()
    bars, _ = ov.generate_ohlcv_gpu(N, T, dev, bp, seed=7)
    fp = ov.true_params(N, bp)
    minute = torch.from_numpy(bars.minutes(bp.day).astype("int16")).to(dev)
    st_in = torch.from_numpy(fp.initial_state()).to(dev)
    close = torch.empty(N, T, device=dev)
    feat = torch.empty(N, T, BF.NF, dtype=torch.bfloat16, device=dev)
    st_out = torch.empty(N, BF.NSTATE, device=dev)
    a = BF.BarFeaturesArgs()
    a.open, a.high, a.low, a.close_in, a.volume = (getattr(bars, k).data_ptr() for k in ov.PLANES)
    a.minute, a.state_in = minute.data_ptr(), st_in.data_ptr()
    a.feat, a.close, a.state_out, a.feat32 = feat.data_ptr(), close.data_ptr(), st_out.data_ptr(), None
    a.N, a.T, a.day, a.alpha, a.beta = N, T, bp.day, bp.alpha, bp.beta
    hist = {"series": N, "bars": T}
    keep = {}
    for name, variant in (("tiled", BF.TILED), ("per_series", BF.NAIVE)):
        def run(v=variant):
            native.check(BF.lib().st_bar_features_launch(a, v, native.stream_handle()), "st_bar_features_launch")

        ms = timed(run, args.repeats)
        med = statistics.median(ms)
        hist[name] = {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                      "bars_per_s": round(N * T / (med * 1e-3), 1),
                      "gb_per_s": round(N * T * 46 / (med * 1e-3) / 1e9, 2)}
        keep[name] = (feat.clone(), st_out.clone())
    hist["same_bits"] = bool(torch.equal(keep["tiled"][0].view(torch.int16), keep["per_series"][0].view(torch.int16))
                             and torch.equal(keep["tiled"][1].view(torch.int32),
                                             keep["per_series"][1].view(torch.int32)))
    hist["tiled_over_per_series"] = round(hist["tiled"]["ms"] / hist["per_series"]["ms"], 4)
    out["history"] = hist
    x0 = torch.stack([getattr(bars, k)[:, 0] for k in ov.PLANES], dim=1).contiguous()   # [N, 5]: bar 0 of every series
    f0, c0 = feat[:, 0].contiguous(), close[:, 0].contiguous()
    del bars, minute, feat, close, keep
    # ---------------------------------------------------------------- serving
    pol = GruPolicy(gq.init_params(0), device=dev, seed=0)
    out["serve"] = []
    for B in (int(v) for v in args.batches.split(",")):
        launches = args.launches if B <= 8192 else max(20, args.launches // 4)
        srv = GruSessionServer(pol, B, bar_day=bp.day)
        slots = torch.tensor(srv.open_raw(B, bp.sigma, 1.0), dtype=torch.int32, device=dev)
        rep = (B + N - 1) // N
        x = x0.repeat(rep, 1)[:B].contiguous()
        f, c = f0.repeat(rep, 1)[:B].contiguous(), c0.repeat(rep)[:B].contiguous()
        m = torch.zeros(B, dtype=torch.int32, device=dev)
        acts = torch.empty(B, dtype=torch.int8, device=dev)
        pos = torch.empty(B, dtype=torch.int32, device=dev)
        rew = torch.empty(B, device=dev)
        sf = torch.empty(B, BF.NF, dtype=torch.bfloat16, device=dev)
        sc = torch.empty(B, device=dev)

        def raw():
            for _ in range(launches):
                srv.step_raw_into(slots, x, m, None, acts, pos, rew, feat=sf, close=sc)

        def plain():
            for _ in range(launches):
                srv.step_into(slots, f, c, None, acts, pos, rew)

        row = {"B": B, "launches": launches}
        for name, fn in (("step_into", plain), ("step_raw_into", raw)):
            us = [v * 1e3 / launches for v in timed(fn, args.repeats)]
            med = statistics.median(us)
            row[name] = {"us_per_bar_batch": round(med, 3), "us_min": round(min(us), 3), "us_max": round(max(us), 3),
                         "bars_per_s": round(B / (med * 1e-6), 1)}
        row["raw_over_plain"] = round(row["step_raw_into"]["us_per_bar_batch"]
                                      / row["step_into"]["us_per_bar_batch"], 4)
        out["serve"].append(row)
        del srv
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
