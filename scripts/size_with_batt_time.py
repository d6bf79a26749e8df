#!/usr/bin/env python3
"""Device time of dgen_size_with_batt beside dgen_batt_curve (HIP events, one
process): the benchmark's population (bench.py: res_1m_nem_tou, 1 M agents,
profile order) sized once, then 3 warm-ups + 20 timed runs each of
  dgen_batt_curve, K = 1       at the reference's point (kW* / 0.8, 2 h): one year walk per lane
  dgen_size_with_batt          the search over the sizing call's bracket, no trace
A wave runs as long as its longest lane, so the yardstick for the search is
the K = 1 time x the mean over the 64-lane waves of the wave's largest nfev,
taken from the nfev output in device order.  Prints one JSON line: the median
times (ms), the nfev statistics, the yardstick and the ratio to it.

--wide F: the bracket's upper end x F (explicit lo / hi): longer searches than
the default bracket's, which for a residential agent spans little more than
the tolerance's floor of 2 kW."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--config", default="res_1m_nem_tou")
    ap.add_argument("--wide", type=float, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dgen_amd import _lib
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine, profile_order
    from dgen_amd.synth import make_population

    pop = make_population(args.config, args.agents, seed=20260000 + 3)
    eng = Engine(0, EngineConfig(skip_demand_charges=pop.skip_demand_charges))
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand)
    eng.set_switches(pop.switches)
    batch = eng.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    torch.cuda.synchronize()
    one = (out["system_kw"] / 0.8).view(1, -1).contiguous()
    lo = hi = None
    if args.wide is not None:
        _, naep = eng.profile_sums()
        perm = batch.perm if batch.perm is not None else np.arange(batch.n)
        ml = (pop.cols["load_kwh"] / naep[pop.cols["cf_row"]])[perm]
        lo, hi = ml * 0.8, ml * 1.25 * args.wide

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    want = ("npv", "payback_raw", "bank_kwh", "power_kw", "status")
    c1 = timed(lambda: eng.batt_curve(batch, out, one, want=want))
    swant = ("system_kw",) + want + ("nfev",)
    sw = timed(lambda: eng.size_with_batt(batch, lo=lo, hi=hi, want=swant))
    r = eng.size_with_batt(batch, lo=lo, hi=hi, want=("nfev", "status"))
    torch.cuda.synchronize()
    nfev, st = r["nfev"].cpu().numpy().astype(np.int64), r["status"].cpu().numpy()
    pad = (-nfev.size) % 64
    wave_max = np.concatenate([nfev, np.zeros(pad, np.int64)]).reshape(-1, 64).max(axis=1)
    yard = c1[0] * float(wave_max.mean())
    fatal = _lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_HOURLY_FORM
    print(json.dumps({"agents": batch.n, "config": args.config, "wide": args.wide,
                      "max_periods": int(pop.tariffs["P"].max()),
                      "batt_curve_k1_ms": c1[0], "size_with_batt_ms": sw[0],
                      "nfev_mean": float(nfev.mean()), "nfev_max": int(nfev.max()),
                      "wave_max_nfev_mean": float(wave_max.mean()),
                      "yardstick_ms": yard, "ratio_to_yardstick": sw[0] / yard,
                      "min_max_ms": {"k1": c1[1:], "size_with_batt": sw[1:]},
                      "agents_flagged": int(((st & fatal) != 0).sum())}))
    eng.close()


if __name__ == "__main__":
    main()
