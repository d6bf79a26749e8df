#!/usr/bin/env python3
"""Time one dgen_batt_summary call against the hourly scan it replays, on
bench.py's population (default: 1 M agents of res_1m_nem_tou, one GPU, the
bench's device order and fp32 hourly planes).

  k_hourly_batt   the scan's average device time per sizing call, from the
                  library's own HIP events (Engine.kernel_times) over --steps
                  sizing calls after --warmup
  batt_summary    HIP events around one Engine.batt_summary call, --steps timed
                  after --warmup; mean and median (ms)

Prints one JSON line.  python scripts/batt_summary_time.py [--agents N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--config", default="res_1m_nem_tou")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-hourly", action="store_true", help="size without the hourly planes")
    args = ap.parse_args()
    import torch
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine, profile_order
    from dgen_amd.synth import make_population

    pop = make_population(args.config, args.agents, seed=20260000 + 3)          # bench.py's rank-0 population
    eng = Engine(0, EngineConfig(skip_demand_charges=pop.skip_demand_charges))
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand)
    eng.set_switches(pop.switches)
    batch = eng.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    out = eng.alloc_outputs(batch.n, hourly=not args.no_hourly)
    c_out = eng.c_outputs(out)
    for _ in range(args.warmup):
        eng.size(batch, out, c_out)
    torch.cuda.synchronize()
    eng.kernel_times()                      # drop the warm-up's events
    for _ in range(args.steps):
        eng.size(batch, out, c_out)
    torch.cuda.synchronize()
    k_size, k_hourly, k_fin, calls = eng.kernel_times()

    res = None
    for _ in range(args.warmup):
        res = eng.batt_summary(batch, c_out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = eng.batt_summary(batch, c_out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    mean, med = statistics.fmean(ms), statistics.median(ms)
    cyc = float(res["batt_to_load_kwh"].sum().item())
    print(json.dumps({"agents": batch.n, "config": args.config, "k_size_ms": k_size, "k_hourly_batt_ms": k_hourly,
                      "k_batt_finance_ms": k_fin, "sizing_calls": calls, "batt_summary_ms_mean": mean,
                      "batt_summary_ms_median": med, "batt_summary_ms_min": min(ms), "batt_summary_ms_max": max(ms),
                      "ratio_to_scan": med / k_hourly if k_hourly > 0 else None, "batt_to_load_kwh_total": cyc}))


if __name__ == "__main__":
    main()
