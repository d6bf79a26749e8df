#!/usr/bin/env python3
"""Device time of dgen_batt_curve beside dgen_batt_summary (HIP events, one
process): the benchmark's population (bench.py: res_1m_nem_tou, 1 M agents,
profile order) sized once, then 3 warm-ups + 20 timed runs each of
  dgen_batt_summary            (the same replay without the bins and the year loop)
  dgen_batt_curve, K = 1       at the reference's point (kW* / 0.8, 2 h)
  dgen_batt_curve, K = 6       0, 0.25, 0.5, 1, 2, 4 x kW* / 0.8
Prints one JSON line: the median times (ms), the K = 1 / summary ratio and the
K = 6 time per point over the K = 1 time."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--config", default="res_1m_nem_tou")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
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
    e = out["system_kw"] / 0.8
    one = e.view(1, -1).contiguous()
    six = torch.stack([f * e for f in (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)]).contiguous()

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
    s = timed(lambda: eng.batt_summary(batch, out))
    c1 = timed(lambda: eng.batt_curve(batch, out, one, want=want))
    c6 = timed(lambda: eng.batt_curve(batch, out, six, want=want))
    st = eng.batt_curve(batch, out, six, want=("status",))["status"]
    print(json.dumps({"agents": batch.n, "max_periods": int(pop.tariffs["P"].max()),
                      "batt_summary_ms": s[0], "batt_curve_k1_ms": c1[0], "batt_curve_k6_ms": c6[0],
                      "ratio_k1_over_summary": c1[0] / s[0], "k6_per_point_over_k1": c6[0] / 6.0 / c1[0],
                      "min_max_ms": {"summary": s[1:], "k1": c1[1:], "k6": c6[1:]},
                      "points_flagged": int((st != 0).sum().item())}))
    eng.close()


if __name__ == "__main__":
    main()
