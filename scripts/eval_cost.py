#!/usr/bin/env python3
"""Cost of one evaluation against the search.

On the bench population (bench.py's config and seed, fp32 planes) this times,
with the k_size slot of dgen_kernel_times:
  * the search kernel of Engine.size (certified paths as configured),
  * the evaluation kernel of Engine.evaluate at the sizes the search found,
and, with HIP events around the call, Engine.objective_curve at K = 11 points
(sensitivity.DEFAULT_REL x load_kwh / naep).  Prints one JSON line with the
times, the mean nfev and the ratio of one evaluation call's kernel to
k_size / mean nfev.

    python scripts/eval_cost.py --agents 1000000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--config", default="res_1m_nem_tou")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--exact", type=int, default=-1, choices=[-1, 0, 1, 2])
    args = ap.parse_args()

    import numpy as np
    import torch
    from dgen_amd import sensitivity
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine, profile_order
    from dgen_amd.synth import make_population

    pop = make_population(args.config, args.agents, seed=20260000 + 3)
    eng = Engine(0, EngineConfig(skip_demand_charges=pop.skip_demand_charges, exact_brent=args.exact))
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand)
    eng.set_switches(pop.switches)
    batch = eng.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    out = eng.alloc_outputs(batch.n, hourly=True)
    c_out = eng.c_outputs(out)

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        eng.kernel_times()
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()
        a, b, c, cnt = eng.kernel_times()
        assert cnt == args.steps
        return {"k_size_slot_ms": a, "k_hourly_batt_ms": b, "k_batt_finance_ms": c}

    res = {"config": args.config, "agents": batch.n, "steps": args.steps}
    res["size"] = timed(lambda: eng.size(batch, out, c_out))
    nfev = out["nfev"].double().mean().item()
    kw = out["system_kw"].clone()
    res["mean_nfev"] = nfev
    res["k_size_per_nfev_ms"] = res["size"]["k_size_slot_ms"] / nfev
    res["evaluate"] = timed(lambda: eng.evaluate(batch, out, kw, c_out))
    res["eval_over_k_size"] = res["evaluate"]["k_size_slot_ms"] / res["size"]["k_size_slot_ms"]
    res["eval_over_k_size_per_nfev"] = res["evaluate"]["k_size_slot_ms"] / res["k_size_per_nfev_ms"]
    naep = eng.profile_sums()[1]
    base = batch.cols["load_kwh"].cpu().numpy() / naep[batch.cols["cf_row"].cpu().numpy()]
    xs = eng._to_dev(sensitivity.size_grid(base), torch.float64)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        eng.objective_curve(batch, xs, want=("npv",))
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.steps):
        eng.objective_curve(batch, xs, want=("npv",))
    e1.record()
    torch.cuda.synchronize()
    res["curve_points"] = int(xs.shape[0])
    res["curve_ms"] = e0.elapsed_time(e1) / args.steps
    res["curve_ms_per_point"] = res["curve_ms"] / int(xs.shape[0])
    eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
