#!/usr/bin/env python3
"""Time one dgen_search_trace call on bench.py's population (default: 1 M
agents of res_1m_nem_tou, one GPU, the bench's device order): HIP events around
the call with every member asked for, and with the [n] members alone (nfev,
certified, undecided_at, system_kw: no [n][32] row stored), --steps rounds
after --warmup; beside it k_size's time of the sizing call (Engine.kernel_times).
Prints one JSON line.
python scripts/search_trace_time.py [--agents N] [--config NAME]"""
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    from dgen_amd import _lib
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine, profile_order
    from dgen_amd.synth import make_population

    pop = make_population(args.config, args.agents, seed=20260000 + 3)          # bench.py's rank-0 population
    eng = Engine(0, EngineConfig(skip_demand_charges=pop.skip_demand_charges, exact_brent=1))
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand)
    eng.set_switches(pop.switches)
    batch = eng.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    out = eng.alloc_outputs(batch.n, hourly=False)
    for _ in range(3):
        eng.size(batch, out)
    torch.cuda.synchronize()
    k_size = eng.kernel_times()[0]
    wants = {"all": tuple(_lib.TRACE_FIELDS), "scalars": ("system_kw",) + tuple(_lib.TRACE_I32)}
    ms = {k: [] for k in wants}
    t = None
    for step in range(args.warmup + args.steps):
        for k, want in wants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t = eng.search_trace(batch, out, want)        # includes the output buffers' allocation
            e1.record()
            e1.synchronize()
            if step >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    res = {"agents": batch.n, "config": args.config, "k_size_ms": k_size, "rerun": eng.exact_count(),
           "certified": int((t["certified"] == 1).sum().item()), "nfev_max": int(t["nfev"].max().item())}
    for k, v in ms.items():
        res[f"search_trace_{k}_ms_median"], res[f"search_trace_{k}_ms_min"] = statistics.median(v), min(v)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
