#!/usr/bin/env python3
"""Time dgen_replay_at against the two calls it generalises, on bench.py's
population (default: 1 M agents of res_1m_nem_tou, one GPU, the bench's device
order and fp32 hourly planes), at the reference's bank (kW* / 0.8 kWh, 2 h) so
that all of them do the same dispatch.

  k_hourly_batt    the scan's average device time per sizing call, from the
                   library's own HIP events (Engine.kernel_times) over --steps
                   sizing calls after --warmup
  batt_summary     HIP events around one Engine.batt_summary call
  replay_summary   HIP events around one dgen_replay_at call, summary only
  replay_planes    the same, the three fp32 planes only (written into the
                   sizing call's plane buffers: the same values)

The three timed calls alternate, --steps rounds after --warmup; median, min and
max (ms) of each, replay_summary / batt_summary and replay_planes /
k_hourly_batt.  Prints one JSON line.
python scripts/replay_at_time.py [--agents N]"""
import argparse
import ctypes
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
    args = ap.parse_args()
    import torch
    from dgen_amd import _lib
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine, profile_order
    from dgen_amd.synth import make_population

    pop = make_population(args.config, args.agents, seed=20260000 + 3)          # bench.py's rank-0 population
    eng = Engine(0, EngineConfig(skip_demand_charges=pop.skip_demand_charges))
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand)
    eng.set_switches(pop.switches)
    batch = eng.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    n = batch.n
    out = eng.alloc_outputs(n, hourly=True)
    c_out = eng.c_outputs(out)
    for _ in range(args.warmup):
        eng.size(batch, out, c_out)
    torch.cuda.synchronize()
    eng.kernel_times()                      # drop the warm-up's events
    for _ in range(args.steps):
        eng.size(batch, out, c_out)
    torch.cuda.synchronize()
    k_size, k_hourly, k_fin, calls = eng.kernel_times()

    # the replay's point: the sized kW* (0 where the sizing call left none) at the reference's bank
    st = out["status"]
    bad = (st & (_lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_UNIT)) != 0
    kw = torch.where(bad | ~torch.isfinite(out["system_kw"]), torch.zeros_like(out["system_kw"]), out["system_kw"])
    kwh = kw / 0.8
    mem = {k: torch.empty((12, n), dtype=torch.float64 if k in _lib.BATT_SUMMARY_F64 else torch.int32, device=eng.dev)
           for k in _lib.BATT_SUMMARY_FIELDS}
    so = _lib.BattSummaryOut(**{k: v.data_ptr() for k, v in mem.items()})
    po = _lib.ReplayPlanes(out["baseline"].data_ptr(), out["net_pvonly"].data_ptr(), out["net_with_batt"].data_ptr(),
                           0, 0)
    bank = torch.empty(n, dtype=torch.float64, device=eng.dev)
    power = torch.empty(n, dtype=torch.float64, device=eng.dev)
    status = torch.empty(n, dtype=torch.int32, device=eng.dev)

    def replay(summary, planes):
        _lib.check(eng.lib.dgen_replay_at(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents),
                                          kw.data_ptr(), kwh.data_ptr(), None, n, None,
                                          ctypes.byref(so) if summary else None,
                                          ctypes.byref(po) if planes else None, bank.data_ptr(), power.data_ptr(),
                                          status.data_ptr(), eng.stream_handle()), "dgen_replay_at")

    calls3 = {"batt_summary": lambda: eng.batt_summary(batch, c_out),
              "replay_summary": lambda: replay(True, False),
              "replay_planes": lambda: replay(False, True)}
    ms = {k: [] for k in calls3}
    for step in range(args.warmup + args.steps):
        for k, f in calls3.items():          # alternating launches
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if step >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    res = {"agents": n, "config": args.config, "k_size_ms": k_size, "k_hourly_batt_ms": k_hourly,
           "k_batt_finance_ms": k_fin, "sizing_calls": calls, "flagged": int(status.count_nonzero().item())}
    for k, v in ms.items():
        res[f"{k}_ms_median"], res[f"{k}_ms_min"], res[f"{k}_ms_max"] = statistics.median(v), min(v), max(v)
    res["summary_ratio"] = res["replay_summary_ms_median"] / res["batt_summary_ms_median"]
    res["planes_ratio_to_scan"] = res["replay_planes_ms_median"] / k_hourly if k_hourly > 0 else None
    res["batt_to_load_kwh_total"] = float(mem["batt_to_load_kwh"].sum().item())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
