#!/usr/bin/env python3
"""Time dgen_bill_months (plain and battery form) against dgen_batt_summary in
one process, on bench.py's population (default: 1 M agents of res_1m_nem_tou,
one GPU, the bench's device order), and check a 256-agent sample of that run
(the first and the last two blocks) against the numpy restatement of the
definition (tests/test_bill_metrics.bill_months_ref).

  batt_summary       HIP events around one Engine.batt_summary call
  bill_months        HIP events around one Engine.bill_months call at x_last
  bill_months_batt   the same at system_kw with battery=True
each --steps timed after --warmup; median, mean, min, max (ms) and the ratios
of the medians.  Prints one JSON line.
python scripts/bill_months_time.py [--agents N] [--no-check]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": statistics.median(ms), "mean": statistics.fmean(ms), "min": min(ms), "max": max(ms)}


def sample_check(eng, pop, batch, out, res_plain, res_batt, rows):
    """Device rows `rows` of the two results against bill_months_ref: the worst
    relative difference per form and whether the plain form's kWh members are
    the reference's bits."""
    import numpy as np
    from oracle import oracle as orc
    from tests.helpers import oracle_tariffs
    from tests.test_bill_metrics import bill_months_ref
    from dgen_amd import _lib
    ssum, _ = eng.profile_sums()
    cfg_o = orc.make_cfg()
    otar = oracle_tariffs(pop.tariffs, pop.demand)
    demand = eng.cfg.skip_demand_charges == 0
    host = lambda t: t.cpu().numpy()
    xl, kw, tf = host(out["x_last"]), host(out["system_kw"]), host(out["tariff_final"])
    P = {k: host(res_plain[k]) for k in _lib.BILL_FIELDS}
    B = {k: host(res_batt[k]) for k in _lib.BILL_FIELDS}
    worst = {"plain": 0.0, "batt": 0.0}
    exact = True
    c = pop.cols
    for j in rows:
        i = int(batch.perm[j]) if batch.perm is not None else int(j)
        lr, cr, wr = int(c["load_row"][i]), int(c["cf_row"][i]), int(c["wholesale_row"][i])
        ls = float(c["load_kwh"][i]) / float(ssum[lr])
        load = pop.shapes[lr].astype(np.float64) * ls
        t = otar[int(tf[j])]
        ts = None
        if int(t.mo) == 2 and not (int(c["flags"][i]) & 2) and wr >= 0 and pop.wholesale is not None:
            ts = (pop.wholesale[wr] * float(c["price_mult"][i])).astype(np.float32).astype(np.float64)
        for form, size, dev in (("plain", xl[j], P), ("batt", kw[j], B)):
            g = pop.cfs[cr].astype(np.float64) * ((((float(size) * 1000.0) * 0.96) / 1000.0) / 1e6)
            if form == "batt":
                bank, power = orc.batt_size(size / 0.8 / 2.0, size / 0.8, 240.0 if c["flags"][i] & 1 else 500.0, cfg_o)
                if bank > 0.0:
                    g, _ = orc.batt_dispatch(load, g, bank, power, cfg_o)
            r = bill_months_ref(load, g, t, cfg_o, ts, demand=demand)
            for k in _lib.BILL_FIELDS:
                err = np.abs(dev[k][:, j] - r[k]) / np.maximum(np.abs(r[k]), 1.0)
                worst[form] = max(worst[form], float(err.max()))
            if form == "plain":
                exact &= all(np.array_equal(dev[k][:, j], r[k]) for k in ("import_kwh", "export_kwh", "billed_kwh", "peak_kw"))
    return {"sample_agents": len(rows), "sample_worst_rel_plain": worst["plain"], "sample_worst_rel_batt": worst["batt"],
            "sample_plain_kwh_bit_exact": bool(exact), "sample_within_1e-6": max(worst.values()) <= 1e-6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1_000_000)
    ap.add_argument("--config", default="res_1m_nem_tou")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-check", action="store_true", help="skip the 256-agent sample check")
    args = ap.parse_args()
    import numpy as np
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
    out = eng.alloc_outputs(batch.n, hourly=False)
    c_out = eng.c_outputs(out)
    eng.size(batch, out, c_out)
    torch.cuda.synchronize()
    xl, kw, tf = out["x_last"], out["system_kw"], out["tariff_final"]
    keep = {}

    def run(name, fn):
        def call():
            keep[name] = fn()
        return timed(torch, call, args.warmup, args.steps)

    t_sum = run("summary", lambda: eng.batt_summary(batch, c_out))
    t_plain = run("plain", lambda: eng.bill_months(batch, xl, tf))
    t_batt = run("batt", lambda: eng.bill_months(batch, kw, tf, battery=True))
    res = {"agents": batch.n, "config": args.config, "steps": args.steps, "warmup": args.warmup,
           "batt_summary_ms": t_sum, "bill_months_ms": t_plain, "bill_months_batt_ms": t_batt,
           "ratio_batt_to_summary": t_batt["median"] / t_sum["median"],
           "ratio_plain_to_summary": t_plain["median"] / t_sum["median"],
           "ratio_plain_to_batt": t_plain["median"] / t_batt["median"],
           "flagged_agents": int((keep["plain"]["status"] != 0).sum().item()),
           "total_usd_plain": float(torch.nansum(keep["plain"]["total"]).item()),
           "total_usd_batt": float(torch.nansum(keep["batt"]["total"]).item())}
    if not args.no_check:
        n = batch.n
        rows = np.unique(np.concatenate([np.arange(min(128, n)), np.arange(max(n - 128, 0), n)]))
        res.update(sample_check(eng, pop, batch, out, keep["plain"], keep["batt"], rows))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
