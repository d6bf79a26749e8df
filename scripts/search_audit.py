#!/usr/bin/env python
"""Audit the certified Brent paths' error bound against the oracle.

    python scripts/search_audit.py CONFIG N [--seed S] [--json PATH] [--tables small|bench] [--long-life]

Sizes a synthetic population of CONFIG (dgen_amd.synth) with N agents in the
default mode, lays the fast search open (Engine.search_trace), runs the
oracle's own traced search per agent (oracle.brent_trace) and prints the worst
observed / bound ratio of the objective (f) and of the evaluation points (x),
for the population and per billing path: NEM, net billing, TS sell rate, kWh/kW
tiers, demand charges billed, agents the search switched to another rate, and
analysis periods over 32 years.  A ratio above 1 is a violation of the
certificate's bound.  --json also writes the figures to PATH.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def paths_of(pop, results):
    """Billing-path membership per agent (an agent can be on several): from the
    initial tariff's record and the oracle's result."""
    t = pop.tariffs[np.asarray(pop.cols["tariff0"], np.int64)]
    mo, unit = t["mo"], t["unit"]
    not_ca = (np.asarray(pop.cols["flags"]) & 2) == 0
    ts = (mo == 2) & not_ca & (np.asarray(pop.cols["wholesale_row"]) >= 0) & (pop.wholesale is not None)
    return {
        "all": np.ones(len(mo), bool),
        "nem": ~np.isin(mo, (2, 3)),
        "net_billing": np.isin(mo, (2, 3)),
        "ts_sell_rate": ts,
        "kwh_per_kw": np.isin(unit, (1, 3)),
        "demand": (t["dc"] > 0) & (pop.skip_demand_charges == 0),
        "switched": np.array([bool(r["switched"]) for r in results]),
        "life_over_32": np.asarray(pop.cols["econ_life"]) > 32,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config")
    ap.add_argument("n", type=int)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--tables", choices=("small", "bench"), default="small",
                    help="small: the parity tests' table sizes; bench: make_population's defaults")
    ap.add_argument("--long-life", action="store_true", help="every third agent gets a 33..50-year life")
    a = ap.parse_args()

    import torch
    from dgen_amd import search_audit
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine
    from dgen_amd.synth import make_population
    from oracle import oracle as orc
    from tests import helpers

    kw = dict(n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48) if a.tables == "small" else {}
    pop = make_population(a.config, a.n, seed=a.seed, **kw)
    if a.long_life:
        life = pop.cols["econ_life"].copy()
        life[::3] = 33 + (np.arange(life[::3].size) % 18)
        pop.cols["econ_life"] = life
    skip = pop.skip_demand_charges
    eng = Engine(0, EngineConfig(skip_demand_charges=skip, exact_brent=1))
    try:
        eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
        eng.set_tariffs(pop.tariffs, None if skip else pop.demand)
        eng.set_switches(pop.switches)
        eng.set_battery(False)
        batch = eng.upload_agents(pop.cols, pop.n_scratch)
        out = eng.alloc_outputs(batch.n, hourly=False)
        eng.size(batch, out)
        t = {k: v.cpu().numpy() for k, v in eng.search_trace(batch, out).items()}
        torch.cuda.synchronize()
        rerun = eng.exact_count()
    finally:
        eng.close()
    t0 = time.perf_counter()
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale,
                                     demand=None if skip else pop.demand)
    ocfg = orc.make_cfg()
    traces, results = [], []
    for i in range(a.n):
        tr, res = orc.brent_trace(opop, ocfg, i)
        traces.append(tr.copy() if res[0]["status"] == 0 else None)
        results.append(res[0])
    c = search_audit.compare(t, traces)
    rows = {}
    for name, m in paths_of(pop, results).items():
        got = m & (c["compared"] > 0)
        rows[name] = {
            "agents": int(m.sum()), "compared_agents": int(got.sum()),
            "evaluations": int(c["compared"][m].sum()),
            "certified": int((t["certified"][m] == 1).sum()), "not_settled": int((t["certified"][m] == 0).sum()),
            "worst_f": float(np.max(c["ratio_f"][got])) if got.any() else None,
            "worst_x": float(np.max(c["ratio_x"][got])) if got.any() else None,
            "f_violations": int(c["f_violations"][m].sum()),
            "x_violations_certified": int(c["x_violations"][m & (t["certified"] == 1)].sum()),
        }
    doc = {"config": a.config, "n": a.n, "seed": a.seed, "tables": a.tables, "long_life": bool(a.long_life),
           "skip_demand_charges": int(skip), "rerun": int(rerun), "oracle_s": round(time.perf_counter() - t0, 2),
           "paths": rows}
    print(f"{a.config} n={a.n}: re-run {rerun}, oracle traces in {doc['oracle_s']} s")
    print(f"{'path':<14}{'agents':>8}{'evals':>8}{'cert':>7}{'open':>6}{'worst f':>11}{'worst x':>11}{'viol':>6}")
    for name, r in rows.items():
        f = lambda v: "-" if v is None else f"{v:.3g}"
        print(f"{name:<14}{r['agents']:>8}{r['evaluations']:>8}{r['certified']:>7}{r['not_settled']:>6}"
              f"{f(r['worst_f']):>11}{f(r['worst_x']):>11}{r['f_violations'] + r['x_violations_certified']:>6}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)
    return 0 if rows["all"]["f_violations"] == 0 and rows["all"]["x_violations_certified"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
