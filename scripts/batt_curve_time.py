#!/usr/bin/env python3
"""Device time of dgen_batt_curve beside dgen_batt_summary (HIP events, one
process): the benchmark's population (bench.py: res_1m_nem_tou, 1 M agents,
profile order) sized once, then 3 warm-ups + 20 timed runs each of
  dgen_batt_summary            (the same replay without the bins and the year loop)
  dgen_batt_curve, K = 1       at the reference's point (kW* / 0.8, 2 h)
  dgen_batt_curve, K = 6       0, 0.25, 0.5, 1, 2, 4 x kW* / 0.8
Prints one JSON line: the median times (ms), the K = 1 / summary ratio and the
K = 6 time per point over the K = 1 time.

--net: dgen_batt_curve_net alone (on buffers dgen_batt_curve filled) at K = 1
and K = 6, beside dgen_batt_curve at K = 1 and the sizing call's own
battery-case kernels (k_hourly_batt + k_batt_finance, dgen_kernel_times), which
do the same work for the reference's point; the default population is then
bench.py's ca_res_storage with 200 k agents in device order.

--peak: the same for dgen_batt_curve_peak (demand charges, kWh/kW tiers); the
default population is bench.py's com_dc_batt with 200 k agents."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--net", action="store_true", help="time dgen_batt_curve_net (net-billing tariffs)")
    ap.add_argument("--peak", action="store_true", help="time dgen_batt_curve_peak (demand charges, kWh/kW tiers)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    fill = args.net or args.peak
    if args.config is None:
        args.config = "com_dc_batt" if args.peak else "ca_res_storage" if args.net else "res_1m_nem_tou"
    if args.agents is None:
        args.agents = 200_000 if fill else 1_000_000
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
    if fill:
        eng.kernel_times()                   # reset: the sizing call's kernels over the runs below alone
        for _ in range(3):
            eng.size(batch, out)
        torch.cuda.synchronize()
        k_size, k_hourly, k_finance, _ = eng.kernel_times()
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
    if fill:
        import ctypes
        from dgen_amd import _lib
        co = eng.c_outputs(out)
        name = "dgen_batt_curve_peak" if args.peak else "dgen_batt_curve_net"
        tag = "peak" if args.peak else "net"

        def net_call(pts):
            res = eng.batt_curve(batch, out, pts, want=want)
            bo = _lib.BattCurveOut(**{k: v.data_ptr() for k, v in res.items()})
            no = _lib.BattPeakOpt(0, 0) if args.peak else _lib.BattNetOpt(0, 0)
            entry = getattr(eng.lib, name)

            def fn():
                _lib.check(entry(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), ctypes.byref(co),
                                 batch.n, int(pts.shape[0]), pts.data_ptr(), None, ctypes.byref(no), ctypes.byref(bo),
                                 eng.stream_handle()), name)
            return fn, res
        f1, r1 = net_call(one)
        f6, r6 = net_call(six)
        n1, n6 = timed(f1), timed(f6)
        torch.cuda.synchronize()             # the buffers now hold what the fill-in wrote
        c1 = timed(lambda: eng.batt_curve(batch, out, one, want=want))
        torch.cuda.synchronize()
        print(json.dumps({"agents": batch.n, "config": args.config, "max_periods": int(pop.tariffs["P"].max()),
                          f"batt_curve_{tag}_k1_ms": n1[0], f"batt_curve_{tag}_k6_ms": n6[0], "batt_curve_k1_ms": c1[0],
                          "sizing_k_hourly_batt_ms": k_hourly, "sizing_k_batt_finance_ms": k_finance,
                          f"ratio_{tag}_k1_over_sizing_battery_case": n1[0] / (k_hourly + k_finance),
                          "k6_per_point_over_k1": n6[0] / 6.0 / n1[0],
                          "min_max_ms": {f"{tag}_k1": n1[1:], f"{tag}_k6": n6[1:], "k1": c1[1:]},
                          "points_flagged_k1": int((r1["status"] != 0).sum().item()),
                          "points_flagged_k6": int((r6["status"] != 0).sum().item())}))
        eng.close()
        return
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
