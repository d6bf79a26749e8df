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
the tolerance's floor of 2 kW.

--net: the net-billing fill-in instead, on ca_res_storage (200 k agents unless
--agents is given), every agent on metering option 2:
  dgen_batt_curve_net, K = 1   alone on the buffers dgen_batt_curve filled
  dgen_size_with_batt_net      alone on the buffers dgen_size_with_batt filled
  both search calls            as Engine.size_with_batt(net=True) issues them
with the same yardstick from the fill-in's nfev: the K = 1 net time x the mean
over the waves of the wave's largest nfev.

--peak: the demand-charge / kWh/kW fill-in, on bench.py's com_dc_batt (the C4
population, 200 k agents unless --agents is given, demand charges billed),
every agent a candidate:
  dgen_batt_curve_peak, K = 1  alone on the buffers dgen_batt_curve filled
  dgen_size_with_batt_peak     alone on the buffers the first two calls filled
  the three search calls       as Engine.size_with_batt(net=True, peak=True) issues them
with the yardstick from the fill-in's nfev and the K = 1 peak time."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--net", action="store_true")
    ap.add_argument("--peak", action="store_true")
    ap.add_argument("--wide", type=float, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    if args.config is None:
        args.config = "com_dc_batt" if args.peak else "ca_res_storage" if args.net else "res_1m_nem_tou"
    if args.agents is None:
        args.agents = 200_000 if (args.net or args.peak) else 1_000_000
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
    swant = ("system_kw",) + want + ("nfev",)
    if args.peak:
        peak_mode(args, eng, batch, out, one, lo, hi, want, swant, timed, pop)
        eng.close()
        return
    if args.net:
        net_mode(args, eng, batch, out, one, lo, hi, want, swant, timed, pop)
        eng.close()
        return
    c1 = timed(lambda: eng.batt_curve(batch, out, one, want=want))
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


def net_mode(args, eng, batch, out, one, lo, hi, want, swant, timed, pop):
    import ctypes
    import numpy as np
    import torch
    from dgen_amd import _lib
    n = batch.n
    args_c = (eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents))
    # dgen_batt_curve_net alone, on the members dgen_batt_curve filled
    cur = eng.batt_curve(batch, out, one, want=want)
    bo = _lib.BattCurveOut(**{k: v.data_ptr() for k, v in cur.items()})
    co, no = eng.c_outputs(out), _lib.BattNetOpt(0, 0)

    def k1():
        _lib.check(eng.lib.dgen_batt_curve_net(*args_c, ctypes.byref(co), n, 1, one.data_ptr(), None, ctypes.byref(no),
                                               ctypes.byref(bo), eng.stream_handle()), "dgen_batt_curve_net")
    c1 = timed(k1)
    # dgen_size_with_batt_net alone, on the members dgen_size_with_batt filled
    a = None if lo is None else eng._to_dev(lo, torch.float64).contiguous()
    b = None if hi is None else eng._to_dev(hi, torch.float64).contiguous()
    res = eng.size_with_batt(batch, lo=a, hi=b, want=swant)
    so = _lib.SwbOut(**{k: v.data_ptr() for k, v in res.items()})
    opt, sno = _lib.SwbOpt(0.8, 2.0, 0, 0), _lib.SwbNetOpt(0, 0)
    pa, pb = (None if a is None else a.data_ptr()), (None if b is None else b.data_ptr())

    def fill():
        _lib.check(eng.lib.dgen_size_with_batt_net(*args_c, n, pa, pb, ctypes.byref(opt), ctypes.byref(sno),
                                                   ctypes.byref(so), eng.stream_handle()), "dgen_size_with_batt_net")
    sn = timed(fill)
    both = timed(lambda: eng.size_with_batt(batch, lo=a, hi=b, want=swant, net=True))
    first = timed(lambda: eng.size_with_batt(batch, lo=a, hi=b, want=swant))
    r = eng.size_with_batt(batch, lo=a, hi=b, want=("nfev", "status"), net=True)
    torch.cuda.synchronize()
    nfev, st = r["nfev"].cpu().numpy().astype(np.int64), r["status"].cpu().numpy()
    pad = (-nfev.size) % 64
    wave_max = np.concatenate([nfev, np.zeros(pad, np.int64)]).reshape(-1, 64).max(axis=1)
    yard = c1[0] * float(wave_max.mean())
    fatal = _lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_HOURLY_FORM
    print(json.dumps({"agents": n, "config": args.config, "wide": args.wide, "net": True,
                      "max_periods": int(pop.tariffs["P"].max()),
                      "batt_curve_net_k1_ms": c1[0], "size_with_batt_net_ms": sn[0],
                      "size_with_batt_both_ms": both[0], "size_with_batt_first_ms": first[0],
                      "nfev_mean": float(nfev.mean()), "nfev_max": int(nfev.max()),
                      "wave_max_nfev_mean": float(wave_max.mean()),
                      "yardstick_ms": yard, "ratio_to_yardstick": sn[0] / yard,
                      "min_max_ms": {"k1": c1[1:], "net": sn[1:], "both": both[1:], "first": first[1:]},
                      "agents_flagged": int(((st & fatal) != 0).sum())}))


def peak_mode(args, eng, batch, out, one, lo, hi, want, swant, timed, pop):
    import ctypes
    import numpy as np
    import torch
    from dgen_amd import _lib
    n = batch.n
    args_c = (eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents))
    # dgen_batt_curve_peak alone, on the members dgen_batt_curve filled
    cur = eng.batt_curve(batch, out, one, want=want)
    bo = _lib.BattCurveOut(**{k: v.data_ptr() for k, v in cur.items()})
    co, po = eng.c_outputs(out), _lib.BattPeakOpt(0, 0)

    def k1():
        _lib.check(eng.lib.dgen_batt_curve_peak(*args_c, ctypes.byref(co), n, 1, one.data_ptr(), None, ctypes.byref(po),
                                                ctypes.byref(bo), eng.stream_handle()), "dgen_batt_curve_peak")
    c1 = timed(k1)
    # dgen_size_with_batt_peak alone, on the members the first two calls filled
    a = None if lo is None else eng._to_dev(lo, torch.float64).contiguous()
    b = None if hi is None else eng._to_dev(hi, torch.float64).contiguous()
    res = eng.size_with_batt(batch, lo=a, hi=b, want=swant, net=True)
    so = _lib.SwbOut(**{k: v.data_ptr() for k, v in res.items()})
    opt, spo = _lib.SwbOpt(0.8, 2.0, 0, 0), _lib.SwbPeakOpt(0, 0, 0, 0)
    pa, pb = (None if a is None else a.data_ptr()), (None if b is None else b.data_ptr())

    def fill():
        _lib.check(eng.lib.dgen_size_with_batt_peak(*args_c, n, pa, pb, ctypes.byref(opt), ctypes.byref(spo),
                                                    ctypes.byref(so), eng.stream_handle()), "dgen_size_with_batt_peak")
    sp = timed(fill)
    three = timed(lambda: eng.size_with_batt(batch, lo=a, hi=b, want=swant, net=True, peak=True))
    two = timed(lambda: eng.size_with_batt(batch, lo=a, hi=b, want=swant, net=True))
    r = eng.size_with_batt(batch, lo=a, hi=b, want=("nfev", "status"), net=True, peak=True)
    torch.cuda.synchronize()
    nfev, st = r["nfev"].cpu().numpy().astype(np.int64), r["status"].cpu().numpy()
    pad = (-nfev.size) % 64
    wave_max = np.concatenate([nfev, np.zeros(pad, np.int64)]).reshape(-1, 64).max(axis=1)
    yard = c1[0] * float(wave_max.mean())
    fatal = _lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_HOURLY_FORM
    print(json.dumps({"agents": n, "config": args.config, "wide": args.wide, "peak": True,
                      "max_periods": int(pop.tariffs["P"].max()),
                      "agents_with_storage_rows": int((pop.cols["sw_storage_cnt"] > 0).sum()),
                      "batt_curve_peak_k1_ms": c1[0], "size_with_batt_peak_ms": sp[0],
                      "size_with_batt_three_ms": three[0], "size_with_batt_first_two_ms": two[0],
                      "nfev_mean": float(nfev.mean()), "nfev_max": int(nfev.max()),
                      "wave_max_nfev_mean": float(wave_max.mean()),
                      "yardstick_ms": yard, "ratio_to_yardstick": sp[0] / yard,
                      "min_max_ms": {"k1": c1[1:], "peak": sp[1:], "three": three[1:], "first_two": two[1:]},
                      "agents_flagged": int(((st & fatal) != 0).sum())}))


if __name__ == "__main__":
    main()
