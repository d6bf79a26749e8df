"""Battery size what-if on the GPU: dgen_batt_curve against curve_ref (the
oracle's PV+battery run with the desired bank supplied, tests/test_batt_sizing)
at the device's own sizes, against the sizing call at the reference's point,
the storage rate switch, the coverage bit, the edges the header names, and its
way up through Engine.batt_curve, dgen_amd.batt_sizing and the drop-in switch
size_frame / size_chunk(batt_sizing=...).

Worst differences observed against curve_ref (MI355X; K = 6 over 257
residential agents and 64 commercial agents): see DESIGN.md section 5."""
import ctypes

import numpy as np
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig
from dgen_amd.engine import outputs_to_host
from dgen_amd.synth import make_population, subset
from oracle import oracle as orc
from tests import helpers
from tests.test_batt_sizing import _opop, curve_ref, curve_ref_points

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-6               # the project's tolerance on money (tests/test_gpu_parity.py)
RES_N = (1, 63, 65, 257)         # one lane; a 64-lane block less one lane, and plus one; five blocks with a ragged tail
RES_SEED, COM_SEED = 20260003, 20260007
FRACS = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)      # x kW* / 0.8
MONEY = ("npv", "total_cost", "bill_w_year1", "bill_wo_year1", "lifetime_savings")


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


def _load(eng, pop):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, None if pop.skip_demand_charges else pop.demand)
    eng.set_switches(pop.switches)


def _size(eng, pop):
    """Device rows are caller rows (no order)."""
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    torch.cuda.synchronize()
    return batch, out, outputs_to_host(out)


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _points(o):
    return np.stack([f * (o["system_kw"] / 0.8) for f in FRACS])


def compare(dev, ref, what, keep=None):
    """bank and power bit for bit, tariff and switched exact, money 1e-6
    relative / 1e-6 absolute, payback 1e-9 relative where finite; the worst
    differences are printed ahead of the assertions."""
    keep = np.ones(dev["npv"].shape, bool) if keep is None else keep
    worst = {k: float((np.abs(dev[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1.0))[keep].max(initial=0.0)) for k in MONEY}
    fin = keep & (ref["payback_raw"] < 1e98)
    worst["payback_raw"] = float((np.abs(dev["payback_raw"] - ref["payback_raw"]) / np.abs(ref["payback_raw"]))[fin]
                                 .max(initial=0.0))
    print(f"{what}: worst relative " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in ("bank_kwh", "power_kw", "tariff", "switched"):
        assert np.array_equal(dev[k][keep], ref[k][keep]), (what, k)
    for k in MONEY:
        assert np.allclose(dev[k][keep], ref[k][keep], rtol=RTOL, atol=ATOL), (what, k, worst[k])
    assert np.array_equal(dev["payback_raw"][keep] < 1e98, ref["payback_raw"][keep] < 1e98), what
    assert (np.abs(dev["payback_raw"] - ref["payback_raw"])[fin] <= 1e-9 * np.abs(ref["payback_raw"])[fin]).all(), \
        (what, worst["payback_raw"])


@pytest.fixture(scope="module")
def res_case(engine):
    """The 257-agent residential NEM population sized once on the device, its
    K = 6 curve, and curve_ref at the device's sizes (computed once, shared)."""
    pop = _pop("res_1m_nem_tou", max(RES_N), RES_SEED)
    _load(engine, pop)
    batch, out, o = _size(engine, pop)
    assert (o["status"] == 0).all()
    kwh = _points(o)
    dev = _host(engine.batt_curve(batch, out, kwh))
    opop, cfg_o = _opop(pop), orc.make_cfg()
    ref = curve_ref_points(pop, opop, cfg_o, o, kwh)
    return {"pop": pop, "batch": batch, "out": out, "o": o, "kwh": kwh, "dev": dev, "ref": ref, "opop": opop,
            "cfg_o": cfg_o}


@pytest.mark.parametrize("n", RES_N)
def test_residential_curve_matches_curve_ref(engine, res_case, n):
    pop, o = res_case["pop"], res_case["o"]
    if n == max(RES_N):
        dev = res_case["dev"]
    else:
        sub = subset(pop, np.arange(n))
        _load(engine, pop)
        batch, out, os_ = _size(engine, sub)
        assert np.array_equal(os_["system_kw"], o["system_kw"][:n]) and (os_["status"] == 0).all()
        dev = _host(engine.batt_curve(batch, out, res_case["kwh"][:, :n]))
    assert (dev["status"] == 0).all()            # nothing silently left out
    for k in _lib.BATT_CURVE_FIELDS:
        assert dev[k].shape == (len(FRACS), n) and dev[k].dtype == (np.float64 if k in _lib.BATT_CURVE_F64 else np.int32)
    ref = {k: v[:, :n] for k, v in res_case["ref"].items()}
    compare(dev, ref, f"res_1m_nem_tou n={n} K=6 2 h")
    assert (dev["bank_kwh"][0] == 0).all() and (dev["bank_kwh"][1:] > 0).all()
    if n > 1:                                    # the bank changes the economics
        assert (dev["npv"][1] != dev["npv"][5]).all()


def test_one_and_four_hour_banks_match_curve_ref(engine, res_case):
    """kw_pts given: points 0, 2, 4 are 1-hour banks, points 1, 3, 5 4-hour banks."""
    pop, o, n = res_case["pop"], res_case["o"], 65
    sub = subset(pop, np.arange(n))
    _load(engine, pop)
    batch, out, os_ = _size(engine, sub)
    kwh = res_case["kwh"][:, :n]
    hours = np.array([1.0, 4.0, 1.0, 4.0, 1.0, 4.0])[:, None]
    kw = kwh / hours
    kw[0] = 1.0                                  # kwh = 0: the power is not read
    dev = _host(engine.batt_curve(batch, out, kwh, kw))
    assert (dev["status"] == 0).all()
    ref = curve_ref_points(sub, res_case["opop"], res_case["cfg_o"], os_, kwh, kw)
    compare(dev, ref, "res_1m_nem_tou n=65 K=6 1 h / 4 h")
    two = {k: v[:, :n] for k, v in res_case["dev"].items()}
    assert np.array_equal(dev["bank_kwh"], two["bank_kwh"]) and not np.array_equal(dev["power_kw"][1:], two["power_kw"][1:])
    assert not np.array_equal(dev["npv"][1:], two["npv"][1:])


def test_commercial_curve_matches_curve_ref(engine):
    """64 commercial agents: 500 V banks, the commercial Cashloan (depreciation, taxes)."""
    pop = _pop("com_8m", 64, COM_SEED)
    assert not (pop.cols["flags"] & 1).any()
    _load(engine, pop)
    batch, out, o = _size(engine, pop)
    assert (o["status"] == 0).all()
    kwh = _points(o)
    dev = _host(engine.batt_curve(batch, out, kwh))
    assert (dev["status"] == 0).all()
    compare(dev, curve_ref_points(pop, _opop(pop), orc.make_cfg(), o, kwh), "com_8m n=64 K=6 2 h")
    series = np.ceil(500.0 / engine.cfg.batt_v_nom)
    string = engine.cfg.batt_q_full * engine.cfg.batt_v_nom * series * 0.001
    assert np.allclose(dev["bank_kwh"][1:] / string, np.round(dev["bank_kwh"][1:] / string), atol=1e-9)


def test_reference_point_equals_the_sizing_call(engine, res_case):
    o, dev = res_case["o"], res_case["dev"]
    k = FRACS.index(1.0)
    assert np.array_equal(dev["bank_kwh"][k], o["batt_kwh"]) and np.array_equal(dev["power_kw"][k], o["batt_kw"])
    assert np.array_equal(dev["tariff"][k], o["tariff_final"]) and np.array_equal(dev["switched"][k], o["switched"])
    assert np.allclose(dev["npv"][k], o["npv_pv_batt"], rtol=RTOL, atol=ATOL)
    assert np.allclose(dev["bill_w_year1"][k], o["bill_w_batt"][:, 1], rtol=RTOL, atol=ATOL)
    assert np.allclose(dev["bill_wo_year1"][k], o["bill_wo_batt"][:, 1], rtol=RTOL, atol=ATOL)
    print("reference point vs sizing call: worst relative npv",
          float((np.abs(dev["npv"][k] - o["npv_pv_batt"]) / np.maximum(np.abs(o["npv_pv_batt"]), 1.0)).max()))


def _net_hourly_form(pop, tariff, dc_on):
    t = pop.tariffs
    f = np.isin(t["mo"][tariff], (2, 3)) | np.isin(t["unit"][tariff], (1, 3))
    if dc_on:
        f |= t["dc"][tariff] > 0
    return f


def test_storage_rate_switch_on_both_sides_of_a_row(engine):
    pop = helpers.edge_population("res_1m_nem_tou", 66, "short", 31)
    c, sw = pop.cols, pop.switches
    _load(engine, pop)
    batch, out, o = _size(engine, pop)
    ok = (o["status"] & _lib.ST_FATAL) == 0
    assert ok.all()
    n, cfg_o = 66, orc.make_cfg()
    # points below, inside and above the agent's row (agents without a row: around the reference's bank)
    kwh = np.stack([f * (o["system_kw"] / 0.8) for f in (0.5, 1.0, 2.0, 1.0)])
    has = c["sw_storage_cnt"] > 0
    for i in np.nonzero(has)[0]:
        r = sw[int(c["sw_storage_off"][i])]
        lo, hi = float(r["min_kw"]), float(r["max_kw"])
        hi = hi if np.isfinite(hi) and hi < 1e6 else lo + 50.0
        kwh[:, i] = [max(lo * 0.5, 0.3), 0.5 * (lo + hi), hi * 2.0 + 5.0, max(lo - 2.0, 0.0)]
    # from the rows alone: some agent has a point that hits and a point that misses
    hit = np.zeros((4, n), bool)
    for i in np.nonzero(has)[0]:
        r = sw[int(c["sw_storage_off"][i])]
        for k in range(4):
            bank, _ = orc.batt_size(kwh[k, i] / 2.0, kwh[k, i], 240.0 if c["flags"][i] & 1 else 500.0, cfg_o)
            hit[k, i] = bank > 0.0 and float(r["min_kw"]) <= bank < float(r["max_kw"])
    both = hit.any(axis=0) & ~hit.all(axis=0) & ok
    assert both.any(), "no agent with points on both sides of its storage row"
    dev = _host(engine.batt_curve(batch, out, kwh))
    ref = curve_ref_points(pop, _opop(pop), cfg_o, o, kwh)
    keepc = np.broadcast_to(ok, (4, n))
    assert np.array_equal(dev["tariff"][keepc], ref["tariff"][keepc])
    assert np.array_equal(dev["switched"][keepc], ref["switched"][keepc])
    assert (dev["switched"][hit & keepc] == 1).all()
    flagged = _net_hourly_form(pop, ref["tariff"], False) & keepc
    assert np.array_equal((dev["status"] & _lib.ST_HOURLY_FORM) != 0, flagged | ((o["status"] & _lib.ST_UNIT) != 0))
    val = keepc & ~flagged
    assert (dev["status"][val] == 0).all() and (val & hit).any()
    otc = np.zeros((4, n))
    for i in np.nonzero(has)[0]:
        otc[:, i] = np.where(hit[:, i], float(sw[int(c["sw_storage_off"][i])]["one_time_charge"]), 0.0)
    assert (otc[val & hit] > 0).any()            # the one-time charge is in the cost
    compare(dev, ref, "storage switch n=66 K=4", keep=val)


@pytest.mark.parametrize("config,dc", [("metering_mix", False), ("com_kwkw", False), ("com_dc_batt", True)])
def test_coverage_bit_is_the_tariff_form(engine, engine_dc, config, dc):
    eng = engine_dc if dc else engine
    pop = _pop(config, 65, 20260011)
    _load(eng, pop)
    batch, out, o = _size(eng, pop)
    kwh = np.stack([f * (o["system_kw"] / 0.8) for f in (0.0, 1.0)])
    kwh = np.where(np.isfinite(kwh), kwh, 1.0)
    dev = _host(eng.batt_curve(batch, out, kwh))
    want = _net_hourly_form(pop, o["tariff_final"], dc) | ((o["status"] & _lib.ST_UNIT) != 0)
    unsized = (o["status"] & (_lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS)) != 0
    assert not unsized.any()
    got = (dev["status"] & _lib.ST_HOURLY_FORM) != 0
    assert np.array_equal(got, np.broadcast_to(want, got.shape)), config
    for k in _lib.BATT_CURVE_F64:
        assert np.isnan(dev[k][got]).all() and not np.isnan(dev[k][~got]).any(), (config, k)
    if config == "com_dc_batt":
        assert want.all()
        return
    assert want.any() and not want.all()
    if config == "metering_mix":
        assert set(pop.tariffs["mo"][o["tariff_final"][~want]]) == {0, 1, 4}
    else:
        assert np.isin(pop.tariffs["unit"][o["tariff_final"][want]], (1, 3)).any()
    keep = np.broadcast_to(~want, got.shape)
    assert (dev["status"][keep] == 0).all()
    ref = curve_ref_points(pop, _opop(pop), orc.make_cfg(), o, np.where(keep, kwh, 0.0))
    compare(dev, ref, f"{config} n=65 K=2", keep=keep)


def test_edge_points(engine, res_case):
    pop, n = res_case["pop"], 65
    sub = subset(pop, np.arange(n))
    _load(engine, pop)
    batch, out, o = _size(engine, sub)
    e = o["system_kw"] / 0.8
    kwh = np.stack([np.zeros(n), np.full(n, 1e-9), e, -e, np.full(n, np.nan), np.full(n, np.inf), e, e, e, e])
    kw = kwh / 2.0
    kw[6], kw[7], kw[8] = 0.0, -1.0, np.nan
    kw[9] = np.inf
    dev = _host(engine.batt_curve(batch, out, kwh, kw))
    good, bad = [0, 1, 2], [3, 4, 5, 6, 7, 8, 9]
    assert (dev["status"][good] == 0).all() and (dev["status"][bad] == _lib.ST_BOUNDS).all()
    for k in _lib.BATT_CURVE_F64:
        assert np.isnan(dev[k][bad]).all() and np.isfinite(dev[k][good]).all(), k
    # neighbouring points' bits untouched: point 2 is the K = 6 call's reference point
    for k in _lib.BATT_CURVE_FIELDS:
        assert np.array_equal(dev[k][2], res_case["dev"][k][FRACS.index(1.0), :n]), k
    # no bank: no switch, the cost without the battery term
    c = sub.cols
    assert (dev["bank_kwh"][0] == 0).all() and (dev["power_kw"][0] == 0).all()
    assert np.array_equal(dev["tariff"][0], o["tariff_final"]) and np.array_equal(dev["switched"][0], o["switched"])
    assert np.array_equal(dev["total_cost"][0], ((c["capex_combined"] * o["system_kw"] + 0.0) * c["ccm"]) + 0.0 + 0.0)
    # a positive kWh below half a string still buys one string (battery_model_sizing)
    one = orc.batt_size(0.5e-9, 1e-9, 240.0, orc.make_cfg())
    assert one[0] > 0 and (dev["bank_kwh"][1] == one[0]).all() and (dev["power_kw"][1] == one[1]).all()
    ref = curve_ref_points(sub, res_case["opop"], res_case["cfg_o"], o, kwh[:2], kw[:2])
    compare({k: v[:2] for k, v in dev.items()}, ref, "no bank / one string n=65")


def test_arguments(engine, engine_hourly_plan, res_case):
    _load(engine, res_case["pop"])
    batch, out, kwh = res_case["batch"], res_case["out"], res_case["kwh"]
    n = batch.n
    for K in (0, 17):
        with pytest.raises(_lib.DgenError):
            engine.batt_curve(batch, out, np.ones((K, n)))
    co = engine.c_outputs(out)
    e = torch.ones((17, n), dtype=torch.float64, device=engine.dev)
    bo = _lib.BattCurveOut()
    args = (engine.ctx, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents), ctypes.byref(co))
    for K in (0, 17, -1):
        assert engine.lib.dgen_batt_curve(*args, n, K, e.data_ptr(), None, ctypes.byref(bo), engine.stream_handle()) == -1
        assert "dgen_batt_curve" in _lib.last_error()
    assert engine.lib.dgen_batt_curve(*args, n, 1, None, None, ctypes.byref(bo), engine.stream_handle()) == -1
    assert engine.lib.dgen_batt_curve(*args, 0, 1, e.data_ptr(), None, ctypes.byref(bo), engine.stream_handle()) == 0
    with pytest.raises(ValueError):
        engine.batt_curve(batch, out, kwh, want=("npv", "nope"))
    with pytest.raises(ValueError):
        engine.batt_curve(batch, out, kwh[:, :5])
    # the hourly re-plan is not replayed
    eng = engine_hourly_plan
    _load(eng, res_case["pop"])
    sub = subset(res_case["pop"], np.arange(4))
    b4 = eng.upload_agents(sub.cols, sub.n_scratch)
    o4 = eng.alloc_outputs(4, hourly=False)
    with pytest.raises(_lib.DgenError, match="dgen_batt_curve"):
        eng.batt_curve(b4, o4, np.ones((1, 4)))


def test_battery_off_every_bank_is_zero(engine, res_case):
    pop, n = res_case["pop"], 65
    sub = subset(pop, np.arange(n))
    _load(engine, pop)
    engine.set_battery(False)
    try:
        batch, out, o = _size(engine, sub)
        dev = _host(engine.batt_curve(batch, out, res_case["kwh"][:, :n]))
    finally:
        engine.set_battery(True)
    assert (dev["status"] == 0).all() and (dev["bank_kwh"] == 0).all() and (dev["power_kw"] == 0).all()
    for k in _lib.BATT_CURVE_FIELDS:             # every point is the no-bank point
        assert (dev[k] == dev[k][0]).all(), k
        assert np.array_equal(dev[k][0], res_case["dev"][k][0, :n]), k


def test_lives_1_and_50_and_an_unsized_row(engine, res_case):
    pop, n = res_case["pop"], 66
    sub = subset(pop, np.arange(n))
    life = sub.cols["econ_life"].copy()
    life[[1, 64]], life[[2, 65]], life[3] = 1, 50, 51
    sub.cols["econ_life"] = life
    _load(engine, pop)
    batch, out, o = _size(engine, sub)
    assert o["status"][3] == _lib.ST_YEARS and (np.delete(o["status"], 3) == 0).all()
    kwh = res_case["kwh"][:, :n].copy()
    kwh[:, 3] = 1.0
    dev = _host(engine.batt_curve(batch, out, kwh))
    assert (dev["status"][:, 3] == _lib.ST_YEARS).all() and (np.delete(dev["status"], 3, axis=1) == 0).all()
    for k in _lib.BATT_CURVE_F64:
        assert np.isnan(dev[k][:, 3]).all(), k
    same = np.setdiff1d(np.arange(n), [1, 2, 3, 64, 65])
    assert np.array_equal(o["system_kw"][same], res_case["o"]["system_kw"][same])
    for k in _lib.BATT_CURVE_FIELDS:             # the other rows' bits alone
        assert np.array_equal(dev[k][:, same], res_case["dev"][k][:, same]), k
    rows = np.array([1, 2, 64, 65])
    so = subset(sub, rows)
    os_ = {k: v[rows] for k, v in o.items() if v is not None and v.ndim >= 1 and v.shape[0] == n}
    ref = curve_ref_points(so, _opop(so), orc.make_cfg(), os_, kwh[:, rows])
    compare({k: v[:, rows] for k, v in dev.items()}, ref, "lives 1 and 50")


def test_points_are_independent_and_runs_identical(engine, res_case):
    _load(engine, res_case["pop"])
    batch, out, kwh, dev = res_case["batch"], res_case["out"], res_case["kwh"], res_case["dev"]
    again = _host(engine.batt_curve(batch, out, kwh))
    for k in _lib.BATT_CURVE_FIELDS:
        assert np.array_equal(again[k], dev[k], equal_nan=True), k
    for p in (0, 3, 5):
        one = _host(engine.batt_curve(batch, out, kwh[p]))
        for k in _lib.BATT_CURVE_FIELDS:
            assert one[k].shape == (1, batch.n) and np.array_equal(one[k][0], dev[k][p]), (p, k)
    want = ("npv", "bank_kwh", "status")
    part = _host(engine.batt_curve(batch, out, kwh, want=want))
    assert tuple(part) == want
    for k in want:
        assert np.array_equal(part[k], dev[k]), k
    # NULL members are not written: sentinel-filled buffers the struct does not name stay as they are
    n, K = batch.n, kwh.shape[0]
    bufs = {k: torch.full((K, n), -7.0, dtype=torch.float64, device=engine.dev) for k in _lib.BATT_CURVE_F64}
    bufs.update({k: torch.full((K, n), -7, dtype=torch.int32, device=engine.dev) for k in _lib.BATT_CURVE_I32})
    named = ("payback_raw", "tariff")
    bo = _lib.BattCurveOut(**{k: bufs[k].data_ptr() for k in named})
    co = engine.c_outputs(out)
    e = torch.as_tensor(kwh, device=engine.dev).contiguous()
    rc = engine.lib.dgen_batt_curve(engine.ctx, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents),
                                    ctypes.byref(co), n, K, e.data_ptr(), None, ctypes.byref(bo), engine.stream_handle())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for k in _lib.BATT_CURVE_FIELDS:
        a = bufs[k].cpu().numpy()
        assert np.array_equal(a, dev[k]) if k in named else (a == -7).all(), k


def test_curve_outputs_and_best_point_in_caller_order(engine, res_case):
    from dgen_amd.engine import profile_order
    pop = subset(res_case["pop"], np.arange(65))
    _load(engine, res_case["pop"])
    batch = engine.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    assert batch.perm is not None
    out = engine.alloc_outputs(batch.n, hourly=False)
    engine.size(batch, out)
    d = _host(bs.curve_outputs(engine, batch, out, res_case["kwh"][:, :65]))
    for k in _lib.BATT_CURVE_FIELDS:
        assert np.array_equal(d[k], res_case["dev"][k][:, :65]), k
    best = bs.best_point(d)
    assert np.array_equal(best, np.argmax(d["npv"], axis=0)) and (best >= 0).all()


def test_drop_in_switch(engine):
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    spec = {"pv_to_batt": (0.4, 1.6), "hours": (1.0, 4.0)}
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec)
    arr, _ = ff.size_chunk(df, None, table, "simple", hourly="array", batt_sizing=spec)
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec, max_rows=64)
    off, o_off = ff.size_chunk(df, None, table, "simple", hourly="none")
    assert list(non.columns)[-7:] == list(bs.COLUMNS)
    assert list(off.columns) == [c for c in non.columns if c not in bs.COLUMNS]
    assert not any(c in o_off for c in bs.COLUMNS)
    for c in off.columns:                        # the frame's other columns: the bits of a call without the option
        a, b = off[c].to_numpy(), non[c].to_numpy()
        if a.dtype.kind in "fiu":
            assert np.array_equal(a, b, equal_nan=True), c
        else:
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)), c
    for c in bs.COLUMNS:
        a = non[c].to_numpy()
        assert a.dtype == (np.int64 if c in ("batt_opt_point", "batt_opt_status") else np.float64), c
        assert np.array_equal(a, arr[c].to_numpy(), equal_nan=True), c
        assert np.array_equal(a, sub[c].to_numpy(), equal_nan=True), c
    pt, st = non["batt_opt_point"].to_numpy(), non["batt_opt_status"].to_numpy()
    valid = pt >= 0
    assert valid.any() and ((st[valid] & bs.INVALID) == 0).all() and pt.max() <= 4
    # the reference's point is in the grid: where it is valid the best is no worse
    gain = non["batt_opt_npv_gain"].to_numpy()
    assert (gain[np.isfinite(gain)] >= 0).all() and np.isfinite(gain).any()
    ref_best = pt == 4
    assert np.array_equal(non["batt_opt_kwh"].to_numpy()[ref_best], non["batt_kwh"].to_numpy()[ref_best])
