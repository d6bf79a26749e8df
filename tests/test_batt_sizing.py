"""Battery size what-if, host side: curve_ref -- one more PV+battery run of the
oracle's driver with the battery's desired kWh / kW supplied, composed from the
oracle's Python entry points -- against Population.run at the reference's
point, and dgen_amd.batt_sizing's host functions on hand-made curves."""
import ctypes

import numpy as np
import pytest

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from dgen_amd.synth import make_population
from oracle import oracle as orc
from tests import helpers

NH = 8760


def agent_hours(a, kw_star):
    """load, pv and the f32-rounded TS sell series (or None) of oracle agent a,
    formed as size_agent_impl forms them."""
    shape = np.ctypeslib.as_array(a.shape, (NH,)).astype(np.float64)
    load = (shape / orc.np_sum(shape)) * a.load_kwh
    gpk = np.ctypeslib.as_array(a.cf, (NH,)).astype(np.float64) / 1e6
    pv = (((gpk * kw_star) * 1000.0) * 0.96) / 1000.0
    ts = None
    if a.wholesale:
        ts = (np.ctypeslib.as_array(a.wholesale, (NH,)) * a.price_mult).astype(np.float32).astype(np.float64)
        if not np.isfinite(ts).all():
            ts = None
    return load, pv, ts


def curve_ref(pop, cfg, i, kw_star, tariff, switched, desired_kwh, desired_kw):
    """The PV+battery run of size_agent_impl (oracle/orc.c) for agent i of the
    orc.Population at kw_star, with desired_kwh / desired_kw in place of
    kw_star / 0.8 and kw_star / 0.8 / 2, from the sticky state (tariff,
    switched).  The storage switch and loan_inputs are restated here."""
    a = pop.agents[i]
    N = int(a.econ_life)
    load, pv, ts = agent_hours(a, kw_star)
    bank, power = orc.batt_size(desired_kw, desired_kwh, 240.0 if a.is_res else 500.0, cfg)
    sysgen, _ = orc.batt_dispatch(load, pv, bank, power, cfg)
    otc = 0.0
    if bank > 0.0:                      # rate_switch: exactly one row with min <= bank < max
        hits = [a.sw_storage[r] for r in range(a.n_sw_storage)
                if a.sw_storage[r].min_kw <= bank and a.sw_storage[r].max_kw > bank]
        if len(hits) == 1:
            tariff, switched, otc = int(hits[0].tariff), 1, float(hits[0].one_time_charge)
    t = pop.tariffs[tariff]
    tsp = ts if (t.mo == 2 and not a.is_ca) else None
    u = orc.ur5(t, cfg, sysgen, load, tsp, N, a.inflation * 100.0, a.escalator * 100.0, a.pv_deg * 100.0)
    aev = u["aev"] + a.vor              # ff:275 (index 0 too)
    system_costs = a.capex_combined * kw_star if kw_star > 0.0 else a.capex * kw_star
    batt_costs = a.batt_capex_kwh_combined * bank * 0.7
    total = ((system_costs + batt_costs) * a.ccm) + 0.0 + otc
    li = orc.LoanIn(nyears=N, market=0 if a.is_res else 1, loan_term=a.loan_term,
                    depr_fed_type=0 if a.is_res else 2, depr_sta_type=0 if a.is_res else 2, pad=0,
                    debt_fraction_pct=100.0 - (a.down_payment * 100.0), fed_tax_pct=(a.tax_rate * 100.0) * 0.7,
                    sta_tax_pct=(a.tax_rate * 100.0) * 0.3, real_disc_pct=a.real_discount * 100.0,
                    inflation_pct=a.inflation * 100.0, itc_fed_pct=a.itc_frac, total_cost=total)
    c = orc.cashloan(li, cfg, aev)
    life = 0.0
    for y in range(1, N + 1):
        life += aev[y]
    return {"npv": c["npv"], "payback_raw": c["payback"], "total_cost": total, "bank_kwh": bank, "power_kw": power,
            "bill_w_year1": u["bill_w"][1], "bill_wo_year1": u["bill_wo"][1], "lifetime_savings": life,
            "tariff": tariff, "switched": switched, "bill_w": u["bill_w"], "bill_wo": u["bill_wo"], "otc": otc}


def curve_ref_points(pop, opop, cfg_o, o, kwh, kw=None, hours=2.0):
    """curve_ref of every (point, agent) of kwh [K, n] at the device's sizes
    and sticky state (o: host outputs): {member: [K, n]}."""
    K, n = kwh.shape
    res = {k: np.zeros((K, n), np.float64 if k in _lib.BATT_CURVE_F64 else np.int32)
           for k in _lib.BATT_CURVE_FIELDS if k != "status"}
    for k in range(K):
        for i in range(n):
            r = curve_ref(opop, cfg_o, i, float(o["system_kw"][i]), int(o["tariff_final"][i]), int(o["switched"][i]),
                          float(kwh[k, i]), float(kwh[k, i]) / hours if kw is None else float(kw[k, i]))
            for m in res:
                res[m][k, i] = r[m]
    return res


def _opop(pop):
    return helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale,
                                     demand=None if pop.skip_demand_charges else pop.demand)


@pytest.mark.parametrize("config,seed", [("res_1m_nem_tou", 11), ("com_8m", 12)])
def test_curve_ref_reproduces_the_driver_at_the_reference_point(config, seed):
    """16 residential and 16 commercial agents, every second one with a storage
    rate-switch row: at (kW* / 0.8, kW* / 0.8 / 2) curve_ref is the driver's
    PV+battery run bit for bit, from the state before and after that run."""
    pop = helpers.edge_population(config, 16, "short", seed)
    assert (pop.cols["sw_storage_cnt"] > 0).sum() >= 4
    opop, cfg = _opop(pop), orc.make_cfg()
    ref = opop.run(cfg)
    n_sw = 0
    for i, r in enumerate(ref):
        assert r["status"] == 0
        kw = r["system_kw"]
        e = kw / 0.8
        # the state the PV-only search left (the storage switch not yet applied) ...
        pre = opop.eval_at(orc.make_cfg(), i, kw, r["x_last"], r["tariff_final"], r["switched"])
        starts = [(r["tariff_final"], r["switched"])]
        if not r["switched"]:
            starts.append((int(pop.cols["tariff0"][i]), 0))
        assert pre["npv_pv_batt"] == r["npv_pv_batt"]
        for t0, s0 in starts:           # ... and the sticky state after it: the switch is idempotent
            c = curve_ref(opop, cfg, i, kw, t0, s0, e, e / 2.0)
            assert c["npv"] == r["npv_pv_batt"], (i, c["npv"], r["npv_pv_batt"])
            assert np.array_equal(c["bill_w"], r["bill_w_pv_batt"]) and np.array_equal(c["bill_wo"], r["bill_wo_pv_batt"])
            assert c["bank_kwh"] == r["batt_kwh"] and c["power_kw"] == r["batt_kw"]
            assert c["tariff"] == r["tariff_final"] and c["switched"] == r["switched"]
        n_sw += int(c["otc"] != 0.0 or c["tariff"] != int(pop.cols["tariff0"][i]))
    print(f"{config}: {n_sw} of {len(ref)} agents off their own tariff after the battery run")


def test_curve_ref_zero_bank_is_the_pv_only_economics_with_the_combined_capex():
    pop = make_population("res_1m_nem_tou", 4, seed=5, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16,
                          n_tariffs=48)
    opop, cfg = _opop(pop), orc.make_cfg()
    for i, r in enumerate(opop.run(cfg)):
        c = curve_ref(opop, cfg, i, r["system_kw"], r["tariff_final"], r["switched"], 0.0, 0.0)
        assert c["bank_kwh"] == 0.0 and c["power_kw"] == 0.0 and c["otc"] == 0.0
        a = opop.agents[i]
        assert c["total_cost"] == ((a.capex_combined * r["system_kw"] + 0.0) * a.ccm) + 0.0 + 0.0
        assert np.isfinite(c["npv"])


# ---- host functions ---------------------------------------------------------
def test_ratio_points_layout_and_the_reference_point():
    kw = np.array([4.0, 7.3, 0.0])
    kwh, p = bs.ratio_points(kw, (0.4, 0.8), (1.0, 2.0, 4.0))
    assert kwh.shape == p.shape == (6, 3)
    for a, r in enumerate((0.4, 0.8)):
        for b, h in enumerate((1.0, 2.0, 4.0)):
            assert np.array_equal(kwh[a * 3 + b], kw / r) and np.array_equal(p[a * 3 + b], kw / r / h)
    e, q = bs.ratio_points(kw)
    assert np.array_equal(e[0], kw / 0.8) and np.array_equal(q[0], kw / 0.8 / 2.0) and e.shape == (1, 3)
    with pytest.raises(ValueError):
        bs.ratio_points(kw, (0.0,), (2.0,))
    with pytest.raises(ValueError):
        bs.ratio_points(kw, (0.8,), (np.nan,))
    with pytest.raises(ValueError):
        bs.ratio_points(kw, tuple(np.linspace(0.1, 1.0, 9)), (1.0, 2.0))      # 18 points > 16


def _curve():
    nan = np.nan
    #            agent: 0 tie   1 NaN skipped  2 all invalid  3 flagged best  4 last
    npv = np.array([[5.0,  nan,  nan,  9.0, 1.0],
                    [5.0,  2.0,  nan,  3.0, 2.0],
                    [4.0,  nan,  nan,  1.0, 3.0]])
    st = np.array([[0, _lib.ST_BOUNDS, _lib.ST_HOURLY_FORM, _lib.ST_HOURLY_FORM, 0],
                   [0, 0, _lib.ST_BOUNDS, 0, 0],
                   [0, _lib.ST_BOUNDS, _lib.ST_HOURLY_FORM, 0, _lib.ST_ZERO_LOAD]], np.int32)
    f = lambda s: np.arange(15, dtype=np.float64).reshape(3, 5) * s
    return {"npv": npv, "status": st, "bank_kwh": f(1.0), "power_kw": f(0.5), "payback_raw": f(0.1)}


def test_best_point_ties_invalid_and_nan():
    c = _curve()
    assert bs.best_point(c).tolist() == [0, 1, -1, 1, 2]     # first wins the tie; a flagged 9.0 is not a value
    c["npv"][1, 1] = np.nan                                  # status 0 but NaN: skipped
    assert bs.best_point(c).tolist() == [0, -1, -1, 1, 2]


def test_best_point_torch_agrees_with_numpy():
    torch = pytest.importorskip("torch")
    c = _curve()
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    assert bs.best_point(t).tolist() == bs.best_point(c).tolist()
    a, b = bs.summarize(c, 1), bs.summarize(t, 1)
    for k in bs.COLUMNS:
        assert np.array_equal(a[k], b[k].numpy(), equal_nan=True), k


def test_summarize_columns():
    c = _curve()
    s = bs.summarize(c, ref_point=1)
    assert tuple(s) == bs.COLUMNS and len(bs.COLUMNS) == 7
    assert s["batt_opt_point"].tolist() == [0, 1, -1, 1, 2]
    assert np.array_equal(s["batt_opt_kwh"], [0.0, 6.0, np.nan, 8.0, 14.0], equal_nan=True)
    assert np.array_equal(s["batt_opt_kw"], [0.0, 3.0, np.nan, 4.0, 7.0], equal_nan=True)
    assert np.array_equal(s["batt_opt_npv"], [5.0, 2.0, np.nan, 3.0, 3.0], equal_nan=True)
    assert np.array_equal(s["batt_opt_npv_gain"], [0.0, 0.0, np.nan, 0.0, 1.0], equal_nan=True)
    assert np.allclose(s["batt_opt_payback"][[0, 1, 3, 4]], [0.0, 0.6, 0.8, 1.4])
    assert s["batt_opt_status"].tolist() == [0, 0, _lib.ST_BOUNDS | _lib.ST_HOURLY_FORM, 0, _lib.ST_ZERO_LOAD]


def test_grid_spec_forms():
    assert bs.grid(True) == ((0.4, 0.8, 1.6), (1.0, 2.0, 4.0))
    assert bs.grid({"hours": [1, 4]}) == ((0.8,), (1, 4))
    assert bs.grid(([0.5], [3.0])) == ((0.5,), (3.0,))
    with pytest.raises(ValueError):
        bs.grid({"ratio": [1]})


def test_abi_binding_is_declared():
    assert "dgen_batt_curve" in _lib.EXPORTED and _lib.ST_HOURLY_FORM == 0x100
    assert [n for n, _ in _lib.BattCurveOut._fields_] == _lib.BATT_CURVE_FIELDS
    assert ctypes.sizeof(_lib.BattCurveOut) == 11 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.ST_HOURLY_FORM & _lib.ST_FATAL == 0 and bs.INVALID & _lib.ST_HOURLY_FORM
