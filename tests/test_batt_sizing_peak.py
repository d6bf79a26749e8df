"""Battery size what-if on demand-charge and kWh/kW-tier tariffs, host side:
curve_ref (tests/test_batt_sizing) on such agents against Population.run at
the reference's point -- the checker the device entry dgen_batt_curve_peak is
held to --, the numpy restatement of the per-point demand record's keep rule
(kept_hours / kept_counts: what the kernel keeps per month, and that every
year's peaks over the kept hours are its peaks over all hours), and the Python
plumbing of peak= / "peak_billing"."""
import ctypes

import numpy as np
import pytest

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from oracle import oracle as orc
from tests import helpers
from tests.test_batt_sizing import _opop, agent_hours, curve_ref

NH = 8760
DAYS = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])
MON = np.repeat(np.arange(12), DAYS * 24)


@pytest.mark.parametrize("config,seed", [("com_dc_batt", 31), ("com_kwkw", 32)])
def test_curve_ref_reproduces_the_driver_with_peaks(config, seed):
    """16 edge agents each, every second one with a storage row: at (kW* / 0.8,
    kW* / 0.8 / 2) curve_ref is the driver's PV+battery run bit for bit with
    demand charges billed and with kWh/kW tier caps."""
    pop = helpers.edge_population(config, 16, "short", seed)
    assert (pop.cols["sw_storage_cnt"] > 0).sum() >= 4
    opop, cfg = _opop(pop), orc.make_cfg()
    ref = opop.run(cfg)
    n_dc = n_pk = 0
    for i, r in enumerate(ref):
        assert r["status"] == 0
        t = opop.tariffs[r["tariff_final"]]
        n_dc += int(t.dc_on)
        n_pk += int(t.unit in (1, 3))
        kw = r["system_kw"]
        e = kw / 0.8
        c = curve_ref(opop, cfg, i, kw, r["tariff_final"], r["switched"], e, e / 2.0)
        assert c["npv"] == r["npv_pv_batt"], (i, c["npv"], r["npv_pv_batt"])
        assert np.array_equal(c["bill_w"], r["bill_w_pv_batt"]) and np.array_equal(c["bill_wo"], r["bill_wo_pv_batt"])
        assert c["bank_kwh"] == r["batt_kwh"] and c["power_kw"] == r["batt_kw"]
        assert c["tariff"] == r["tariff_final"] and c["switched"] == r["switched"]
    print(f"{config}: {n_dc} agents with demand charges billed, {n_pk} on kWh/kW tiers, of {len(ref)}")
    assert (n_dc if config == "com_dc_batt" else n_pk) >= 4


# ---- the keep rule ------------------------------------------------------------
def demand_periods(t):
    """[8760] demand period of every hour under oracle tariff t (one period
    without a demand record): the calendar of orc.c's year_demand."""
    if not t.dc_on:
        return np.zeros(NH, np.int64)
    wd = np.array([[t.dc_wkday[m][h] for h in range(24)] for m in range(12)])
    we = np.array([[t.dc_wkend[m][h] for h in range(24)] for m in range(12)])
    i = np.arange(NH)
    return np.where((i % 168) >= 120, we[MON, i % 24], wd[MON, i % 24]).astype(np.int64)


def s_range(pv_deg, life):
    base, s_n = 1.0 - (pv_deg * 100.0) * 0.01, 1.0
    for _ in range(int(life) - 1):
        s_n = s_n * base
    return base, min(s_n, 1.0), max(s_n, 1.0)


def kept_hours(load, sysgen, per, s_lo, s_hi):
    """The kernel's per-point demand record: (keep [8760] bool: the hours whose
    max(d(s_lo), d(s_hi)) exceeds the running lb of their (month, period) as it
    stood before them, lb [8760]: the final lb of each hour's (month, period))."""
    vlo, vhi = load - sysgen * s_lo, load - sysgen * s_hi
    mn, mx = np.minimum(vlo, vhi), np.maximum(vlo, vhi)
    keep, lb = np.zeros(NH, bool), np.zeros(NH)
    grp = MON * 256 + per
    for g in np.unique(grp):
        idx = np.nonzero(grp == g)[0]
        run = np.maximum.accumulate(np.maximum(mn[idx], 0.0))
        keep[idx] = mx[idx] > np.concatenate([[0.0], run[:-1]])
        lb[idx] = run[-1]
    return keep, lb


def point_hours(opop, cfg, i, kw_star, dkwh, dkw):
    a = opop.agents[i]
    load, pv, _ = agent_hours(a, kw_star)
    bank, power = orc.batt_size(dkw, dkwh, 240.0 if a.is_res else 500.0, cfg)
    sysgen, _ = orc.batt_dispatch(load, pv, bank, power, cfg)
    return load, sysgen


def kept_counts(opop, cfg, i, kw_star, dkwh, dkw, tariff, pv_deg=None, life=None):
    """[12] kept hours per month of one point, before the month-end compaction
    (what cap_kept bounds), on the oracle's dispatch under tariff's demand
    schedule."""
    a = opop.agents[i]
    load, sysgen = point_hours(opop, cfg, i, kw_star, dkwh, dkw)
    _, lo, hi = s_range(a.pv_deg if pv_deg is None else pv_deg, a.econ_life if life is None else life)
    keep, _ = kept_hours(load, sysgen, demand_periods(opop.tariffs[tariff]), lo, hi)
    return np.bincount(MON[keep], minlength=12)


def group_peaks(d, grp, hours=None, start=None):
    """max(start, max over the group's hours of d) per (month, period) group, start 0 by default."""
    out = {}
    for g in np.unique(grp):
        sel = grp == g
        s0 = 0.0 if start is None else float(start[sel][0])
        if hours is not None:
            sel = sel & hours
        out[int(g)] = max(s0, float(d[sel].max(initial=s0)))
    return out


@pytest.mark.parametrize("pv_deg", (0.0, 0.05))
def test_kept_hours_carry_every_years_peaks(pv_deg):
    """A dozen demand-charge agents at 0.5, 1 and 4 x the reference's bank: for
    every analysis year the peaks over the kept hours alone (from 0), and over
    the compacted list started from lb, are the peaks over all 8760 hours, bit
    for bit."""
    pop = helpers.edge_population("com_dc_batt", 16, "short", 41, storage_rows=False)
    opop, cfg = _opop(pop), orc.make_cfg()
    ref = opop.run(cfg)[:12]
    worst = 0
    for i, r in enumerate(ref):
        a = opop.agents[i]
        life = max(int(a.econ_life), 25)
        per = demand_periods(opop.tariffs[r["tariff_final"]])
        grp = MON * 256 + per
        base, lo, hi = s_range(pv_deg, life)
        for f in (0.5, 1.0, 4.0):
            e = f * r["system_kw"] / 0.8
            load, sysgen = point_hours(opop, cfg, i, r["system_kw"], e, e / 2.0)
            keep, lb = kept_hours(load, sysgen, per, lo, hi)
            comp = keep & (np.maximum(load - sysgen * lo, load - sysgen * hi) > lb)
            worst = max(worst, int(np.bincount(MON[keep], minlength=12).max()))
            s = 1.0
            for _ in range(life):
                d = load - sysgen * s
                full = group_peaks(d, grp)
                assert group_peaks(d, grp, keep) == full
                assert group_peaks(d, grp, comp, lb) == full
                s = s * base
            assert comp.sum() <= keep.sum() < NH
    print(f"pv_deg {pv_deg}: worst month keeps {worst} hours before compaction")
    assert worst <= _lib.BATT_PEAK_CAPK_MAX


# ---- host plumbing ----------------------------------------------------------
class _Batch:
    perm = None

    def __init__(self, n):
        self.n = n


class _FakeEngine:
    """Engine.batt_curve's signature over a hand-made curve: agent 1's points
    are flagged ST_HOURLY_FORM unless peak=True."""

    def __init__(self):
        self.calls = []

    def _to_dev(self, a, dtype):
        import torch
        return torch.as_tensor(np.asarray(a)).to(dtype)

    def batt_curve(self, batch, out, kwh, kw=None, want=None, net=False, net_cap=None, peak=False, peak_caps=None):
        import torch
        self.calls.append({"net": net, "peak": peak, "peak_caps": peak_caps, "K": int(kwh.shape[0])})
        K, n = kwh.shape
        npv = torch.arange(K * n, dtype=torch.float64).view(K, n)
        st = torch.zeros((K, n), dtype=torch.int32)
        if not peak:
            st[:, 1] = _lib.ST_HOURLY_FORM
            npv[:, 1] = float("nan")
        d = {"npv": npv, "payback_raw": npv * 0.5, "bank_kwh": kwh.clone(), "power_kw": kwh / 2.0, "status": st,
             "total_cost": npv, "bill_w_year1": npv, "bill_wo_year1": npv, "lifetime_savings": npv,
             "tariff": st, "switched": st}
        return {k: d[k] for k in (want or _lib.BATT_CURVE_FIELDS)}


def test_grid_accepts_the_peak_billing_key():
    assert bs.grid({"hours": [1, 4], "peak_billing": True}) == ((0.8,), (1, 4))
    assert bs.grid({"net_billing": True, "peak_billing": True}) == ((bs.REF_PV_TO_BATT,), (bs.REF_HOURS,))
    assert bs.peak_billing({"peak_billing": True}) and not bs.peak_billing({"net_billing": True})
    assert not bs.peak_billing(True) and not bs.peak_billing(([0.8], [2.0])) and not bs.peak_billing({"peak_billing": 0})
    assert not bs.net_billing({"peak_billing": True})         # the one implies nothing about the other
    with pytest.raises(ValueError):
        bs.grid({"peak_biling": True})


def test_peak_is_threaded_to_the_engine_and_fills_the_flagged_agent():
    torch = pytest.importorskip("torch")
    eng, batch = _FakeEngine(), _Batch(3)
    out = {"system_kw": torch.tensor([4.0, 7.3, 2.0], dtype=torch.float64)}
    off = bs.annual_columns(eng, batch, out, {"pv_to_batt": (0.4, 1.6)})
    on = bs.annual_columns(eng, batch, out, {"pv_to_batt": (0.4, 1.6), "peak_billing": True})
    both = bs.annual_columns(eng, batch, out, {"net_billing": True, "peak_billing": True})
    assert [(c["net"], c["peak"]) for c in eng.calls] == [(False, False), (False, True), (True, True)]
    assert all(c["peak_caps"] is None for c in eng.calls) and both["batt_opt_point"].tolist() == [1, 1, 1]
    assert off["batt_opt_point"].tolist() == [2, -1, 2] and on["batt_opt_point"].tolist() == [2, 2, 2]
    assert off["batt_opt_status"][1] == _lib.ST_HOURLY_FORM and on["batt_opt_status"][1] == 0
    for k in bs.COLUMNS:                        # the other agents' columns do not move
        assert np.array_equal(off[k][[0, 2]], on[k][[0, 2]]), k
    kwh = np.ones((2, 3))
    bs.curve_outputs(eng, batch, out, kwh)
    bs.curve_outputs(eng, batch, out, kwh, peak=True)
    bs.curve_outputs(eng, batch, out, kwh, net=True, peak=True, peak_caps=(0, 7))
    assert [(c["net"], c["peak"], c["peak_caps"]) for c in eng.calls[3:]] == \
        [(False, False, None), (False, True, None), (True, True, (0, 7))]
    assert bs._peak_kw(False) == {} and bs._peak_kw(True) == {"peak": True}
    assert bs._peak_kw(True, (3, 4)) == {"peak": True, "peak_caps": (3, 4)}


def test_abi_binding_is_declared():
    assert "dgen_batt_curve_peak" in _lib.EXPORTED
    assert [n for n, _ in _lib.BattPeakOpt._fields_] == ["cap_mixed", "cap_kept"] and ctypes.sizeof(_lib.BattPeakOpt) == 8
    import inspect
    from dgen_amd.engine import Engine
    p = inspect.signature(Engine.batt_curve).parameters
    assert p["peak"].default is False and p["peak_caps"].default is None
    with open(_lib._build.HDR) as f:
        hdr = f.read()
    assert "int32_t dgen_batt_curve_peak(" in hdr and "dgen_batt_peak_opt" in hdr
    assert f"#define DGEN_BATT_PEAK_CAPK      {_lib.BATT_PEAK_CAPK}" in hdr
    assert f"#define DGEN_BATT_PEAK_CAPK_MAX  {_lib.BATT_PEAK_CAPK_MAX}" in hdr
    assert _lib.BATT_PEAK_CAPM_MAX == _lib.NB_CAPM and _lib.BATT_PEAK_CAPK <= _lib.BATT_PEAK_CAPK_MAX == 744
    L = _lib.load(build_if_missing=True)
    at = L.dgen_batt_curve_peak.argtypes
    assert L.dgen_batt_curve_peak.restype is ctypes.c_int32 and len(at) == 11
    assert at[8] is ctypes.POINTER(_lib.BattPeakOpt) and at[9] is ctypes.POINTER(_lib.BattCurveOut)
