"""Battery size what-if on demand-charge and kWh/kW-tier tariffs on the GPU:
dgen_batt_curve (+ dgen_batt_curve_net) followed by dgen_batt_curve_peak
against curve_ref (the oracle's PV+battery run with the desired bank supplied,
tests/test_batt_sizing) at the device's own sizes and sticky state; the
fill-in contract (what the entry writes and what it leaves), every metering
option with the TS sell rate, the storage switch across tariff forms,
degradation and life edges, the forced overflow of the kept-hour lists, and
the way up through Engine.batt_curve(peak=True) and
size_chunk(batt_sizing={"peak_billing": True}).

Before each comparison the CPU counts the kept hours (kept_counts,
tests/test_batt_sizing_peak) and the mixed hours (mixed_counts,
tests/test_gpu_batt_curve_net) of every point; a "no overflow" case asserts
that every point is within the default caps and comes back with status 0.

Worst differences observed against curve_ref (MI355X): see DESIGN.md section 5."""
import ctypes

import numpy as np
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from dgen_amd import financial_functions as ff
from dgen_amd.columnar import assign_scratch
from dgen_amd.engine import SWITCH_DTYPE
from dgen_amd.synth import subset
from oracle import oracle as orc
from tests import test_gpu_batt_curve as bc
from tests import test_gpu_batt_curve_net as bn
from tests.test_batt_sizing import _opop, curve_ref_points
from tests.test_batt_sizing_peak import kept_counts

pytestmark = pytest.mark.gpu

DC_SEED, KW_SEED, MIX_SEED = 20260031, 20260033, 20260023
FRACS = bn.FRACS                 # 0.5, 1, 2 x kW* / 0.8
SENT = bn.SENT
UNSIZED = bn.UNSIZED
ALL = lambda a: np.ones(a.shape, bool)


def _peak_raw(eng, batch, out, kwh, kw=None, caps=(0, 0), names=None):
    """dgen_batt_curve_peak alone on sentinel-filled buffers: {member: host [K, n]} of every member
    (those `names` leaves out are not handed to the entry)."""
    e = eng._to_dev(np.atleast_2d(kwh), torch.float64).contiguous()
    p = None if kw is None else eng._to_dev(np.atleast_2d(kw), torch.float64).contiguous()
    K, n = e.shape
    bufs = {k: torch.full((K, n), float(SENT), dtype=torch.float64, device=eng.dev) for k in _lib.BATT_CURVE_F64}
    bufs.update({k: torch.full((K, n), SENT, dtype=torch.int32, device=eng.dev) for k in _lib.BATT_CURVE_I32})
    names = _lib.BATT_CURVE_FIELDS if names is None else names
    bo = _lib.BattCurveOut(**{k: bufs[k].data_ptr() for k in names})
    co = eng.c_outputs(out)
    po = _lib.BattPeakOpt(*caps)
    rc = eng.lib.dgen_batt_curve_peak(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), ctypes.byref(co),
                                      n, K, e.data_ptr(), None if p is None else p.data_ptr(), ctypes.byref(po),
                                      ctypes.byref(bo), eng.stream_handle())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def peak_points(pop, o, tar, dc_on):
    """[K, n]: the points dgen_batt_curve_peak covers (valid kwh assumed): the agent sized, the point's
    tariff on kWh/kW tiers or with a demand record that the engine bills, no malformed demand mats."""
    t = pop.tariffs
    dcb = np.zeros(tar.shape, bool)
    bad = (t["flags"][tar] & _lib.ST_DEMAND) != 0
    if pop.demand is not None and pop.demand.size:
        has = t["dc"][tar] > 0
        dcb = has & bool(dc_on)
        bad |= has & ((pop.demand["flags"][np.maximum(t["dc"][tar], 1) - 1] & _lib.ST_DEMAND) != 0)
    return (np.isin(t["unit"][tar], (1, 3)) | dcb) & ~bad & np.broadcast_to((o["status"] & UNSIZED) == 0, tar.shape)


def worst_lists(pop, opop, cfg, o, kwh, kw=None, where=None):
    """([K, n] worst month's kept hours, [K, n] worst month's mixed hours -- 0 on a bins-form tariff) of
    the points in `where`, counted on the CPU."""
    K, n = kwh.shape
    tar = bn.point_tariffs(pop, o, kwh, kw)
    netf = np.isin(pop.tariffs["mo"][tar], (2, 3))
    kept, mixed = np.zeros((K, n), np.int64), np.zeros((K, n), np.int64)
    for k in range(K):
        for i in range(n):
            if where is not None and not where[k, i]:
                continue
            p = kwh[k, i] / 2.0 if kw is None else kw[k, i]
            a = (opop, cfg, i, float(o["system_kw"][i]), float(kwh[k, i]), float(p))
            kept[k, i] = kept_counts(*a, int(tar[k, i])).max()
            if netf[k, i]:
                mixed[k, i] = bn.mixed_counts(*a).max()
    return kept, mixed


def _mix_dc_pop(n, seed):
    """metering_mix (options 0-4, the TS rate, some kWh/kW tiers) with the demand records of a
    com_dc_batt table behind every second tariff: demand charges under every metering option."""
    pop = bc._pop("metering_mix", n, seed)
    dem = bc._pop("com_dc_batt", 8, DC_SEED).demand
    assert dem is not None and dem.size and (pop.demand is None or not pop.demand.size)
    t = pop.tariffs.copy()
    ix = np.arange(t.size)
    t["dc"] = np.where(ix % 2 == 0, 1 + (ix // 2) % dem.size, 0)
    pop.tariffs, pop.demand = t, dem
    pop.n_scratch = assign_scratch(pop.cols, pop.tariffs, pop.switches)
    return pop


@pytest.fixture(scope="module")
def dc_case(engine_dc):
    """65 com_dc_batt agents sized once on the demand-charge engine, their K = 3 curve after the three
    calls, dgen_batt_curve_peak alone on sentinel buffers, curve_ref and the CPU's list counts (shared)."""
    eng = engine_dc
    pop = bc._pop("com_dc_batt", 65, DC_SEED)
    bc._load(eng, pop)
    batch, out, o = bc._size(eng, pop)
    assert (o["status"] == 0).all()
    kwh = bn._points(o)
    dev = bc._host(eng.batt_curve(batch, out, kwh, net=True, peak=True))
    raw = _peak_raw(eng, batch, out, kwh)
    opop, cfg_o = _opop(pop), orc.make_cfg()
    ref = curve_ref_points(pop, opop, cfg_o, o, kwh)
    kept, mixed = worst_lists(pop, opop, cfg_o, o, kwh)
    print(f"com_dc_batt n=65 K=3: worst month keeps {kept.max()} hours, holds {mixed.max()} mixed hours")
    assert kept.max() <= _lib.BATT_PEAK_CAPK and mixed.max() <= _lib.NB_CAPM          # no overflow
    return {"pop": pop, "batch": batch, "out": out, "o": o, "kwh": kwh, "dev": dev, "raw": raw, "ref": ref,
            "opop": opop, "cfg_o": cfg_o, "kept": kept}


@pytest.mark.parametrize("n", (1, 63, 65))
def test_demand_charge_curve_matches_curve_ref(engine_dc, dc_case, n):
    eng, pop, o = engine_dc, dc_case["pop"], dc_case["o"]
    if n == 65:
        dev, raw = dc_case["dev"], dc_case["raw"]
    else:
        sub = subset(pop, np.arange(n))
        bc._load(eng, pop)
        batch, out, os_ = bc._size(eng, sub)
        assert np.array_equal(os_["system_kw"], o["system_kw"][:n]) and (os_["status"] == 0).all()
        dev = bc._host(eng.batt_curve(batch, out, dc_case["kwh"][:, :n], net=True, peak=True))
        raw = _peak_raw(eng, batch, out, dc_case["kwh"][:, :n])
    assert (dev["status"] == 0).all()            # every point computed after the three calls
    assert bn._written(raw).all()                # and all of them by the peak entry
    bn._same_bits(raw, dev, ALL(raw["npv"]), "peak alone vs the three calls")
    ref = {k: v[:, :n] for k, v in dc_case["ref"].items()}
    bc.compare(dev, ref, f"com_dc_batt n={n} K=3 2 h")
    assert (dev["bank_kwh"] > 0).all()
    if n > 1:
        assert (dev["npv"][0] != dev["npv"][2]).all()


def test_kwh_per_kw_tiers_in_reference_mode(engine):
    pop = bc._pop("com_kwkw", 65, KW_SEED)
    bc._load(engine, pop)
    batch, out, o = bc._size(engine, pop)
    kwh = bn._points(o)
    kwh = np.where(np.isfinite(kwh), kwh, 1.0)
    three = bc._host(engine.batt_curve(batch, out, kwh, net=True, peak=True))
    two = bc._host(engine.batt_curve(batch, out, kwh, net=True))
    raw = _peak_raw(engine, batch, out, kwh)
    tar = bn.point_tariffs(pop, o, kwh)
    cov = peak_points(pop, o, tar, dc_on=False)
    opop, cfg_o = _opop(pop), orc.make_cfg()
    kept, mixed = worst_lists(pop, opop, cfg_o, o, kwh, where=cov)
    print(f"com_kwkw n=65 K=3: {int(cov[0].sum())} kWh/kW agents, worst month keeps {kept.max()} hours, "
          f"holds {mixed.max()} mixed hours")
    assert kept.max() <= _lib.BATT_PEAK_CAPK and mixed.max() <= _lib.NB_CAPM          # no overflow
    assert cov.any() and (~cov).any()
    netf = np.isin(pop.tariffs["mo"][tar], (2, 3))
    print(f"  of them {int((cov & netf)[0].sum())} on net-billing tariffs")
    # the entry wrote exactly the unit 1 / 3 points, bins and net-billing tariffs alike
    assert np.array_equal(bn._written(raw), cov)
    bn._same_bits(raw, three, cov, "peak points")
    bn._same_bits(three, two, ~cov, "every other element: the two-call result")
    assert ((two["status"][cov] & _lib.ST_HOURLY_FORM) != 0).all() and (three["status"][cov] == 0).all()
    flagged = (three["status"] & _lib.ST_HOURLY_FORM) != 0
    assert np.array_equal(flagged, np.broadcast_to((o["status"] & _lib.ST_UNIT) != 0, flagged.shape))
    keep = ~flagged
    assert (three["status"][keep] == 0).all()
    ref = curve_ref_points(pop, opop, cfg_o, o, np.where(keep, kwh, 0.0))
    bc.compare(three, ref, "com_kwkw n=65 K=3 (all points)", keep=keep)
    bc.compare(three, ref, "com_kwkw kWh/kW points", keep=cov)
    if (cov & netf).any():
        bc.compare(three, ref, "com_kwkw kWh/kW points on net-billing tariffs", keep=cov & netf)


@pytest.fixture(scope="module")
def mix_case(engine_dc):
    eng = engine_dc
    pop = _mix_dc_pop(65, MIX_SEED)
    bc._load(eng, pop)
    batch, out, o = bc._size(eng, pop)
    kwh = bn._points(o)
    kwh = np.where(np.isfinite(kwh), kwh, 1.0)
    return {"pop": pop, "batch": batch, "out": out, "o": o, "kwh": kwh, "opop": _opop(pop), "cfg_o": orc.make_cfg()}


def test_metering_mix_with_demand_charges(engine_dc, mix_case):
    eng = engine_dc
    pop, batch, out, o, kwh, opop, cfg_o = (mix_case[k] for k in ("pop", "batch", "out", "o", "kwh", "opop", "cfg_o"))
    bc._load(eng, pop)
    three = bc._host(eng.batt_curve(batch, out, kwh, net=True, peak=True))
    two = bc._host(eng.batt_curve(batch, out, kwh, net=True))
    raw = _peak_raw(eng, batch, out, kwh)
    tar = bn.point_tariffs(pop, o, kwh)
    cov = peak_points(pop, o, tar, dc_on=True)
    kept, mixed = worst_lists(pop, opop, cfg_o, o, kwh, where=cov)
    fits = (kept <= _lib.BATT_PEAK_CAPK) & (mixed <= _lib.NB_CAPM)
    mo = pop.tariffs["mo"][tar]
    ts = bn.ts_agents(pop, tar) & cov
    print(f"metering_mix + demand n=65 K=3: covered per option {[int((cov & (mo == m)).sum()) for m in range(5)]}, "
          f"{int(ts.sum())} on the TS rate, worst month keeps {kept.max()} hours, holds {mixed.max()} mixed hours, "
          f"{int((cov & ~fits).sum())} points beyond a cap")
    assert set(mo[cov & fits]) == {0, 1, 2, 3, 4} and (ts & fits).any()
    assert (cov & fits).sum() * 2 >= cov.sum()
    # written: exactly the covered points within the caps; the siblings' points keep their bits
    assert np.array_equal(bn._written(raw), cov & fits)
    bn._same_bits(raw, three, cov & fits, "peak points")
    bn._same_bits(three, two, ~(cov & fits), "points the peak entry leaves alone")
    assert ((two["status"][cov] & _lib.ST_HOURLY_FORM) != 0).all()
    flagged = (three["status"] & _lib.ST_HOURLY_FORM) != 0
    unit = np.broadcast_to((o["status"] & _lib.ST_UNIT) != 0, flagged.shape)
    assert np.array_equal(flagged & ~unit, cov & ~fits & ~unit)      # beside the DGEN_ST_UNIT agents: overflow alone
    keep = ~flagged & np.broadcast_to((o["status"] & UNSIZED) == 0, flagged.shape)
    assert (three["status"][keep] & bs.INVALID == 0).all()
    ref = curve_ref_points(pop, opop, cfg_o, o, np.where(keep, kwh, 0.0))
    bc.compare(three, ref, "metering_mix + demand (all computed points)", keep=keep)
    for m in range(5):
        bc.compare(three, ref, f"metering_mix + demand, option {m}", keep=cov & fits & (mo == m))
    bc.compare(three, ref, "metering_mix + demand, TS sell rate", keep=ts & fits)


def test_one_and_four_hour_banks_and_no_bank(engine_dc, dc_case):
    eng, pop, batch, out, o = engine_dc, dc_case["pop"], dc_case["batch"], dc_case["out"], dc_case["o"]
    bc._load(eng, pop)
    e = o["system_kw"] / 0.8
    kwh = np.stack([np.zeros_like(e), e, e])
    kw = np.stack([np.ones_like(e), e / 1.0, e / 4.0])       # kwh = 0: the power is not read
    kept, mixed = worst_lists(pop, dc_case["opop"], dc_case["cfg_o"], o, kwh, kw)
    assert kept.max() <= _lib.BATT_PEAK_CAPK and mixed.max() <= _lib.NB_CAPM
    dev = bc._host(eng.batt_curve(batch, out, kwh, kw, net=True, peak=True))
    assert (dev["status"] == 0).all()
    ref = curve_ref_points(pop, dc_case["opop"], dc_case["cfg_o"], o, kwh, kw)
    bc.compare(dev, ref, "com_dc_batt n=65 no bank / 1 h / 4 h")
    two = dc_case["dev"]
    assert np.array_equal(dev["bank_kwh"][1], two["bank_kwh"][1]) and not np.array_equal(dev["power_kw"][1], dev["power_kw"][2])
    assert not np.array_equal(dev["npv"][1], dev["npv"][2])          # the power limit moves the peaks
    # no bank: no switch, and the demand charge still billed on the PV-only peaks
    c = pop.cols
    assert (dev["bank_kwh"][0] == 0).all() and (dev["power_kw"][0] == 0).all()
    assert np.array_equal(dev["tariff"][0], o["tariff_final"]) and np.array_equal(dev["switched"][0], o["switched"])
    assert np.array_equal(dev["total_cost"][0], ((c["capex_combined"] * o["system_kw"] + 0.0) * c["ccm"]) + 0.0 + 0.0)
    assert (dev["bill_w_year1"][0] != dev["bill_w_year1"][1]).any()


def test_storage_switch_across_forms(engine_dc):
    """Hand-set storage rows that only the 2 x point's bank reaches: half of the agents without a billed
    demand charge move onto a demand-charge tariff there (computed by the peak entry only), half of the
    agents with one move off it (left to the two siblings)."""
    eng = engine_dc
    pop = _mix_dc_pop(48, MIX_SEED + 1)
    c, t = pop.cols, pop.tariffs
    bc._load(eng, pop)
    _, _, o0 = bc._size(eng, pop)
    ok_unit = ~np.isin(t["unit"], (1, 3))
    dc_t = np.nonzero((t["dc"] > 0) & ok_unit)[0]
    no_t = np.nonzero((t["dc"] == 0) & ok_unit)[0]
    assert dc_t.size and no_t.size
    kwh = bn._points(o0)
    kwh = np.where(np.isfinite(kwh), kwh, 1.0)
    bank = bn.point_banks(pop, o0, kwh)
    is_dc0 = t["dc"][o0["tariff_final"]] > 0
    rows, off, cnt = [r for r in pop.switches], c["sw_storage_off"].copy(), c["sw_storage_cnt"].copy()
    sized = ((o0["status"] & UNSIZED) == 0) & ok_unit[o0["tariff_final"]]
    for j, i in enumerate(np.nonzero(sized)[0]):
        if j % 2 or not (bank[2, i] > bank[1, i] > 0.0):
            continue
        rec = np.zeros((), dtype=SWITCH_DTYPE)
        rec["min_kw"], rec["max_kw"], rec["one_time_charge"] = 0.5 * (bank[1, i] + bank[2, i]), 1e9, 25.0 + j
        tgt = no_t if is_dc0[i] else dc_t
        rec["tariff"] = tgt[j % tgt.size]
        off[i], cnt[i] = len(rows), 1
        rows.append(rec)
    pop.switches = np.stack(rows).astype(SWITCH_DTYPE)
    c["sw_storage_off"], c["sw_storage_cnt"] = off, cnt
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    bc._load(eng, pop)
    batch, out, o = bc._size(eng, pop)
    assert np.array_equal(o["system_kw"], o0["system_kw"], equal_nan=True)
    assert np.array_equal(o["tariff_final"], o0["tariff_final"])          # the reference's bank misses every row
    tar = bn.point_tariffs(pop, o, kwh)
    cov = peak_points(pop, o, tar, dc_on=True)
    moved = tar != o["tariff_final"]
    to_dc = cov & ~np.broadcast_to(is_dc0, cov.shape) & moved
    off_dc = ~cov & np.broadcast_to(is_dc0 & sized, cov.shape) & moved
    assert to_dc.any() and off_dc.any(), "the rows do not cross the forms both ways"
    opop, cfg_o = _opop(pop), orc.make_cfg()
    kept, mixed = worst_lists(pop, opop, cfg_o, o, kwh, where=cov)
    fits = (kept <= _lib.BATT_PEAK_CAPK) & (mixed <= _lib.NB_CAPM)
    three = bc._host(eng.batt_curve(batch, out, kwh, net=True, peak=True))
    two = bc._host(eng.batt_curve(batch, out, kwh, net=True))
    raw = _peak_raw(eng, batch, out, kwh)
    assert np.array_equal(bn._written(raw), cov & fits)
    print(f"storage switch: {int(to_dc.sum())} points onto a demand charge, {int(off_dc.sum())} off one, "
          f"{int((to_dc & fits).sum())} of the former within the caps")
    assert (to_dc & fits).any()
    assert ((two["status"][to_dc] & _lib.ST_HOURLY_FORM) != 0).all() and (three["status"][to_dc & fits] == 0).all()
    assert (two["status"][off_dc] & _lib.ST_HOURLY_FORM == 0).all()
    bn._same_bits(three, two, ~(cov & fits), "points the peak entry leaves alone")
    assert (three["switched"][to_dc & fits] == 1).all() and (three["switched"][off_dc] == 1).all()
    keep = ((three["status"] & bs.INVALID) == 0)
    ref = curve_ref_points(pop, opop, cfg_o, o, np.where(keep, kwh, 0.0))
    assert np.array_equal(ref["tariff"][keep], tar[keep])
    bc.compare(three, ref, "storage switch across forms n=48 K=3", keep=keep)
    bc.compare(three, ref, "switched onto a demand charge", keep=to_dc & fits)
    bc.compare(three, ref, "switched off a demand charge", keep=off_dc & keep)


def test_degradation_and_life_edges(engine_dc):
    eng = engine_dc
    pop = bc._pop("com_dc_batt", 64, DC_SEED)
    c = pop.cols
    deg, life = c["pv_deg"].copy(), c["econ_life"].copy()
    deg[0:16] = 0.0                  # s_lo = s_hi
    life[16:32] = 1
    life[32:48] = 50
    deg[48:64], life[48:64] = 0.05, 32          # s_N ~ 0.2: long lists
    c["pv_deg"], c["econ_life"] = deg, life
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    bc._load(eng, pop)
    batch, out, o = bc._size(eng, pop)
    assert (o["status"] == 0).all()
    kwh = bn._points(o)
    opop, cfg_o = _opop(pop), orc.make_cfg()
    kept, mixed = worst_lists(pop, opop, cfg_o, o, kwh)
    fits = (kept <= _lib.BATT_PEAK_CAPK) & (mixed <= _lib.NB_CAPM)
    print("edges: worst month's kept hours per group", [int(kept[:, a:a + 16].max()) for a in (0, 16, 32, 48)],
          "mixed", [int(mixed[:, a:a + 16].max()) for a in (0, 16, 32, 48)])
    assert kept[:, 48:].max() > kept[:, :16].max()
    dev = bc._host(eng.batt_curve(batch, out, kwh, net=True, peak=True))
    assert (dev["status"][fits] == 0).all() and ((dev["status"][~fits] & _lib.ST_HOURLY_FORM) != 0).all()
    ref = curve_ref_points(pop, opop, cfg_o, o, kwh)
    for name, a in (("pv_deg = 0", 0), ("life 1", 16), ("life 50", 32), ("pv_deg = 0.05, life 32", 48)):
        keep = fits.copy()
        keep[:, :a] = False
        keep[:, a + 16:] = False
        print(f"edges: {name}: {int(keep.sum())} of {3 * 16} points compared")
        assert keep.sum() * 2 >= 3 * 16
        bc.compare(dev, ref, f"edges: {name}", keep=keep)


def test_forced_overflow_leaves_points_unwritten(engine_dc):
    """cap_kept = 2.  A load shape that falls through every month has its month's peak in the month's
    first hour (midnight, no PV): without a bank that hour alone is kept, so the kwh = 0 points of the
    agents on that shape fit; every other point keeps more than two hours in some month."""
    eng = engine_dc
    pop = bc._pop("com_dc_batt", 65, DC_SEED)
    r0 = int(pop.cols["load_row"][0])
    shapes = pop.shapes.copy()
    shapes[r0] = np.concatenate([2.0 - np.arange(d * 24) / 1000.0 for d in
                                 (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)]).astype(np.float32)
    pop.shapes = shapes
    pop.cols["load_row"][:8] = r0
    bc._load(eng, pop)
    batch, out, o = bc._size(eng, pop)
    assert (o["status"] == 0).all()
    e = o["system_kw"] / 0.8
    kwh = np.stack([np.zeros_like(e), e, 2.0 * e])
    opop, cfg_o = _opop(pop), orc.make_cfg()
    kept, mixed = worst_lists(pop, opop, cfg_o, o, kwh)
    over = kept > 2
    assert mixed.max() <= _lib.NB_CAPM and kept.max() <= _lib.BATT_PEAK_CAPK
    assert over.any() and (~over).any(), (int(over.sum()), over.size)
    full = _peak_raw(eng, batch, out, kwh)
    assert bn._written(full).all()
    raw = _peak_raw(eng, batch, out, kwh, caps=(0, 2))
    assert np.array_equal(bn._written(raw), ~over)
    bn._same_bits(raw, full, ~over, "cap_kept = 2 vs the default cap")
    # through the engine: the overflowed points stay flagged by dgen_batt_curve
    dev = bc._host(eng.batt_curve(batch, out, kwh, net=True, peak=True, peak_caps=(None, 2)))
    assert np.array_equal((dev["status"] & _lib.ST_HOURLY_FORM) != 0, over)
    assert np.isnan(dev["npv"][over]).all() and (dev["status"][~over] == 0).all()
    bc.compare(bc._host(eng.batt_curve(batch, out, kwh, peak=True)), curve_ref_points(pop, opop, cfg_o, o, kwh),
               "falling load shape, default caps")


def test_reference_point_independence_and_identity(engine_dc, dc_case):
    eng = engine_dc
    pop, batch, out, o, kwh, dev = (dc_case[k] for k in ("pop", "batch", "out", "o", "kwh", "dev"))
    bc._load(eng, pop)
    again = bc._host(eng.batt_curve(batch, out, kwh, net=True, peak=True))
    bn._same_bits(again, dev, ALL(kwh), "repeat call")
    for p in range(len(FRACS)):
        one = _peak_raw(eng, batch, out, kwh[p])
        for k in _lib.BATT_CURVE_FIELDS:
            assert one[k].shape == (1, batch.n) and np.array_equal(one[k][0], dev[k][p]), (p, k)
    named = ("npv", "switched")
    part = _peak_raw(eng, batch, out, kwh, names=named)
    for k in _lib.BATT_CURVE_FIELDS:             # NULL members are not written
        assert np.array_equal(part[k], dev[k]) if k in named else (part[k] == SENT).all(), k
    # the reference's point against the sizing call
    k = FRACS.index(1.0)
    assert np.array_equal(dev["bank_kwh"][k], o["batt_kwh"]) and np.array_equal(dev["power_kw"][k], o["batt_kw"])
    assert np.array_equal(dev["tariff"][k], o["tariff_final"])
    print("reference point vs sizing call: worst relative npv",
          float((np.abs(dev["npv"][k] - o["npv_pv_batt"]) / np.maximum(np.abs(o["npv_pv_batt"]), 1.0)).max()))
    assert np.allclose(dev["npv"][k], o["npv_pv_batt"], rtol=bc.RTOL, atol=bc.ATOL)
    assert np.allclose(dev["bill_w_year1"][k], o["bill_w_batt"][:, 1], rtol=bc.RTOL, atol=bc.ATOL)


def test_arguments(engine_dc, engine_hourly_plan, dc_case):
    eng, pop, batch, out = engine_dc, dc_case["pop"], dc_case["batch"], dc_case["out"]
    bc._load(eng, pop)
    n = batch.n
    for K in (0, 17):
        with pytest.raises(_lib.DgenError):
            eng.batt_curve(batch, out, np.ones((K, n)), peak=True)
    e = torch.ones((17, n), dtype=torch.float64, device=eng.dev)
    bo, po = _lib.BattCurveOut(), _lib.BattPeakOpt(0, 0)

    def call(en, b, o_, n_, K, kwh, opt=po):
        co = en.c_outputs(o_)
        return en.lib.dgen_batt_curve_peak(en.ctx, ctypes.byref(en.tables), ctypes.byref(b.c_agents), ctypes.byref(co),
                                           n_, K, kwh, None, None if opt is None else ctypes.byref(opt),
                                           ctypes.byref(bo), en.stream_handle())
    for K in (0, 17, -1):
        assert call(eng, batch, out, n, K, e.data_ptr()) == -1
        assert "dgen_batt_curve_peak" in _lib.last_error()
    assert call(eng, batch, out, n, 1, None) == -1
    assert call(eng, batch, out, 0, 1, e.data_ptr()) == 0
    assert call(eng, batch, out, 0, 1, e.data_ptr(), opt=None) == 0
    assert call(eng, batch, out, n, 1, e.data_ptr(), opt=_lib.BattPeakOpt(_lib.BATT_PEAK_CAPM_MAX + 1, 0)) == -1
    assert call(eng, batch, out, n, 1, e.data_ptr(), opt=_lib.BattPeakOpt(0, _lib.BATT_PEAK_CAPK_MAX + 1)) == -1
    assert call(eng, batch, out, n, 1, e.data_ptr(), opt=_lib.BattPeakOpt(_lib.BATT_PEAK_CAPM_MAX, _lib.BATT_PEAK_CAPK_MAX)) == 0
    with pytest.raises(_lib.DgenError):
        eng.batt_curve(batch, out, np.ones((1, n)), peak=True, peak_caps=(0, _lib.BATT_PEAK_CAPK_MAX + 1))
    torch.cuda.synchronize()
    # the hourly re-plan is not replayed
    en = engine_hourly_plan
    bc._load(en, pop)
    sub = subset(pop, np.arange(4))
    b4 = en.upload_agents(sub.cols, sub.n_scratch)
    o4 = en.alloc_outputs(4, hourly=False)
    e4 = torch.ones((1, 4), dtype=torch.float64, device=en.dev)
    assert call(en, b4, o4, 4, 1, e4.data_ptr()) == -1 and "dgen_batt_curve_peak" in _lib.last_error()
    with pytest.raises(_lib.DgenError):
        en.batt_curve(b4, o4, np.ones((1, 4)), peak=True)


def test_drop_in_switch_with_peak_billing():
    """size_chunk on a frame whose commercial rows carry com_dc_batt's demand-charge tariffs or
    com_kwkw's kWh/kW-tier tariffs.  The drop-in path compiles tariffs as the reference does (demand
    charges not billed), so there the demand-charge rows bill from bins and the kWh/kW rows are the
    ones "peak_billing": True fills in: valid batt_opt_* columns, the same bits for every max_rows;
    without the key the frame is what it was."""
    from dgen_amd.synth import random_tariffs, reference_frame
    df, store, table = reference_frame(100)
    dc_raws = random_tariffs(np.random.default_rng(DC_SEED), 4, "nem_dc")
    kw_raws = random_tariffs(np.random.default_rng(KW_SEED), 8, "kwkw")
    com = np.nonzero((df["sector_abbr"] == "com").to_numpy())[0]
    assert com.size >= 12
    dc_rows, kw_rows = com[0::2], com[1::2]
    td, tid = df["tariff_dict"].to_list(), df["tariff_id"].to_numpy().copy()
    for j, i in enumerate(dc_rows):
        td[i], tid[i] = dc_raws[j % 4], 9000 + j % 4
    for j, i in enumerate(kw_rows):
        td[i], tid[i] = kw_raws[j % 8], 9100 + j % 8
    df["tariff_dict"], df["tariff_id"] = td, tid
    ff._worker_conn = store
    spec = {"pv_to_batt": (0.8, 1.6), "hours": (2.0,), "net_billing": True, "peak_billing": True}
    net = {k: v for k, v in spec.items() if k != "peak_billing"}
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec)
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec, max_rows=64)
    old, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=net)
    off, _ = ff.size_chunk(df, None, table, "simple", hourly="none")
    assert list(non.columns) == list(old.columns) and list(non.columns)[-7:] == list(bs.COLUMNS)
    for c in off.columns:                        # the frame's other columns: the bits of a call without the option
        a, b = off[c].to_numpy(), non[c].to_numpy()
        if a.dtype.kind in "fiu":
            assert np.array_equal(a, b, equal_nan=True), c
        else:
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)), c
    for c in bs.COLUMNS:
        assert np.array_equal(non[c].to_numpy(), sub[c].to_numpy(), equal_nan=True), c
    pt, pt_old, st = (non["batt_opt_point"].to_numpy(), old["batt_opt_point"].to_numpy(),
                      non["batt_opt_status"].to_numpy())
    print(f"drop-in: {dc_rows.size} demand-charge rows ({int((pt_old[dc_rows] == -1).sum())} without a value "
          f"before, {int((pt[dc_rows] == -1).sum())} after), {kw_rows.size} kWh/kW-tariff rows "
          f"({int((pt_old[kw_rows] == -1).sum())} before, {int((pt[kw_rows] == -1).sum())} after)")
    assert (st[dc_rows] == 0).all() and (pt[dc_rows] >= 0).all()
    assert (pt_old[kw_rows] == -1).any() and (pt[kw_rows] >= 0).all() and (st[kw_rows] == 0).all()
    had = pt_old >= 0                            # the rows the key-less call already valued keep their bits
    for c in bs.COLUMNS:
        assert np.array_equal(non[c].to_numpy()[had], old[c].to_numpy()[had], equal_nan=True), c
