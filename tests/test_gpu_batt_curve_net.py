"""Battery size what-if under net billing on the GPU: dgen_batt_curve followed
by dgen_batt_curve_net against curve_ref (the oracle's PV+battery run with the
desired bank supplied, tests/test_batt_sizing) at the device's own sizes and
sticky state; the fill-in contract (what the entry writes and what it leaves),
the TS sell rate, the storage switch across tariff forms, degradation and life
edges, the forced overflow of the mixed-hour lists, and the way up through
Engine.batt_curve(net=True) and size_chunk(batt_sizing={"net_billing": True}).

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
from tests.test_batt_sizing import _opop, agent_hours, curve_ref_points

pytestmark = pytest.mark.gpu

CA_SEED, MIX_SEED = 20260021, 20260023
FRACS = (0.5, 1.0, 2.0)          # x kW* / 0.8
SENT = -7
MON = np.repeat(np.arange(12), np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]) * 24)
UNSIZED = _lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_UNIT


def _points(o):
    return np.stack([f * (o["system_kw"] / 0.8) for f in FRACS])


def _net_raw(eng, batch, out, kwh, kw=None, cap=0, names=None):
    """dgen_batt_curve_net alone on sentinel-filled buffers: {member: host [K, n]} of every member
    (those `names` leaves out are not handed to the entry)."""
    e = eng._to_dev(np.atleast_2d(kwh), torch.float64).contiguous()
    p = None if kw is None else eng._to_dev(np.atleast_2d(kw), torch.float64).contiguous()
    K, n = e.shape
    bufs = {k: torch.full((K, n), float(SENT), dtype=torch.float64, device=eng.dev) for k in _lib.BATT_CURVE_F64}
    bufs.update({k: torch.full((K, n), SENT, dtype=torch.int32, device=eng.dev) for k in _lib.BATT_CURVE_I32})
    names = _lib.BATT_CURVE_FIELDS if names is None else names
    bo = _lib.BattCurveOut(**{k: bufs[k].data_ptr() for k in names})
    co = eng.c_outputs(out)
    no = _lib.BattNetOpt(cap, 0)
    rc = eng.lib.dgen_batt_curve_net(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), ctypes.byref(co),
                                     n, K, e.data_ptr(), None if p is None else p.data_ptr(), ctypes.byref(no),
                                     ctypes.byref(bo), eng.stream_handle())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _written(raw):
    """[K, n]: the points the entry wrote; every member agrees on it."""
    w = raw["status"] != SENT
    for k in _lib.BATT_CURVE_FIELDS:
        assert np.array_equal(raw[k] != SENT, w), k
    return w


def _same_bits(a, b, where, what):
    for k in _lib.BATT_CURVE_FIELDS:
        assert np.array_equal(a[k][where], b[k][where], equal_nan=True), (what, k)


def point_banks(pop, o, kwh, kw=None):
    cfg, c = orc.make_cfg(), pop.cols
    K, n = kwh.shape
    bank = np.zeros((K, n))
    for k in range(K):
        for i in range(n):
            p = kwh[k, i] / 2.0 if kw is None else kw[k, i]
            bank[k, i] = orc.batt_size(float(p), float(kwh[k, i]), 240.0 if c["flags"][i] & 1 else 500.0, cfg)[0]
    return bank


def point_tariffs(pop, o, kwh, kw=None):
    """The tariff each point bills under, from the rows alone: the sticky tariff_final, moved by exactly
    one storage row with min_kw <= bank < max_kw."""
    c, sw = pop.cols, pop.switches
    bank = point_banks(pop, o, kwh, kw)
    tar = np.broadcast_to(o["tariff_final"], kwh.shape).copy()
    for i in np.nonzero(c["sw_storage_cnt"] > 0)[0]:
        rows = sw[int(c["sw_storage_off"][i]):int(c["sw_storage_off"][i]) + int(c["sw_storage_cnt"][i])]
        for k in range(kwh.shape[0]):
            hits = [r for r in rows if bank[k, i] > 0.0 and float(r["min_kw"]) <= bank[k, i] < float(r["max_kw"])]
            if len(hits) == 1:
                tar[k, i] = int(hits[0]["tariff"])
    return tar


def net_points(pop, o, tar):
    """[K, n]: the points dgen_batt_curve_net covers (valid kwh assumed; no demand charge billed)."""
    t = pop.tariffs
    return (np.isin(t["mo"][tar], (2, 3)) & ~np.isin(t["unit"][tar], (1, 3))
            & np.broadcast_to((o["status"] & UNSIZED) == 0, tar.shape))


def ts_agents(pop, tar):
    c = pop.cols
    return ((pop.tariffs["mo"][tar] == 2) & np.broadcast_to(((c["flags"] & 2) == 0) & (c["wholesale_row"] >= 0), tar.shape)
            & (pop.wholesale is not None))


def mixed_counts(opop, cfg, i, kw_star, dkwh, dkw):
    """[12] mixed hours per month of one point, by the kernel's classification over [s_N, 1] on the
    oracle's dispatch."""
    a = opop.agents[i]
    load, pv, _ = agent_hours(a, kw_star)
    bank, power = orc.batt_size(dkw, dkwh, 240.0 if a.is_res else 500.0, cfg)
    sysgen, _ = orc.batt_dispatch(load, pv, bank, power, cfg)
    base, s_n = 1.0 - (a.pv_deg * 100.0) * 0.01, 1.0
    for _ in range(int(a.econ_life) - 1):
        s_n = s_n * base
    lo, hi = min(s_n, 1.0), max(s_n, 1.0)
    vlo, vhi = load - sysgen * lo, load - sysgen * hi
    slack = 1e-10 * (np.abs(load) + np.abs(sysgen) * hi)
    imp = np.minimum(vlo, vhi) > -slack
    exq = ~imp & (np.maximum(vlo, vhi) < -slack)
    return np.bincount(MON[~imp & ~exq], minlength=12)


def worst_months(opop, cfg, o, kwh, kw=None):
    K, n = kwh.shape
    w = np.zeros((K, n), np.int64)
    for k in range(K):
        for i in range(n):
            p = kwh[k, i] / 2.0 if kw is None else kw[k, i]
            w[k, i] = mixed_counts(opop, cfg, i, float(o["system_kw"][i]), float(kwh[k, i]), float(p)).max()
    return w


@pytest.fixture(scope="module")
def ca_case(engine):
    """65 CA agents sized once on the device, their K = 3 curve after both calls, dgen_batt_curve_net
    alone on sentinel buffers, curve_ref and the CPU's mixed-hour counts (computed once, shared)."""
    pop = bc._pop("ca_res_storage", 65, CA_SEED)
    bc._load(engine, pop)
    batch, out, o = bc._size(engine, pop)
    assert (o["status"] == 0).all()
    assert (pop.tariffs["mo"][o["tariff_final"]] == 2).all() and (pop.cols["flags"] & 2).all()   # option 2, no TS rate
    kwh = _points(o)
    dev = bc._host(engine.batt_curve(batch, out, kwh, net=True))
    raw = _net_raw(engine, batch, out, kwh)
    opop, cfg_o = _opop(pop), orc.make_cfg()
    ref = curve_ref_points(pop, opop, cfg_o, o, kwh)
    worst = worst_months(opop, cfg_o, o, kwh)
    print(f"ca_res_storage n=65 K=3: worst month holds {worst.max()} mixed hours")
    assert worst.max() <= _lib.NB_CAPM
    return {"pop": pop, "batch": batch, "out": out, "o": o, "kwh": kwh, "dev": dev, "raw": raw, "ref": ref,
            "opop": opop, "cfg_o": cfg_o, "worst": worst}


@pytest.mark.parametrize("n", (1, 63, 65))
def test_ca_curve_matches_curve_ref(engine, ca_case, n):
    pop, o = ca_case["pop"], ca_case["o"]
    if n == 65:
        dev, raw = ca_case["dev"], ca_case["raw"]
    else:
        sub = subset(pop, np.arange(n))
        bc._load(engine, pop)
        batch, out, os_ = bc._size(engine, sub)
        assert np.array_equal(os_["system_kw"], o["system_kw"][:n]) and (os_["status"] == 0).all()
        dev = bc._host(engine.batt_curve(batch, out, ca_case["kwh"][:, :n], net=True))
        raw = _net_raw(engine, batch, out, ca_case["kwh"][:, :n])
    assert (dev["status"] == 0).all()            # every point computed after both calls
    assert _written(raw).all()                   # and all of them by the net-billing entry
    _same_bits(raw, dev, np.ones(raw["npv"].shape, bool), "net alone vs both calls")
    ref = {k: v[:, :n] for k, v in ca_case["ref"].items()}
    bc.compare(dev, ref, f"ca_res_storage n={n} K=3 2 h")
    assert (dev["bank_kwh"] > 0).all()
    if n > 1:
        assert (dev["npv"][0] != dev["npv"][2]).all()


def test_metering_mix_fill_in(engine):
    pop = bc._pop("metering_mix", 65, MIX_SEED)
    bc._load(engine, pop)
    batch, out, o = bc._size(engine, pop)
    assert ((o["status"] & (_lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS)) == 0).all()
    kwh = _points(o)
    kwh = np.where(np.isfinite(kwh), kwh, 1.0)
    both = bc._host(engine.batt_curve(batch, out, kwh, net=True))
    plain = bc._host(engine.batt_curve(batch, out, kwh))
    raw = _net_raw(engine, batch, out, kwh)
    tar = point_tariffs(pop, o, kwh)
    net = net_points(pop, o, tar)
    # options 2 and 3 and the TS sell rate are all reached (from the columns)
    ts = ts_agents(pop, tar) & net
    assert set(pop.tariffs["mo"][tar[net]]) == {2, 3} and ts.any() and (net & ~ts & (pop.tariffs["mo"][tar] == 2)).any()
    print(f"metering_mix: {int(net[0].sum())} net-billing agents, {int(ts[0].sum())} on the TS sell rate")
    # the entry wrote exactly the option 2 / 3 points, nothing else
    assert np.array_equal(_written(raw), net)
    _same_bits(raw, both, net, "net points")
    # the bins points are a plain dgen_batt_curve call's bits
    _same_bits(both, plain, ~net, "bins points")
    assert ((plain["status"][net] & _lib.ST_HOURLY_FORM) != 0).all()
    # what stays flagged: kWh/kW tier units and the agents the sizing call flagged for them
    flagged = (both["status"] & _lib.ST_HOURLY_FORM) != 0
    want = np.isin(pop.tariffs["unit"][tar], (1, 3)) | np.broadcast_to((o["status"] & _lib.ST_UNIT) != 0, tar.shape)
    assert np.array_equal(flagged, want)
    keep = ~flagged
    assert (both["status"][keep] == 0).all() and net.any() and (keep & ~net).any()
    ref = curve_ref_points(pop, _opop(pop), orc.make_cfg(), o, np.where(keep, kwh, 0.0))
    bc.compare(both, ref, "metering_mix n=65 K=3 (all covered points)", keep=keep)
    bc.compare(both, ref, "metering_mix net-billing points", keep=net)
    bc.compare(both, ref, "metering_mix TS sell rate points", keep=ts)
    bc.compare(both, ref, "metering_mix option 3 points", keep=net & (pop.tariffs["mo"][tar] == 3))


def test_one_and_four_hour_banks_and_no_bank(engine, ca_case):
    pop, batch, out, o = ca_case["pop"], ca_case["batch"], ca_case["out"], ca_case["o"]
    bc._load(engine, pop)
    e = o["system_kw"] / 0.8
    kwh = np.stack([np.zeros_like(e), e, e])
    kw = np.stack([np.ones_like(e), e / 1.0, e / 4.0])       # kwh = 0: the power is not read
    dev = bc._host(engine.batt_curve(batch, out, kwh, kw, net=True))
    assert (dev["status"] == 0).all()
    ref = curve_ref_points(pop, ca_case["opop"], ca_case["cfg_o"], o, kwh, kw)
    bc.compare(dev, ref, "ca_res_storage n=65 no bank / 1 h / 4 h")
    two = ca_case["dev"]
    assert np.array_equal(dev["bank_kwh"][1], two["bank_kwh"][1]) and not np.array_equal(dev["power_kw"][1], dev["power_kw"][2])
    # (a residential bank rarely meets its power limit: the 1 h bank's economics may equal the 2 h bank's)
    assert not np.array_equal(dev["npv"][2], dev["npv"][0])
    # no bank: no switch, the PV-only net-billing economics at the combined capex
    c = pop.cols
    assert (dev["bank_kwh"][0] == 0).all() and (dev["power_kw"][0] == 0).all()
    assert np.array_equal(dev["tariff"][0], o["tariff_final"]) and np.array_equal(dev["switched"][0], o["switched"])
    assert np.array_equal(dev["total_cost"][0], ((c["capex_combined"] * o["system_kw"] + 0.0) * c["ccm"]) + 0.0 + 0.0)


def test_storage_switch_across_forms(engine):
    """Hand-set storage rows that only the 2 x point's bank reaches: half of the NEM agents move onto a
    net-billing tariff there (computed by the net entry only), half of the net-billing agents move onto a
    bins tariff (left to dgen_batt_curve)."""
    pop = bc._pop("metering_mix", 48, MIX_SEED + 1)
    c, t = pop.cols, pop.tariffs
    bc._load(engine, pop)
    _, _, o0 = bc._size(engine, pop)
    ok_unit = ~np.isin(t["unit"], (1, 3))
    net_t = np.nonzero(np.isin(t["mo"], (2, 3)) & ok_unit)[0]
    bin_t = np.nonzero(np.isin(t["mo"], (0, 1, 4)) & ok_unit)[0]
    assert net_t.size and bin_t.size
    kwh = _points(o0)
    kwh = np.where(np.isfinite(kwh), kwh, 1.0)
    bank = point_banks(pop, o0, kwh)
    is_net0 = np.isin(t["mo"][o0["tariff_final"]], (2, 3))
    rows, off, cnt = [r for r in pop.switches], c["sw_storage_off"].copy(), c["sw_storage_cnt"].copy()
    sized = ((o0["status"] & UNSIZED) == 0) & ok_unit[o0["tariff_final"]]
    for j, i in enumerate(np.nonzero(sized)[0]):
        if j % 2 or not (bank[2, i] > bank[1, i] > 0.0):
            continue
        rec = np.zeros((), dtype=SWITCH_DTYPE)
        rec["min_kw"], rec["max_kw"], rec["one_time_charge"] = 0.5 * (bank[1, i] + bank[2, i]), 1e9, 25.0 + j
        tgt = bin_t if is_net0[i] else net_t
        rec["tariff"] = tgt[j % tgt.size]
        off[i], cnt[i] = len(rows), 1
        rows.append(rec)
    pop.switches = np.stack(rows).astype(SWITCH_DTYPE)
    c["sw_storage_off"], c["sw_storage_cnt"] = off, cnt
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    bc._load(engine, pop)
    batch, out, o = bc._size(engine, pop)
    assert np.array_equal(o["system_kw"], o0["system_kw"], equal_nan=True)
    assert np.array_equal(o["tariff_final"], o0["tariff_final"])          # the reference's bank misses every row
    tar = point_tariffs(pop, o, kwh)
    net = net_points(pop, o, tar)
    to_net = net & ~np.broadcast_to(is_net0, net.shape) & (tar != o["tariff_final"])
    to_bins = ~net & np.broadcast_to(is_net0 & sized, net.shape) & (tar != o["tariff_final"])
    assert to_net.any() and to_bins.any(), "the rows do not cross the forms both ways"
    both = bc._host(engine.batt_curve(batch, out, kwh, net=True))
    plain = bc._host(engine.batt_curve(batch, out, kwh))
    raw = _net_raw(engine, batch, out, kwh)
    assert np.array_equal(_written(raw), net)
    assert ((plain["status"][to_net] & _lib.ST_HOURLY_FORM) != 0).all() and (both["status"][to_net] == 0).all()
    assert (plain["status"][to_bins] == 0).all()
    _same_bits(both, plain, ~net, "points the net entry leaves alone")
    assert (both["switched"][to_net | to_bins] == 1).all()
    keep = (both["status"] & _lib.ST_HOURLY_FORM) == 0
    assert (both["status"][keep] == 0).all()
    ref = curve_ref_points(pop, _opop(pop), orc.make_cfg(), o, np.where(keep, kwh, 0.0))
    assert np.array_equal(ref["tariff"][keep], tar[keep])
    bc.compare(both, ref, "storage switch across forms n=48 K=3", keep=keep)
    bc.compare(both, ref, "switched onto net billing", keep=to_net)


def test_degradation_and_life_edges(engine):
    pop = bc._pop("ca_res_storage", 64, CA_SEED)
    c = pop.cols
    deg, life = c["pv_deg"].copy(), c["econ_life"].copy()
    deg[0:16] = 0.0                  # the range collapses
    life[16:32] = 1
    life[32:48] = 50
    deg[48:64], life[48:64] = 0.05, 32          # s_N ~ 0.2: long lists
    c["pv_deg"], c["econ_life"] = deg, life
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    bc._load(engine, pop)
    batch, out, o = bc._size(engine, pop)
    assert (o["status"] == 0).all()
    kwh = _points(o)
    opop, cfg_o = _opop(pop), orc.make_cfg()
    worst = worst_months(opop, cfg_o, o, kwh)
    fits = worst <= _lib.NB_CAPM
    print("edges: worst month per group", [int(worst[:, a:a + 16].max()) for a in (0, 16, 32, 48)],
          f"{int(fits[:, 48:].sum())} of {fits[:, 48:].size} long-list points within the cap")
    assert fits[:, :48].all() and fits[:, 48:].any() and worst[:, 48:].max() > worst[:, :48].max()
    dev = bc._host(engine.batt_curve(batch, out, kwh, net=True))
    assert (dev["status"][fits] == 0).all()
    ref = curve_ref_points(pop, opop, cfg_o, o, kwh)
    for name, a in (("pv_deg = 0", 0), ("life 1", 16), ("life 50", 32), ("pv_deg = 0.05, life 32", 48)):
        keep = fits.copy()
        keep[:, :a] = False
        keep[:, a + 16:] = False
        bc.compare(dev, ref, f"edges: {name}", keep=keep)


def test_forced_overflow_leaves_points_unwritten(engine, ca_case):
    """cap = 2.  At the reference's bank every agent has a month with more mixed hours; a bank four or
    eight times as large takes the whole PV surplus of about half of the agents (their near-zero battery
    hours count as imports), so points of both kinds exist."""
    pop, batch, out, o = ca_case["pop"], ca_case["batch"], ca_case["out"], ca_case["o"]
    bc._load(engine, pop)
    kwh = np.stack([f * (o["system_kw"] / 0.8) for f in (1.0, 4.0, 8.0)])
    over = worst_months(ca_case["opop"], ca_case["cfg_o"], o, kwh) > 2
    assert over.any() and (~over).any(), (int(over.sum()), over.size)
    full = _net_raw(engine, batch, out, kwh)
    assert _written(full).all()
    raw = _net_raw(engine, batch, out, kwh, cap=2)
    assert np.array_equal(_written(raw), ~over)
    _same_bits(raw, full, ~over, "cap = 2 vs the default cap")
    # through the engine: the overflowed points stay flagged by dgen_batt_curve
    dev = bc._host(engine.batt_curve(batch, out, kwh, net=True, net_cap=2))
    assert np.array_equal((dev["status"] & _lib.ST_HOURLY_FORM) != 0, over)
    assert np.isnan(dev["npv"][over]).all() and (dev["status"][~over] == 0).all()


def test_independence_and_identity(engine, ca_case):
    pop, batch, out, o, kwh, dev = (ca_case[k] for k in ("pop", "batch", "out", "o", "kwh", "dev"))
    bc._load(engine, pop)
    again = bc._host(engine.batt_curve(batch, out, kwh, net=True))
    _same_bits(again, dev, np.ones(kwh.shape, bool), "repeat call")
    for p in range(len(FRACS)):
        one = _net_raw(engine, batch, out, kwh[p])
        for k in _lib.BATT_CURVE_FIELDS:
            assert one[k].shape == (1, batch.n) and np.array_equal(one[k][0], dev[k][p]), (p, k)
    named = ("npv", "switched")
    part = _net_raw(engine, batch, out, kwh, names=named)
    for k in _lib.BATT_CURVE_FIELDS:             # NULL members are not written
        assert np.array_equal(part[k], dev[k]) if k in named else (part[k] == SENT).all(), k
    # the reference's point against the sizing call
    k = FRACS.index(1.0)
    assert np.array_equal(dev["bank_kwh"][k], o["batt_kwh"]) and np.array_equal(dev["tariff"][k], o["tariff_final"])
    assert np.allclose(dev["npv"][k], o["npv_pv_batt"], rtol=bc.RTOL, atol=bc.ATOL)
    assert np.allclose(dev["bill_w_year1"][k], o["bill_w_batt"][:, 1], rtol=bc.RTOL, atol=bc.ATOL)
    print("reference point vs sizing call: worst relative npv",
          float((np.abs(dev["npv"][k] - o["npv_pv_batt"]) / np.maximum(np.abs(o["npv_pv_batt"]), 1.0)).max()))


def test_arguments(engine, engine_hourly_plan, ca_case):
    pop, batch, out = ca_case["pop"], ca_case["batch"], ca_case["out"]
    bc._load(engine, pop)
    n = batch.n
    for K in (0, 17):
        with pytest.raises(_lib.DgenError):
            engine.batt_curve(batch, out, np.ones((K, n)), net=True)
    e = torch.ones((17, n), dtype=torch.float64, device=engine.dev)
    bo, no = _lib.BattCurveOut(), _lib.BattNetOpt(0, 0)

    def call(eng, b, o_, n_, K, kwh, opt=no):
        co = eng.c_outputs(o_)
        return eng.lib.dgen_batt_curve_net(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(b.c_agents), ctypes.byref(co),
                                           n_, K, kwh, None, None if opt is None else ctypes.byref(opt),
                                           ctypes.byref(bo), eng.stream_handle())
    for K in (0, 17, -1):
        assert call(engine, batch, out, n, K, e.data_ptr()) == -1
        assert "dgen_batt_curve_net" in _lib.last_error()
    assert call(engine, batch, out, n, 1, None) == -1
    assert call(engine, batch, out, 0, 1, e.data_ptr()) == 0
    assert call(engine, batch, out, 0, 1, e.data_ptr(), opt=None) == 0
    assert call(engine, batch, out, n, 1, e.data_ptr(), opt=_lib.BattNetOpt(_lib.NB_CAPM + 1, 0)) == -1
    # the hourly re-plan is not replayed
    eng = engine_hourly_plan
    bc._load(eng, pop)
    sub = subset(pop, np.arange(4))
    b4 = eng.upload_agents(sub.cols, sub.n_scratch)
    o4 = eng.alloc_outputs(4, hourly=False)
    e4 = torch.ones((1, 4), dtype=torch.float64, device=eng.dev)
    assert call(eng, b4, o4, 4, 1, e4.data_ptr()) == -1 and "dgen_batt_curve_net" in _lib.last_error()
    with pytest.raises(_lib.DgenError):
        eng.batt_curve(b4, o4, np.ones((1, 4)), net=True)


def test_drop_in_switch_with_net_billing(engine):
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    spec = {"pv_to_batt": (0.4, 1.6), "hours": (1.0, 4.0), "net_billing": True}
    bins = {k: v for k, v in spec.items() if k != "net_billing"}
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec)
    arr, _ = ff.size_chunk(df, None, table, "simple", hourly="array", batt_sizing=spec)
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec, max_rows=64)
    old, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=bins)
    off, _ = ff.size_chunk(df, None, table, "simple", hourly="none")
    assert list(non.columns) == list(old.columns) and list(non.columns)[-7:] == list(bs.COLUMNS)
    for c in off.columns:                        # the frame's other columns: the bits of a call without the option
        a, b = off[c].to_numpy(), non[c].to_numpy()
        if a.dtype.kind in "fiu":
            assert np.array_equal(a, b, equal_nan=True), c
        else:
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)), c
    for c in bs.COLUMNS:
        a = non[c].to_numpy()
        assert np.array_equal(a, arr[c].to_numpy(), equal_nan=True), c
        assert np.array_equal(a, sub[c].to_numpy(), equal_nan=True), c
    ca = (df["state_abbr"] == "CA").to_numpy()
    pt, pt_old = non["batt_opt_point"].to_numpy(), old["batt_opt_point"].to_numpy()
    assert ca.any() and (pt_old[ca] == -1).all() and (pt[ca] >= 0).all()
    assert (non["batt_opt_status"].to_numpy()[ca] & bs.INVALID == 0).all()
    had = pt_old >= 0                            # the agents the key-less call already valued keep their bits
    for c in bs.COLUMNS:
        assert np.array_equal(non[c].to_numpy()[had], old[c].to_numpy()[had], equal_nan=True), c
