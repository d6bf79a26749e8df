"""The demand-charge and kWh/kW tariffs of the PV search on the with-battery
objective on the GPU (dgen_size_with_batt, dgen_size_with_batt_net, then
dgen_size_with_batt_peak).

The yardsticks are the existing kernels: every traced evaluation and every
member at system_kw is the point of Engine.batt_curve(net=True, peak=True),
K = 1, on a hand-made sized batch at the traced x, bit for bit; the search is
scipy's bounded minimiser replayed over the device's own trace; the written set
is tests/test_size_with_batt_peak.candidates_peak; the point at system_kw is
compared with curve_ref (the oracle's hourly bills and month peaks).

Worst relative differences against curve_ref (MI355X): see DESIGN.md section 5."""
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
from tests.test_batt_sizing import _opop
from tests.test_batt_sizing_peak import kept_counts
from tests.test_gpu_batt_curve import compare
from tests.test_gpu_batt_curve_net import mixed_counts, ts_agents
from tests.test_gpu_batt_curve_peak import _mix_dc_pop
from tests.test_gpu_size_with_batt import (FATAL, POINT, TRACE, _host, _load, _oracle_at, _pop, check_search,
                                           default_bracket, same)
from tests.test_gpu_size_with_batt_net import INFO, MEMBERS, SENT, trace_tariffs
from tests.test_size_with_batt_peak import candidates_peak

pytestmark = pytest.mark.gpu

DC_SEED, KW_SEED, MIX_SEED = 20260031, 20260033, 20260023


def _run(eng, pop, **kw):
    """The three calls through the engine, full trace; device rows are caller rows."""
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    kw.setdefault("net", True)
    kw.setdefault("peak", True)
    return batch, _host(eng.size_with_batt(batch, trace=TRACE, **kw))


def _raw(eng, batch, lo=None, hi=None, caps=(0, 0), blocks=0, names=None, first=True, net=True):
    """The C entries on sentinel-filled buffers: (host members after the earlier calls or None, host
    members after dgen_size_with_batt_peak).  Members `names` leaves out are not handed to any entry."""
    n = batch.n
    bufs = {k: torch.full((n,), float(SENT), dtype=torch.float64, device=eng.dev) for k in _lib.SWB_F64}
    bufs.update({k: torch.full((n,), SENT, dtype=torch.int32, device=eng.dev) for k in _lib.SWB_I32})
    bufs.update({k: torch.full((n, TRACE), float(SENT), dtype=torch.float64, device=eng.dev)
                 for k in ("trace_x", "trace_f")})
    so = _lib.SwbOut(**{k: bufs[k].data_ptr() for k in (MEMBERS if names is None else names)})
    a = None if lo is None else eng._to_dev(np.ascontiguousarray(lo), torch.float64)
    b = None if hi is None else eng._to_dev(np.ascontiguousarray(hi), torch.float64)
    opt, no, po = _lib.SwbOpt(0.8, 2.0, TRACE, 0), _lib.SwbNetOpt(0, 0), _lib.SwbPeakOpt(caps[0], caps[1], blocks, 0)
    args = (eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), n, None if a is None else a.data_ptr(),
            None if b is None else b.data_ptr(), ctypes.byref(opt))
    sh = eng.stream_handle()
    before = None
    if first:
        assert eng.lib.dgen_size_with_batt(*args, ctypes.byref(so), sh) == 0, _lib.last_error()
        if net:
            assert eng.lib.dgen_size_with_batt_net(*args, ctypes.byref(no), ctypes.byref(so), sh) == 0, _lib.last_error()
        before = _host(bufs)
    assert eng.lib.dgen_size_with_batt_peak(*args, ctypes.byref(po), ctypes.byref(so), sh) == 0, _lib.last_error()
    return before, _host(bufs)


def curve_at(eng, pop, batch, x, ratio, hours, caps=None):
    """Engine.batt_curve(net=True, peak=True), K = 1, of a hand-made sized batch: system_kw = x from
    (tariff0, not switched, status 0), kwh = x / ratio, kw = kwh / hours, the fill-ins at the same caps."""
    out = eng.alloc_outputs(batch.n, hourly=False)
    out["system_kw"].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    out["tariff_final"].copy_(torch.from_numpy(np.ascontiguousarray(pop.cols["tariff0"], np.int32)))
    out["switched"].zero_()
    out["status"].zero_()
    kwh = x / ratio
    d = _host(eng.batt_curve(batch, out, kwh, kwh / hours, net=True, net_cap=None if caps is None else caps[0],
                             peak=True, peak_caps=caps))
    return {k: v[0] for k, v in d.items()}


def check_objective(eng, pop, batch, r, ratio=0.8, hours=2.0, caps=None):
    """tests/test_gpu_size_with_batt_net.check_objective with the third call added: every traced
    evaluation is the point of the three what-if calls, and so is every member at system_kw; returns the
    valued agents."""
    n = batch.n
    tx, tf, nfev = r["trace_x"], r["trace_f"], r["nfev"]
    assert tx.shape == tf.shape == (n, TRACE)
    col = np.arange(TRACE)[None, :]
    assert np.isnan(tx[col >= nfev[:, None]]).all() and np.isnan(tf[col >= nfev[:, None]]).all()
    assert not np.isnan(tx[col < np.minimum(nfev, TRACE)[:, None]]).any()
    for k in range(int(min(nfev.max(initial=0), TRACE))):
        live = nfev > k
        c = curve_at(eng, pop, batch, np.where(live, tx[:, k], 1.0), ratio, hours, caps)
        val = live & ((c["status"] & FATAL) == 0)
        assert same((-c["npv"])[val], tf[val, k]), f"evaluation {k}"
        assert np.isnan(tf[live & ~val, k]).all(), f"evaluation {k}"
        last = live & ~val                       # an evaluation that cannot be valued is the agent's last
        assert (nfev[last] == k + 1).all() and ((r["status"][last] & _lib.ST_HOURLY_FORM) != 0).all(), f"evaluation {k}"
        assert np.array_equal(r["tariff"][last], c["tariff"][last]), f"evaluation {k}"
        assert np.array_equal(r["switched"][last], c["switched"][last]), f"evaluation {k}"
    ok = (r["status"] & FATAL) == 0
    assert (nfev[ok] >= 1).all()
    c = curve_at(eng, pop, batch, np.where(ok, r["system_kw"], 1.0), ratio, hours, caps)
    for m in POINT:
        if m == "status":
            assert np.array_equal(r[m][ok] & ~INFO, c[m][ok]), m
        else:
            assert same(r[m][ok], c[m][ok]), m
    if ok.any():
        assert same(np.nanmin(tf[ok], axis=1), -r["npv"][ok])
    for m in _lib.SWB_F64:
        assert np.isnan(r[m][~ok]).all() and not np.isnan(r[m][ok]).any(), m
    return ok


def peak_tariffs(eng, dc_on):
    """[n_tariffs] bool: the tariffs of peak form as the engine holds them."""
    t = eng.tariff_records
    return np.isin(t["unit"], (1, 3)) | (bool(dc_on) & (t["dc"] > 0))


def list_counts(pop, opop, cfg_o, i, x, tariff, ratio=0.8, hours=2.0):
    """(worst month's kept hours, worst month's mixed hours -- 0 on a bins-form tariff) of agent i's
    evaluation at x billed under `tariff`, counted on the CPU."""
    a = (opop, cfg_o, int(i), float(x), float(x) / ratio, float(x) / ratio / hours)
    kept = int(kept_counts(*a, int(tariff)).max())
    mixed = int(mixed_counts(*a).max()) if pop.tariffs["mo"][tariff] in (2, 3) else 0
    return kept, mixed


def _banks(pop, x, ratio=0.8, hours=2.0):
    cfg_o, c = orc.make_cfg(), pop.cols
    return np.array([orc.batt_size(float(v) / ratio / hours, float(v) / ratio, 240.0 if c["flags"][i] & 1 else 500.0,
                                   cfg_o)[0] for i, v in enumerate(x)])


@pytest.fixture(scope="module")
def dc_case(engine_dc):
    """129 com_dc_batt agents (three tiles) on the demand-charge engine, searched once with the full
    trace after the three calls and after the first two alone (shared, not modified)."""
    eng = engine_dc
    pop = _pop("com_dc_batt", 129, DC_SEED)
    _load(eng, pop)
    lo, hi = default_bracket(eng, pop)
    # on the CPU, ahead of the GPU comparison: no month beyond the default caps at the bracket's ends
    opop, cfg_o = _opop(pop), orc.make_cfg()
    worst_k = worst_m = 0
    for i in range(0, 129, 8):
        for x in (lo[i], hi[i]):
            k, m = list_counts(pop, opop, cfg_o, i, x, pop.cols["tariff0"][i])
            worst_k, worst_m = max(worst_k, k), max(worst_m, m)
    print(f"com_dc_batt: worst month at the bracket's ends keeps {worst_k} hours, holds {worst_m} mixed hours")
    assert worst_k <= _lib.BATT_PEAK_CAPK and worst_m <= _lib.NB_CAPM
    batch, r = _run(eng, pop)
    _, two = _run(eng, pop, peak=False)
    return {"pop": pop, "batch": batch, "r": r, "two": two, "lo": lo, "hi": hi, "opop": opop, "cfg_o": cfg_o}


def test_demand_charge_objective_and_search(engine_dc, dc_case):
    eng = engine_dc
    pop, batch, r, two, lo, hi = (dc_case[k] for k in ("pop", "batch", "r", "two", "lo", "hi"))
    _load(eng, pop)
    assert candidates_peak(eng.tariff_records, pop, lo, hi, True).all()         # every agent is a candidate
    # none was valued by the first two calls: each ended at its first evaluation
    assert ((two["status"] & _lib.ST_HOURLY_FORM) != 0).all() and (two["nfev"] == 1).all()
    for k in _lib.SWB_FIELDS:
        assert r[k].shape == (129,) and r[k].dtype == (np.float64 if k in _lib.SWB_F64 else np.int32), k
    assert ((r["status"] & FATAL) == 0).all(), np.unique(r["status"])
    ok = check_objective(eng, pop, batch, r)
    assert ok.all() and (r["bank_kwh"] > 0).all()
    assert check_search(r, lo, hi).all()
    print("com_dc_batt n=129 nfev:", np.bincount(r["nfev"]))
    assert same(r["trace_x"][:, 0], two["trace_x"][:, 0])
    _, e = _run(eng, pop, lo=lo, hi=hi)          # the default bracket: the bits of the explicit one
    for k, v in e.items():
        assert same(v, r[k]), k


@pytest.mark.parametrize("n", (1, 63, 65))
def test_agents_do_not_depend_on_the_batch(engine_dc, dc_case, n):
    _load(engine_dc, dc_case["pop"])
    _, s = _run(engine_dc, subset(dc_case["pop"], np.arange(n)))
    for k, v in s.items():
        assert same(v, dc_case["r"][k][:n]), k


def test_grid_stride(engine_dc, dc_case):
    """Three tiles through one block's slice (peak_blocks = 1), a ragged stride (2) and the default launch."""
    _load(engine_dc, dc_case["pop"])
    for blocks in (1, 2):
        got = _host(engine_dc.size_with_batt(dc_case["batch"], trace=TRACE, net=True, peak=True, peak_blocks=blocks))
        for k, v in got.items():
            assert same(v, dc_case["r"][k]), (blocks, k)


@pytest.fixture(scope="module")
def kw_case(engine):
    """65 com_kwkw agents in the reference's mode (demand charges not billed): the raw C entries on
    sentinel-filled buffers."""
    pop = _pop("com_kwkw", 65, KW_SEED)
    _load(engine, pop)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    two, three = _raw(engine, batch)
    lo, hi = default_bracket(engine, pop)
    return {"pop": pop, "batch": batch, "two": two, "three": three, "lo": lo, "hi": hi,
            "cand": candidates_peak(engine.tariff_records, pop, lo, hi, False)}


def test_kwh_per_kw_fill_in(engine, kw_case):
    pop, batch, two, three, cand = (kw_case[k] for k in ("pop", "batch", "two", "three", "cand"))
    _load(engine, pop)
    t = engine.tariff_records
    assert pop.skip_demand_charges == 1 and cand.any() and (~cand).any()
    # alone on sentinel buffers the entry writes exactly the candidates, every member of them
    _, alone = _raw(engine, batch, first=False)
    for k in MEMBERS:
        w = alone[k] != SENT
        w = w.all(axis=1) if w.ndim == 2 else w
        assert np.array_equal(w, cand), k
        assert np.array_equal((alone[k] == SENT).all(axis=1) if alone[k].ndim == 2 else alone[k] == SENT, ~cand), k
        assert same(alone[k][cand], three[k][cand]), k
        assert same(three[k][~cand], two[k][~cand]), k          # every other element: the earlier calls' bits
    ok = check_objective(engine, pop, batch, three)
    check_search(three, kw_case["lo"], kw_case["hi"])
    assert ok[cand].all() and ((two["status"][cand] & _lib.ST_HOURLY_FORM) != 0).all()
    netc = cand & np.isin(t["mo"][three["tariff"]], (2, 3))
    print(f"com_kwkw n=65: {int(cand.sum())} candidates, {int(netc.sum())} of them valued on net-billing tariffs")
    assert netc.any()
    # the DGEN_ST_UNIT agents stay flagged, unsearched; nothing else is flagged
    unit = (t["flags"][pop.cols["tariff0"]] & _lib.ST_UNIT) != 0
    flagged = (three["status"] & _lib.ST_HOURLY_FORM) != 0
    assert np.array_equal(flagged, unit) and (three["nfev"][unit] == 0).all()


@pytest.fixture(scope="module")
def mix_case(engine_dc):
    eng = engine_dc
    pop = _mix_dc_pop(65, MIX_SEED)
    _load(eng, pop)
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    two, three = _raw(eng, batch)
    lo, hi = default_bracket(eng, pop)
    return {"pop": pop, "batch": batch, "two": two, "three": three, "lo": lo, "hi": hi,
            "cand": candidates_peak(eng.tariff_records, pop, lo, hi, True)}


def test_metering_mix_with_demand_charges(engine_dc, mix_case):
    eng = engine_dc
    pop, batch, two, three, cand = (mix_case[k] for k in ("pop", "batch", "two", "three", "cand"))
    _load(eng, pop)
    t = eng.tariff_records
    for k in MEMBERS:                            # non-candidates keep the two-call bits
        assert same(three[k][~cand], two[k][~cand]), k
    _, alone = _raw(eng, batch, first=False)
    for k in MEMBERS:
        w = alone[k] != SENT
        assert np.array_equal(w.all(axis=1) if w.ndim == 2 else w, cand), k
        assert same(alone[k][cand], three[k][cand]), k
    ok = check_objective(eng, pop, batch, three)
    check_search(three, mix_case["lo"], mix_case["hi"])
    mo0 = t["mo"][pop.cols["tariff0"]]
    print(f"metering_mix + demand n=65: candidates per option {[int((cand & (mo0 == m)).sum()) for m in range(5)]}, "
          f"valued {[int((cand & ok & (mo0 == m)).sum()) for m in range(5)]}, "
          f"{int((ts_agents(pop, three['tariff']) & cand & ok).sum())} on the TS rate")
    assert set(mo0[cand]) == set(mo0) and set(mo0[cand & ok]) == set(mo0)
    assert (ts_agents(pop, three["tariff"]) & cand & ok).any()
    # flagged after the three calls: the DGEN_ST_UNIT agents (never searched) and the candidates whose
    # last evaluation the CPU counts beyond a cap
    unit = (t["flags"][pop.cols["tariff0"]] & _lib.ST_UNIT) != 0
    flagged = (three["status"] & FATAL) != 0
    assert not (flagged & ~cand & ~unit & ((two["status"] & FATAL) == 0)).any()
    opop, cfg_o = _opop(pop), orc.make_cfg()
    tar = trace_tariffs(pop, three)
    for i in np.nonzero(flagged & cand)[0]:
        k = int(three["nfev"][i]) - 1
        assert three["tariff"][i] == tar[k, i], i
        kept, mixed = list_counts(pop, opop, cfg_o, i, three["trace_x"][i, k], tar[k, i])
        assert kept > _lib.BATT_PEAK_CAPK or mixed > _lib.NB_CAPM, (i, k, kept, mixed)
    assert (cand & ok).sum() * 2 >= cand.sum()


def test_against_the_oracle(engine_dc, engine, dc_case, kw_case):
    r = dc_case["r"]
    rows = np.arange(65)
    _load(engine_dc, dc_case["pop"])
    compare({k: r[k][rows] for k in POINT}, _oracle_at(dc_case["pop"], r, rows), "size_with_batt_peak com_dc_batt n=65")
    pop, three = kw_case["pop"], kw_case["three"]
    rows = np.nonzero(kw_case["cand"] & ((three["status"] & FATAL) == 0))[0]
    assert rows.size
    compare({k: three[k][rows] for k in POINT}, _oracle_at(pop, three, rows), "size_with_batt_peak com_kwkw candidates")


def test_storage_switch_across_forms(engine_dc):
    """Hand-set storage rows whose edge lies between the banks of the bracket's ends: searches billed
    under bins and peak, under net and peak, under all three (three rows), and candidates whose row lies
    beyond the bracket (never billed under the peak form)."""
    eng = engine_dc
    pop = _mix_dc_pop(64, MIX_SEED + 1)
    c, t = pop.cols, pop.tariffs
    _load(eng, pop)
    lo, hi = default_bracket(eng, pop)
    plain = ~np.isin(t["unit"], (1, 3))
    pk_t = np.nonzero((t["dc"] > 0) & plain)[0]
    net_t = np.nonzero((t["dc"] == 0) & plain & np.isin(t["mo"], (2, 3)))[0]
    bin_t = np.nonzero((t["dc"] == 0) & plain & np.isin(t["mo"], (0, 1, 4)))[0]
    assert pk_t.size and net_t.size and bin_t.size
    b_lo, b_hi = _banks(pop, np.where(lo > 0, lo, 1.0)), _banks(pop, np.where(lo > 0, hi, 2.0))
    nopk0 = np.isin(c["tariff0"], np.concatenate([net_t, bin_t])) & (lo > 0) & (b_hi > b_lo) & (b_lo > 0)
    recs, beyond = {}, np.zeros(64, bool)
    extra = []
    for j, i in enumerate(np.nonzero(nopk0)[0]):
        rec = np.zeros((), dtype=SWITCH_DTYPE)
        rec["one_time_charge"], rec["tariff"] = 25.0 + j, pk_t[j % pk_t.size]
        mid = 0.5 * (b_lo[i] + b_hi[i])
        if j % 3 == 0:                           # tariff0's form below the edge, the peak form above
            rec["min_kw"], rec["max_kw"] = mid, 1e9
        elif j % 3 == 1:
            # three forms whichever way the search turns: the minimiser's first two requests lie at 0.382
            # and 0.618 of the bracket, its third at 0.236 or 0.764.  Banks below 0.30 of the way and from
            # 0.70 on bill under tariff0 (the last through a row onto tariff0 itself), 0.30 .. 0.50 under
            # the other plain form, 0.50 .. 0.70 under the peak form
            at = lambda f: b_lo[i] + f * (b_hi[i] - b_lo[i])
            rec["min_kw"], rec["max_kw"] = at(0.50), at(0.70)
            tgt = bin_t if c["tariff0"][i] in net_t else net_t
            for lo_f, hi_kw, tt in ((0.30, at(0.50), tgt[j % tgt.size]), (0.70, 1e9, c["tariff0"][i])):
                other = np.zeros((), dtype=SWITCH_DTYPE)
                other["min_kw"], other["max_kw"], other["tariff"], other["one_time_charge"] = at(lo_f), hi_kw, tt, 10.0
                extra.append((i, other))
        else:                                    # the row beyond the bracket: a candidate never billed from peaks
            rec["min_kw"], rec["max_kw"] = 2.0 * b_hi[i], 1e9
            beyond[i] = True
        recs[i] = rec
    rows, off, cnt = [r for r in pop.switches], c["sw_storage_off"].copy(), c["sw_storage_cnt"].copy()
    for i, rec in recs.items():
        more = [o for a, o in extra if a == i]
        off[i], cnt[i] = len(rows), 1 + len(more)
        rows.extend([rec] + more)
    pop.switches = np.stack(rows).astype(SWITCH_DTYPE)
    c["sw_storage_off"], c["sw_storage_cnt"] = off, cnt
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    _load(eng, pop)
    batch, r = _run(eng, pop)
    _, two = _run(eng, pop, peak=False)
    cand = candidates_peak(eng.tariff_records, pop, lo, hi, True)
    assert cand[list(recs)].all()
    # from the rows alone, ahead of any comparison: the forms each trace was billed under
    tar = trace_tariffs(pop, r)
    live, ts = tar >= 0, np.maximum(tar, 0)
    pkf = peak_tariffs(eng, True)
    seen_pk = (live & pkf[ts]).any(axis=0)
    seen_net = (live & ~pkf[ts] & np.isin(t["mo"][ts], (2, 3))).any(axis=0)
    seen_bin = (live & ~pkf[ts] & np.isin(t["mo"][ts], (0, 1, 4))).any(axis=0)
    bp, np_, all3, never = (cand & seen_bin & seen_pk & ~seen_net, cand & seen_net & seen_pk & ~seen_bin,
                            cand & seen_bin & seen_net & seen_pk, cand & ~seen_pk)
    print(f"storage switch: {int(bp.sum())} searches under bins and peak, {int(np_.sum())} under net and peak, "
          f"{int(all3.sum())} under all three, {int(never.sum())} candidates never on the peak form")
    assert bp.any() and np_.any() and all3.any() and never.any() and never[beyond].all()
    ok = check_objective(eng, pop, batch, r)
    check_search(r, lo, hi)
    assert ok[never].all()
    for k, v in r.items():                       # never on the peak form: the bits of the first two calls
        assert same(v[never], two[k][never]), k
        assert same(v[~cand], two[k][~cand]), k
    valued = np.nonzero((bp | np_ | all3) & ok)[0]
    assert valued.size
    compare({k: r[k][valued] for k in POINT}, _oracle_at(pop, r, valued), "size_with_batt_peak storage switch across forms")


def test_edges(engine_dc, dc_case):
    eng, pop, base = engine_dc, dc_case["pop"], dc_case["r"]
    _load(eng, pop)
    sub = subset(pop, np.arange(66))
    life, deg = sub.cols["econ_life"].copy(), sub.cols["pv_deg"].copy()
    life[[1, 64]], life[[2, 65]], life[3] = 1, 50, 51
    deg[[4, 5]] = 0.0
    sub.cols["econ_life"], sub.cols["pv_deg"] = life, deg
    batch, r = _run(eng, sub)
    _, two = _run(eng, sub, peak=False)
    assert two["status"][3] == _lib.ST_YEARS and ((np.delete(r["status"], 3) & FATAL) == 0).all()
    for k, v in r.items():                       # a life outside 1 .. MAXY is no candidate
        assert same(v[3:4], two[k][3:4]), k
    check_objective(eng, sub, batch, r)
    rest = np.setdiff1d(np.arange(65), [1, 2, 3, 4, 5, 64])
    for k, v in r.items():                       # the other rows' bits alone
        assert same(v[rest], base[k][rest]), k
    rows = np.array([1, 2, 4, 5, 64, 65])
    compare({k: r[k][rows] for k in POINT}, _oracle_at(sub, r, rows), "size_with_batt_peak lives 1 and 50, pv_deg = 0")
    # a larger, longer bank
    s65, lo, hi = subset(pop, np.arange(65)), dc_case["lo"][:65], dc_case["hi"][:65]
    batch, q = _run(eng, s65, ratio=0.4, hours=4.0)
    assert check_objective(eng, s65, batch, q, 0.4, 4.0).all()
    check_search(q, lo, hi)
    assert not np.array_equal(q["npv"], base["npv"][:65])
    compare({k: q[k][:8] for k in POINT}, _oracle_at(s65, q, np.arange(8), 0.4, 4.0), "size_with_batt_peak 0.4 / 4 h")
    # no battery: the search bills the PV-only peaks
    eng.set_battery(False)
    try:
        batch, z = _run(eng, s65)
        assert ((z["status"] & FATAL) == 0).all() and (z["bank_kwh"] == 0).all() and (z["switched"] == 0).all()
        assert check_objective(eng, s65, batch, z).all()
    finally:
        eng.set_battery(True)
    check_search(z, lo, hi)
    # a bracket 1000 x wider: longer searches, the tolerance above its floor
    lo2, hi2 = lo * 0.25, hi * 1000.0
    assert (np.floor((hi2 - lo2) * 1e-3) > 2.0).all()
    batch, w = _run(eng, s65, lo=lo2, hi=hi2)
    check_search(w, lo2, hi2)
    okw = check_objective(eng, s65, batch, w)
    print("wide bracket nfev:", np.bincount(w["nfev"]), "valued", int(okw.sum()))
    assert okw.any()
    # invalid brackets: the first call's DGEN_ST_BOUNDS, and nothing written by the fill-ins
    lo3, hi3 = lo.copy(), hi.copy()
    bad = [3, 10, 11, 63, 64]
    lo3[3] = hi3[3]
    lo3[10], hi3[10] = hi3[10], lo3[10]
    lo3[11] = np.nan
    hi3[63] = np.inf
    lo3[64] = 0.0
    batch = eng.upload_agents(s65.cols, s65.n_scratch)
    two_, three = _raw(eng, batch, lo=lo3, hi=hi3)
    _, alone = _raw(eng, batch, lo=lo3, hi=hi3, first=False)
    assert (three["status"][bad] == _lib.ST_BOUNDS).all() and (three["nfev"][bad] == 0).all()
    good = np.setdiff1d(np.arange(65), bad)
    for k in MEMBERS:
        assert (alone[k][bad] == SENT).all(), k
        assert same(three[k][bad], two_[k][bad]), k
        assert same(three[k][good], base[k][good]), k


def test_peak_without_net(engine_dc, mix_case):
    """dgen_size_with_batt_peak straight after dgen_size_with_batt: the peak candidates are valued as
    after the three calls, the agents only the net entry searches stay flagged."""
    eng, pop, batch, three, cand = (engine_dc, mix_case["pop"], mix_case["batch"], mix_case["three"], mix_case["cand"])
    _load(eng, pop)
    one, got = _raw(eng, batch, net=False)
    for k in MEMBERS:
        assert same(got[k][cand], three[k][cand]), k
        assert same(got[k][~cand], one[k][~cand]), k
    t = eng.tariff_records
    net_only = ~cand & np.isin(t["mo"][pop.cols["tariff0"]], (2, 3)) & ((one["status"] & _lib.ST_BOUNDS) == 0)
    assert net_only.any() and ((got["status"][net_only] & _lib.ST_HOURLY_FORM) != 0).all()
    assert ((three["status"][net_only] & _lib.ST_HOURLY_FORM) == 0).any()
    via = _host(eng.size_with_batt(batch, trace=TRACE, net=False, peak=True))
    for k, v in via.items():
        assert same(v, got[k]), k


def _forced(eng, pop, base, n, which):
    """The CPU's worst traced month per (evaluation, agent) of the first n agents: `which` 0 kept, 1 mixed."""
    opop, cfg_o = _opop(pop), orc.make_cfg()
    tar = trace_tariffs(pop, base)
    worst = np.zeros((TRACE, n), np.int64)
    for i in range(n):
        for k in range(int(base["nfev"][i])):
            worst[k, i] = list_counts(pop, opop, cfg_o, i, base["trace_x"][i, k], tar[k, i])[which]
    return worst


def _check_forced(r, base, worst, cap, tariff0):
    over = worst > cap
    ends, keeps = over.any(axis=0), ~over.any(axis=0)
    for k, v in r.items():
        assert same(v[keeps], base[k][keeps]), k
    for i in np.nonzero(ends)[0]:
        k = int(np.argmax(over[:, i]))
        assert r["nfev"][i] == k + 1 and (r["status"][i] & FATAL) == _lib.ST_HOURLY_FORM, (i, k)
        assert np.isnan(r["npv"][i]) and np.isnan(r["system_kw"][i])
        assert r["tariff"][i] == tariff0[i] and r["switched"][i] == 0
        assert same(r["trace_x"][i, :k + 1], base["trace_x"][i, :k + 1])
        assert same(r["trace_f"][i, :k], base["trace_f"][i, :k]) and np.isnan(r["trace_f"][i, k:]).all()


def _median_cap(worst):
    """A cap at the median of the agents' worst traced months, moved to the next distinct count below
    when nothing would lie beyond it."""
    per = worst.max(axis=0)
    cap = int(np.median(per))
    if not (per > cap).any():
        cap = int(np.unique(per)[-2])
    return cap


def test_forced_overflow_of_the_kept_list(engine_dc, dc_case):
    eng, pop, n = engine_dc, dc_case["pop"], 10
    sub, base = subset(pop, np.arange(n)), {k: v[:n] for k, v in dc_case["r"].items()}
    _load(eng, pop)
    worst = _forced(eng, sub, base, n, 0)
    assert worst.max() <= _lib.BATT_PEAK_CAPK
    cap = _median_cap(worst)
    over = (worst > cap).any(axis=0)
    print(f"forced overflow: cap_kept {cap}, worst months {worst.max(axis=0).min()} .. {worst.max()}, "
          f"{int(over.sum())} agents end, {int((~over).sum())} keep their bits")
    assert cap >= 1 and over.any() and (~over).any()
    batch, r = _run(eng, sub, peak_caps=(None, cap))
    _check_forced(r, base, worst, cap, sub.cols["tariff0"])
    check_objective(eng, sub, batch, r, caps=(None, cap))


def test_forced_overflow_of_the_mixed_list(engine_dc, mix_case):
    eng, pop, cand, three = engine_dc, mix_case["pop"], mix_case["cand"], mix_case["three"]
    _load(eng, pop)
    t = eng.tariff_records
    rows = np.nonzero(cand & ((three["status"] & FATAL) == 0) & np.isin(t["mo"][pop.cols["tariff0"]], (2, 3))
                      & (pop.cols["sw_storage_cnt"] == 0))[0][:8]
    assert rows.size >= 2
    sub = subset(pop, rows)
    base = {k: v[rows] for k, v in three.items()}
    worst = _forced(eng, sub, base, rows.size, 1)
    assert worst.max() <= _lib.NB_CAPM
    cap = _median_cap(worst)
    over = (worst > cap).any(axis=0)
    print(f"forced overflow: cap_mixed {cap}, worst months {worst.max(axis=0).min()} .. {worst.max()}, "
          f"{int(over.sum())} agents end, {int((~over).sum())} keep their bits")
    assert cap >= 1 and over.any() and (~over).any()
    batch, r = _run(eng, sub, peak_caps=(cap, None))
    _check_forced(r, base, worst, cap, sub.cols["tariff0"])


def test_repeat_and_arguments(engine_dc, engine_hourly_plan, dc_case):
    eng, pop, batch, r = engine_dc, dc_case["pop"], dc_case["batch"], dc_case["r"]
    _load(eng, pop)
    again = _host(eng.size_with_batt(batch, trace=TRACE, net=True, peak=True))
    for k, v in again.items():
        assert same(v, r[k]), k
    named = ["npv", "nfev", "status"]
    _, part = _raw(eng, batch, names=named, first=False)
    for k in MEMBERS:                            # NULL members are not written
        assert same(part[k], r[k]) if k in named else (part[k] == SENT).all(), k
    n = batch.n
    st = torch.zeros(n, dtype=torch.int32, device=eng.dev)
    lo = torch.ones(n, dtype=torch.float64, device=eng.dev)
    args = (eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), n)
    fn, sh = eng.lib.dgen_size_with_batt_peak, eng.stream_handle()
    so = _lib.SwbOut(status=st.data_ptr())
    assert fn(*args, None, None, None, ctypes.byref(_lib.SwbPeakOpt(_lib.NB_CAPM + 1, 0, 0, 0)), ctypes.byref(so), sh) == -1
    assert "dgen_size_with_batt_peak" in _lib.last_error()
    assert fn(*args, None, None, None, ctypes.byref(_lib.SwbPeakOpt(0, _lib.BATT_PEAK_CAPK_MAX + 1, 0, 0)),
              ctypes.byref(so), sh) == -1
    assert fn(*args, lo.data_ptr(), None, None, None, ctypes.byref(so), sh) == -1
    assert fn(*args, None, lo.data_ptr(), None, None, ctypes.byref(so), sh) == -1
    assert fn(*args, None, None, None, None, ctypes.byref(_lib.SwbOut()), sh) == -1         # status NULL
    assert fn(*args, None, None, None, None, None, sh) == -1
    for tn in (-1, TRACE + 1):
        assert fn(*args, None, None, ctypes.byref(_lib.SwbOpt(0.8, 2.0, tn, 0)), None, ctypes.byref(so), sh) == -1
    assert fn(*args[:3], 0, None, None, None, None, ctypes.byref(so), sh) == 0
    assert fn(*args[:3], -1, None, None, None, None, ctypes.byref(so), sh) == -1
    with pytest.raises(_lib.DgenError, match="dgen_size_with_batt_peak"):
        eng.size_with_batt(batch, peak=True, peak_caps=(None, _lib.BATT_PEAK_CAPK_MAX + 1))
    # opt and popt NULL: the defaults; status alone is a valid request
    assert fn(*args, None, None, None, None, ctypes.byref(so), sh) == 0, _lib.last_error()
    assert fn(*args, None, None, None, ctypes.byref(_lib.SwbPeakOpt(_lib.NB_CAPM, _lib.BATT_PEAK_CAPK_MAX, 0, 0)),
              ctypes.byref(so), sh) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), r["status"])
    # the hourly re-plan is not replayed
    en = engine_hourly_plan
    _load(en, pop)
    s4 = subset(pop, np.arange(4))
    b4 = en.upload_agents(s4.cols, s4.n_scratch)
    s4t = torch.zeros(4, dtype=torch.int32, device=en.dev)
    assert en.lib.dgen_size_with_batt_peak(en.ctx, ctypes.byref(en.tables), ctypes.byref(b4.c_agents), 4, None, None,
                                           None, None, ctypes.byref(_lib.SwbOut(status=s4t.data_ptr())),
                                           en.stream_handle()) == -1
    assert "dgen_size_with_batt_peak" in _lib.last_error()


def test_drop_in_switch_with_peak_billing():
    """size_chunk on a reference-schema frame whose commercial rows partly carry com_kwkw's kWh/kW-tier
    tariffs (the drop-in path compiles tariffs as the reference does: demand charges not billed)."""
    from dgen_amd.synth import random_tariffs, reference_frame
    df, store, table = reference_frame(100)
    kw_raws = random_tariffs(np.random.default_rng(KW_SEED), 8, "kwkw")
    com = np.nonzero((df["sector_abbr"] == "com").to_numpy())[0]
    assert com.size >= 12
    kw_rows = com[1::2]
    td, tid = df["tariff_dict"].to_list(), df["tariff_id"].to_numpy().copy()
    for j, i in enumerate(kw_rows):
        td[i], tid[i] = kw_raws[j % 8], 9100 + j % 8
    df["tariff_dict"], df["tariff_id"] = td, tid
    ff._worker_conn = store
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none",
                           pv_batt_sizing={"net_billing": True, "peak_billing": True})
    old, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={"net_billing": True})
    assert list(non.columns) == list(old.columns) and list(non.columns)[-8:] == list(bs.CO_COLUMNS)
    st_old, st = old["pvb_opt_status"].to_numpy(), non["pvb_opt_status"].to_numpy()
    gained = ((st_old & _lib.ST_HOURLY_FORM) != 0) & ((st & bs.INVALID) == 0)
    print(f"drop-in: {kw_rows.size} kWh/kW-tariff rows, {int(((st_old[kw_rows] & _lib.ST_HOURLY_FORM) != 0).sum())} "
          f"without a value before, {int(((st[kw_rows] & bs.INVALID) != 0).sum())} after")
    assert ((st_old[kw_rows] & _lib.ST_HOURLY_FORM) != 0).any() and np.isnan(old["pvb_opt_npv"].to_numpy()[gained]).all()
    assert ((st[kw_rows] & bs.INVALID) == 0).all() and gained[kw_rows].any() and not gained[np.setdiff1d(np.arange(100), kw_rows)].any()
    for c in ("pvb_opt_kw", "pvb_opt_kwh", "pvb_opt_batt_kw", "pvb_opt_npv", "pvb_opt_payback", "pvb_opt_npv_gain"):
        assert np.isfinite(non[c].to_numpy()[kw_rows]).all(), c
    had = (st_old & _lib.ST_HOURLY_FORM) == 0    # the rows the call without the key valued keep their bits
    assert had.any()
    for c in non.columns:
        a, b = old[c].to_numpy(), non[c].to_numpy()
        rows = had if c in bs.CO_COLUMNS else np.ones(len(df), bool)
        if a.dtype.kind in "fiu":
            assert same(a[rows], b[rows]), c
        else:
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[rows], b[rows])), c
    with pytest.raises(ValueError):
        ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={"peak_billing": True, "peak_caps": (0, 1)})
