"""The net-billing tariffs of the PV search on the with-battery objective on the
GPU (dgen_size_with_batt followed by dgen_size_with_batt_net).

The objective is checked point by point against Engine.batt_curve(net=True),
K = 1, on a hand-made sized batch at the traced x (bit for bit, every traced
evaluation and every member at system_kw), the search by replaying scipy's
bounded minimiser over the device's own trace, the fill-in contract on
sentinel-filled buffers against a host restatement of the candidate rule, the
point at system_kw against curve_ref (the oracle's hourly bills), then the
storage switch across the two forms inside one search, the grid stride, the
edges, the forced overflow of the mixed-hour lists and the way up through
size_chunk(pv_batt_sizing={"net_billing": True}).

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
from tests.test_batt_sizing import _opop
from tests.test_gpu_batt_curve import compare
from tests.test_gpu_batt_curve_net import mixed_counts, point_tariffs, ts_agents
from tests.test_gpu_size_with_batt import (FATAL, POINT, TRACE, _host, _load, _oracle_at, _pop, check_search,
                                           default_bracket, same)

pytestmark = pytest.mark.gpu

CA_SEED, MIX_SEED = 20260031, 20260033
SENT = -7
INFO = _lib.ST_EMPTY_EC | _lib.ST_ZERO_LOAD | _lib.ST_DEMAND
MEMBERS = _lib.SWB_FIELDS + ["trace_x", "trace_f"]


def _run(eng, pop, **kw):
    """Both calls through the engine, full trace; device rows are caller rows."""
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    kw.setdefault("net", True)
    return batch, _host(eng.size_with_batt(batch, trace=TRACE, **kw))


def _raw(eng, batch, lo=None, hi=None, ratio=0.8, hours=2.0, cap=0, blocks=0, names=None, first=True):
    """The C entries on sentinel-filled buffers: (host members after dgen_size_with_batt or None, host
    members after dgen_size_with_batt_net).  Members `names` leaves out are not handed to either entry."""
    n = batch.n
    bufs = {k: torch.full((n,), float(SENT), dtype=torch.float64, device=eng.dev) for k in _lib.SWB_F64}
    bufs.update({k: torch.full((n,), SENT, dtype=torch.int32, device=eng.dev) for k in _lib.SWB_I32})
    bufs.update({k: torch.full((n, TRACE), float(SENT), dtype=torch.float64, device=eng.dev)
                 for k in ("trace_x", "trace_f")})
    so = _lib.SwbOut(**{k: bufs[k].data_ptr() for k in (MEMBERS if names is None else names)})
    a = None if lo is None else eng._to_dev(np.ascontiguousarray(lo), torch.float64)
    b = None if hi is None else eng._to_dev(np.ascontiguousarray(hi), torch.float64)
    opt, no = _lib.SwbOpt(ratio, hours, TRACE, 0), _lib.SwbNetOpt(cap, blocks)
    args = (eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), n, None if a is None else a.data_ptr(),
            None if b is None else b.data_ptr(), ctypes.byref(opt))
    one = None
    if first:
        assert eng.lib.dgen_size_with_batt(*args, ctypes.byref(so), eng.stream_handle()) == 0, _lib.last_error()
        one = _host(bufs)
    assert eng.lib.dgen_size_with_batt_net(*args, ctypes.byref(no), ctypes.byref(so), eng.stream_handle()) == 0, \
        _lib.last_error()
    return one, _host(bufs)


def candidates(eng, pop, lo, hi):
    """The entry's candidate rule from the rows alone: a valid bracket, a life in 1 .. MAXY, tariff0
    inside the table without ST_UNIT, and option 2 or 3 on tariff0 or on an in-range storage row."""
    c, t = pop.cols, eng.tariff_records
    t0 = c["tariff0"]
    inr = (t0 >= 0) & (t0 < t.size)
    t0s = np.where(inr, t0, 0)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lo) & np.isfinite(hi) & (lo > 0.0) & (lo < hi)
    ok &= (c["econ_life"] >= 1) & (c["econ_life"] <= _lib.MAXY) & inr & ((t["flags"][t0s] & _lib.ST_UNIT) == 0)
    net = np.isin(t["mo"][t0s], (2, 3))
    for i in np.nonzero(c["sw_storage_cnt"] > 0)[0]:
        off = int(c["sw_storage_off"][i])
        for r in pop.switches[off:off + int(c["sw_storage_cnt"][i])]:
            tt = int(r["tariff"])
            net[i] |= 0 <= tt < t.size and int(t["mo"][tt]) in (2, 3)
    return ok & net


def curve_at(eng, pop, batch, x, ratio, hours, cap=None):
    """Engine.batt_curve(net=True), K = 1, of a hand-made sized batch: system_kw = x from (tariff0, not
    switched, status 0), kwh = x / ratio, kw = kwh / hours, the net entry at the same cap."""
    out = eng.alloc_outputs(batch.n, hourly=False)
    out["system_kw"].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    out["tariff_final"].copy_(torch.from_numpy(np.ascontiguousarray(pop.cols["tariff0"], np.int32)))
    out["switched"].zero_()
    out["status"].zero_()
    kwh = x / ratio
    d = _host(eng.batt_curve(batch, out, kwh, kwh / hours, net=True, net_cap=cap))
    return {k: v[0] for k, v in d.items()}


def check_objective(eng, pop, batch, r, ratio=0.8, hours=2.0, cap=None):
    """Every traced evaluation is the point of dgen_batt_curve + dgen_batt_curve_net, and so is every
    member at system_kw (tests/test_gpu_size_with_batt.check_objective with the net fill-in); returns the
    valued agents."""
    n = batch.n
    tx, tf, nfev = r["trace_x"], r["trace_f"], r["nfev"]
    assert tx.shape == tf.shape == (n, TRACE)
    col = np.arange(TRACE)[None, :]
    assert np.isnan(tx[col >= nfev[:, None]]).all() and np.isnan(tf[col >= nfev[:, None]]).all()
    assert not np.isnan(tx[col < np.minimum(nfev, TRACE)[:, None]]).any()
    for k in range(int(min(nfev.max(initial=0), TRACE))):
        live = nfev > k
        c = curve_at(eng, pop, batch, np.where(live, tx[:, k], 1.0), ratio, hours, cap)
        val = live & ((c["status"] & FATAL) == 0)
        assert same((-c["npv"])[val], tf[val, k]), f"evaluation {k}"
        assert np.isnan(tf[live & ~val, k]).all(), f"evaluation {k}"
        last = live & ~val                       # an evaluation that cannot be valued is the agent's last
        assert (nfev[last] == k + 1).all() and ((r["status"][last] & _lib.ST_HOURLY_FORM) != 0).all(), f"evaluation {k}"
        assert np.array_equal(r["tariff"][last], c["tariff"][last]), f"evaluation {k}"
        assert np.array_equal(r["switched"][last], c["switched"][last]), f"evaluation {k}"
    ok = (r["status"] & FATAL) == 0
    assert (nfev[ok] >= 1).all()
    c = curve_at(eng, pop, batch, np.where(ok, r["system_kw"], 1.0), ratio, hours, cap)
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


def trace_tariffs(pop, r, ratio=0.8, hours=2.0):
    """[TRACE, n] the tariff each traced evaluation bills under, from the rows alone (-1 beyond nfev)."""
    kwh = np.where(np.isnan(r["trace_x"].T), 0.0, r["trace_x"].T) / ratio
    tar = point_tariffs(pop, {"tariff_final": pop.cols["tariff0"]}, kwh, kwh / hours)
    return np.where(np.arange(TRACE)[:, None] < r["nfev"][None, :], tar, -1)


@pytest.fixture(scope="module")
def ca_case(engine):
    """129 CA agents (three tiles), the first 65 searched once with the full trace after both calls and
    after the first call alone (shared, not modified)."""
    pop = _pop("ca_res_storage", 129, CA_SEED)
    _load(engine, pop)
    sub = subset(pop, np.arange(65))
    batch, r = _run(engine, sub)
    _, first = _run(engine, sub, net=False)
    lo, hi = default_bracket(engine, pop)
    return {"pop": pop, "sub": sub, "batch": batch, "r": r, "first": first, "lo": lo, "hi": hi}


def test_ca_objective_and_search(engine, ca_case):
    pop, sub, batch, r, first = (ca_case[k] for k in ("pop", "sub", "batch", "r", "first"))
    _load(engine, pop)
    assert np.isin(pop.tariffs["mo"][sub.cols["tariff0"]], (2, 3)).all()
    # the first call alone ends every agent at its first evaluation
    assert (first["status"] == _lib.ST_HOURLY_FORM).all() and (first["nfev"] == 1).all()
    for k in _lib.SWB_FIELDS:
        assert r[k].shape == (65,) and r[k].dtype == (np.float64 if k in _lib.SWB_F64 else np.int32), k
    assert (r["status"] == 0).all(), np.unique(r["status"])
    ok = check_objective(engine, sub, batch, r)
    assert ok.all() and (r["bank_kwh"] > 0).all()
    lo, hi = ca_case["lo"][:65], ca_case["hi"][:65]
    assert check_search(r, lo, hi).all()
    print("ca_res_storage n=65 nfev:", np.bincount(r["nfev"]))
    assert r["nfev"].max() <= 16
    # the default bracket: the first call's first x, and the bits of the explicit bracket
    assert same(r["trace_x"][:, 0], first["trace_x"][:, 0])
    _, e = _run(engine, sub, lo=lo, hi=hi)
    for k, v in e.items():
        assert same(v, r[k]), k


@pytest.mark.parametrize("n", (1, 63))
def test_agents_do_not_depend_on_the_batch(engine, ca_case, n):
    _load(engine, ca_case["pop"])
    _, s = _run(engine, subset(ca_case["pop"], np.arange(n)))
    for k, v in s.items():
        assert same(v, ca_case["r"][k][:n]), k


def test_grid_stride(engine, ca_case):
    """Three tiles through one block's slice (net_blocks = 1), a ragged stride (2) and the default launch."""
    pop = ca_case["pop"]
    _load(engine, pop)
    batch, full = _run(engine, pop)
    assert batch.n == 129 and (full["status"] == 0).all()
    for k, v in ca_case["r"].items():
        assert same(v, full[k][:65]), k
    for blocks in (1, 2):
        got = _host(engine.size_with_batt(batch, trace=TRACE, net=True, net_blocks=blocks))
        for k, v in got.items():
            assert same(v, full[k]), (blocks, k)


@pytest.fixture(scope="module")
def mix_case(engine):
    """65 agents over every metering option: both C entries on sentinel-filled buffers.  The population
    has no kWh/kW tier units of its own, so two net-billing tariffs are copied with unit codes 1 and 3:
    two net-billing agents get them as tariff0 (their first evaluation ends them), two more reach them
    through a hand-set storage row whose edge lies between the banks of their first two evaluations."""
    pop = _pop("metering_mix", 65, MIX_SEED)
    c, t, cfg_o = pop.cols, pop.tariffs, orc.make_cfg()
    _load(engine, pop)
    _, pre = _run(engine, pop)
    src = np.nonzero(np.isin(t["mo"], (2, 3)) & ~np.isin(t["unit"], (1, 3)))[0][:2]
    extra = t[src].copy()
    extra["unit"] = (1, 3)
    pop.tariffs = np.concatenate([t, extra])
    net0 = np.isin(t["mo"][c["tariff0"]], (2, 3)) & ((pre["status"] & FATAL) == 0)
    head = np.nonzero(net0 & (pre["nfev"] < 3))[0][:2]
    mid = np.nonzero(net0 & (pre["nfev"] >= 3))[0][:2]
    assert head.size == 2 and mid.size == 2
    c["tariff0"] = c["tariff0"].copy()
    c["tariff0"][head] = (t.size, t.size + 1)
    rows, off, cnt = [r for r in pop.switches], c["sw_storage_off"].copy(), c["sw_storage_cnt"].copy()
    for j, i in enumerate(mid):
        v = 240.0 if c["flags"][i] & 1 else 500.0
        b = [orc.batt_size(float(x) / 0.8 / 2.0, float(x) / 0.8, v, cfg_o)[0] for x in pre["trace_x"][i, :2]]
        rec = np.zeros((), dtype=SWITCH_DTYPE)
        rec["min_kw"], rec["max_kw"] = (0.5 * (b[0] + b[1]), 1e9) if b[1] > b[0] else (0.0, 0.5 * (b[0] + b[1]))
        rec["tariff"], rec["one_time_charge"] = t.size + j, 10.0
        off[i], cnt[i] = len(rows), 1
        rows.append(rec)
    pop.switches = np.stack(rows).astype(SWITCH_DTYPE)
    c["sw_storage_off"], c["sw_storage_cnt"] = off, cnt
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    _load(engine, pop)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    one, two = _raw(engine, batch)
    lo, hi = default_bracket(engine, pop)
    return {"pop": pop, "batch": batch, "one": one, "two": two, "cand": candidates(engine, pop, lo, hi), "lo": lo, "hi": hi}


def test_metering_mix_fill_in(engine, mix_case):
    pop, batch, one, two, cand = (mix_case[k] for k in ("pop", "batch", "one", "two", "cand"))
    _load(engine, pop)
    t = engine.tariff_records
    assert pop.skip_demand_charges == 1          # no demand charge is billed here: kWh/kW units are what ends a search
    # alone on sentinel buffers the entry writes exactly the candidates, every member of them
    _, alone = _raw(engine, batch, first=False)
    for k in MEMBERS:
        w = alone[k] != SENT
        w = w.all(axis=1) if w.ndim == 2 else w
        assert np.array_equal(w, cand), k
        assert np.array_equal((alone[k] == SENT).all(axis=1) if alone[k].ndim == 2 else alone[k] == SENT, ~cand), k
        assert same(alone[k][cand], two[k][cand]), k
    # after the first call: a non-candidate keeps the first call's bits, trace rows included
    assert cand.any() and (~cand).any()
    for k in MEMBERS:
        assert same(two[k][~cand], one[k][~cand]), k
    ok = check_objective(engine, pop, batch, two)
    check_search(two, mix_case["lo"], mix_case["hi"])
    # candidates end at the first evaluation on kWh/kW units, as the rows name it; the others are valued
    tar = trace_tariffs(pop, two)
    peak = (tar >= 0) & np.isin(t["unit"][np.maximum(tar, 0)], (1, 3))
    ends, late = 0, 0
    for i in np.nonzero(cand)[0]:
        if peak[:, i].any():
            k = int(np.argmax(peak[:, i]))
            assert two["nfev"][i] == k + 1 and (two["status"][i] & _lib.ST_HOURLY_FORM) and two["tariff"][i] == tar[k, i], i
            assert np.isnan(two["npv"][i]) and np.isnan(two["system_kw"][i]), i
            ends += 1
            late += k > 0
        else:
            assert ok[i] and (two["status"][i] & ~INFO) == 0, (i, int(two["status"][i]))
    at = two["tariff"]
    ts = ts_agents(pop, at) & ok & cand & np.isin(t["mo"][at], (2, 3))
    o3 = ok & cand & (t["mo"][at] == 3)
    print(f"metering_mix: {int(cand.sum())} candidates, {int((ok & cand).sum())} valued, {int(ts.sum())} on the TS sell "
          f"rate, {int(o3.sum())} on option 3, {ends} ended on kWh/kW units ({late} of them after their first evaluation)")
    assert ts.any() and o3.any() and ends >= 1 and late >= 1
    # what the first call valued and cannot reach net billing is untouched; what it flagged for the form is valued now
    gained = cand & ok & ((one["status"] & _lib.ST_HOURLY_FORM) != 0)
    assert gained.any() and np.isin(t["mo"][at[gained]], (2, 3)).all()


def test_against_the_oracle(engine, ca_case, mix_case):
    r = ca_case["r"]
    rows = np.arange(65)
    compare({k: r[k][rows] for k in POINT}, _oracle_at(ca_case["sub"], r, rows), "size_with_batt_net ca_res_storage n=65")
    pop, two = mix_case["pop"], mix_case["two"]
    t = pop.tariffs
    ok = mix_case["cand"] & ((two["status"] & FATAL) == 0)
    at = two["tariff"]
    for what, keep in (("TS sell rate", ok & ts_agents(pop, at) & (t["mo"][at] == 2)),
                       ("option 3", ok & (t["mo"][at] == 3)), ("every valued candidate", ok)):
        rows = np.nonzero(keep)[0]
        assert rows.size
        compare({k: two[k][rows] for k in POINT}, _oracle_at(pop, two, rows), f"size_with_batt_net metering_mix {what}")


def test_storage_switch_across_forms(engine):
    """Hand-set storage rows whose edge lies between the banks of the bracket's ends: NEM agents move onto
    a net-billing tariff inside the search, net-billing agents onto a bins tariff; a third group's row
    names a net-billing tariff beyond the bracket (a candidate billed from bins alone)."""
    pop = _pop("metering_mix", 48, MIX_SEED + 1)
    c, t, cfg_o = pop.cols, pop.tariffs, orc.make_cfg()
    _load(engine, pop)
    lo, hi = default_bracket(engine, pop)
    ok_unit = ~np.isin(t["unit"], (1, 3))
    net_t = np.nonzero(np.isin(t["mo"], (2, 3)) & ok_unit)[0]
    bin_t = np.nonzero(np.isin(t["mo"], (0, 1, 4)) & ok_unit)[0]
    assert net_t.size and bin_t.size
    is_net0 = np.isin(t["mo"][c["tariff0"]], (2, 3))
    rows, off, cnt = [r for r in pop.switches], c["sw_storage_off"].copy(), c["sw_storage_cnt"].copy()
    inside, beyond = np.zeros(48, bool), np.zeros(48, bool)
    for j, i in enumerate(np.nonzero(ok_unit[c["tariff0"]] & (lo > 0.0))[0]):
        v = 240.0 if c["flags"][i] & 1 else 500.0
        b_lo, _ = orc.batt_size(lo[i] / 0.8 / 2.0, lo[i] / 0.8, v, cfg_o)
        b_hi, _ = orc.batt_size(hi[i] / 0.8 / 2.0, hi[i] / 0.8, v, cfg_o)
        if j % 3 == 2 or not (b_hi > b_lo > 0.0):
            continue
        rec = np.zeros((), dtype=SWITCH_DTYPE)
        rec["max_kw"], rec["one_time_charge"] = 1e9, 25.0 + j
        if j % 3 == 0:
            rec["min_kw"] = 0.5 * (b_lo + b_hi)
            rec["tariff"] = (bin_t if is_net0[i] else net_t)[j % (bin_t if is_net0[i] else net_t).size]
            inside[i] = True
        else:
            if is_net0[i]:
                continue
            rec["min_kw"] = 2.0 * b_hi
            rec["tariff"] = net_t[j % net_t.size]
            beyond[i] = True
        off[i], cnt[i] = len(rows), 1
        rows.append(rec)
    assert inside.any() and beyond.any()
    pop.switches = np.stack(rows).astype(SWITCH_DTYPE)
    c["sw_storage_off"], c["sw_storage_cnt"] = off, cnt
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    _load(engine, pop)
    batch, r = _run(engine, pop)
    _, first = _run(engine, pop, net=False)
    cand = candidates(engine, pop, lo, hi)
    assert cand[inside].all() and cand[beyond].all()
    # from the rows alone, ahead of any comparison: a trace billed under both forms, and a candidate's from bins alone
    tar = trace_tariffs(pop, r)
    seen_net = ((tar >= 0) & np.isin(t["mo"][np.maximum(tar, 0)], (2, 3))).any(axis=0)
    seen_bin = ((tar >= 0) & np.isin(t["mo"][np.maximum(tar, 0)], (0, 1, 4))).any(axis=0)
    both, bins_only = cand & seen_net & seen_bin, cand & ~seen_net
    print(f"storage switch: {int(both.sum())} searches under both forms ({int((both & is_net0).sum())} from net billing), "
          f"{int(bins_only.sum())} candidates from bins alone")
    assert (both & is_net0).any() and (both & ~is_net0).any() and bins_only.any()
    ok = check_objective(engine, pop, batch, r)
    check_search(r, lo, hi)
    assert ok[both].all() and ok[bins_only].all()
    for k, v in r.items():
        assert same(v[bins_only], first[k][bins_only]), k
        assert same(v[~cand], first[k][~cand]), k
    rows_ = np.nonzero(both)[0]
    compare({k: r[k][rows_] for k in POINT}, _oracle_at(pop, r, rows_), "size_with_batt_net storage switch across forms")


def test_edges(engine, ca_case):
    pop, base = ca_case["pop"], ca_case["r"]
    _load(engine, pop)
    sub = subset(pop, np.arange(66))
    life, deg = sub.cols["econ_life"].copy(), sub.cols["pv_deg"].copy()
    life[[1, 64]], life[[2, 65]], life[3] = 1, 50, 51
    deg[[4, 5]] = 0.0
    sub.cols["econ_life"], sub.cols["pv_deg"] = life, deg
    batch, r = _run(engine, sub)
    _, first = _run(engine, sub, net=False)
    assert first["status"][3] == _lib.ST_YEARS and (np.delete(r["status"], 3) == 0).all()
    for k, v in r.items():                       # a life outside 1 .. MAXY is no candidate
        assert same(v[3:4], first[k][3:4]), k
    check_objective(engine, sub, batch, r)
    rest = np.setdiff1d(np.arange(65), [1, 2, 3, 4, 5, 64])
    for k, v in r.items():                       # the other rows' bits alone
        assert same(v[rest], base[k][rest]), k
    rows = np.array([1, 2, 4, 5, 64, 65])
    compare({k: r[k][rows] for k in POINT}, _oracle_at(sub, r, rows), "size_with_batt_net lives 1 and 50, pv_deg = 0")
    # a larger, longer bank
    s65, lo, hi = ca_case["sub"], ca_case["lo"][:65], ca_case["hi"][:65]
    batch, q = _run(engine, s65, ratio=0.4, hours=4.0)
    assert check_objective(engine, s65, batch, q, 0.4, 4.0).all()
    check_search(q, lo, hi)
    assert not np.array_equal(q["npv"], base["npv"])
    compare({k: q[k][:8] for k in POINT}, _oracle_at(s65, q, np.arange(8), 0.4, 4.0), "size_with_batt_net 0.4 / 4 h")
    # no battery: the search runs on the PV-only hourly bills
    engine.set_battery(False)
    try:
        batch, z = _run(engine, s65)
        assert (z["status"] == 0).all() and (z["bank_kwh"] == 0).all() and (z["switched"] == 0).all()
        assert check_objective(engine, s65, batch, z).all()
    finally:
        engine.set_battery(True)
    check_search(z, lo, hi)
    # a bracket 1000 x wider: longer searches, the tolerance above its floor (where the objective falls
    # all the way to the lower end every agent walks the same golden-section path: equal lengths are fine)
    lo2, hi2 = lo * 0.25, hi * 1000.0
    assert (np.floor((hi2 - lo2) * 1e-3) > 2.0).all()
    batch, w = _run(engine, s65, lo=lo2, hi=hi2)
    check_search(w, lo2, hi2)
    okw = check_objective(engine, s65, batch, w)
    print("wide bracket nfev:", np.bincount(w["nfev"]), "valued", int(okw.sum()))
    assert okw.any() and w["nfev"][okw].min() > base["nfev"].max()
    # invalid brackets: the first call's DGEN_ST_BOUNDS, and nothing written by the second
    lo3, hi3 = lo.copy(), hi.copy()
    bad = [3, 10, 11, 63, 64]
    lo3[3] = hi3[3]
    lo3[10], hi3[10] = hi3[10], lo3[10]
    lo3[11] = np.nan
    hi3[63] = np.inf
    lo3[64] = 0.0
    batch = engine.upload_agents(s65.cols, s65.n_scratch)
    one, two = _raw(engine, batch, lo=lo3, hi=hi3)
    _, alone = _raw(engine, batch, lo=lo3, hi=hi3, first=False)
    assert (two["status"][bad] == _lib.ST_BOUNDS).all() and (two["nfev"][bad] == 0).all()
    good = np.setdiff1d(np.arange(65), bad)
    for k in MEMBERS:
        assert (alone[k][bad] == SENT).all(), k
        assert same(two[k][bad], one[k][bad]), k
        assert same(two[k][good], base[k][good]), k


def test_forced_overflow(engine, ca_case):
    """A cap at the median of the agents' worst traced months: an agent whose evaluation k is the first
    beyond it ends there, every other agent has the default cap's bits."""
    pop, n = ca_case["pop"], 24
    sub, base = subset(pop, np.arange(n)), {k: v[:n] for k, v in ca_case["r"].items()}
    _load(engine, pop)
    opop, cfg_o = _opop(sub), orc.make_cfg()
    worst = np.zeros((TRACE, n), np.int64)
    for i in range(n):
        for k in range(int(base["nfev"][i])):
            x = float(base["trace_x"][i, k])
            worst[k, i] = mixed_counts(opop, cfg_o, i, x, x / 0.8, x / 0.8 / 2.0).max()
    assert worst.max() <= _lib.NB_CAPM
    cap = int(np.median(worst.max(axis=0)))
    over = worst > cap
    ends, keeps = over.any(axis=0), ~over.any(axis=0)
    print(f"forced overflow: cap {cap}, worst months {worst.max(axis=0).min()} .. {worst.max()}, "
          f"{int(ends.sum())} agents end, {int(keeps.sum())} keep their bits")
    assert cap >= 1 and ends.any() and keeps.any()
    batch, r = _run(engine, sub, net_cap=cap)
    for k, v in r.items():
        assert same(v[keeps], base[k][keeps]), k
    for i in np.nonzero(ends)[0]:
        k = int(np.argmax(over[:, i]))
        assert r["nfev"][i] == k + 1 and r["status"][i] == _lib.ST_HOURLY_FORM, (i, k)
        assert np.isnan(r["npv"][i]) and np.isnan(r["system_kw"][i]) and r["tariff"][i] == sub.cols["tariff0"][i]
        assert same(r["trace_x"][i, :k + 1], base["trace_x"][i, :k + 1])
        assert same(r["trace_f"][i, :k], base["trace_f"][i, :k]) and np.isnan(r["trace_f"][i, k:]).all()
    check_objective(engine, sub, batch, r, cap=cap)


def test_repeat_and_arguments(engine, engine_hourly_plan, ca_case):
    pop, sub, batch, r = (ca_case[k] for k in ("pop", "sub", "batch", "r"))
    _load(engine, pop)
    again = _host(engine.size_with_batt(batch, trace=TRACE, net=True))
    for k, v in again.items():
        assert same(v, r[k]), k
    named = ["npv", "nfev", "status"]
    _, part = _raw(engine, batch, names=named, first=False)
    for k in MEMBERS:                            # NULL members are not written
        assert same(part[k], r[k]) if k in named else (part[k] == SENT).all(), k
    want = ("npv", "system_kw")
    some = _host(engine.size_with_batt(batch, want=want, net=True))
    assert tuple(some) == want + ("status",)
    for k in some:
        assert same(some[k], r[k]), k
    n = batch.n
    st = torch.zeros(n, dtype=torch.int32, device=engine.dev)
    lo = torch.ones(n, dtype=torch.float64, device=engine.dev)
    args = (engine.ctx, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents), n)
    fn, sh = engine.lib.dgen_size_with_batt_net, engine.stream_handle()
    so = _lib.SwbOut(status=st.data_ptr())
    assert fn(*args, None, None, None, ctypes.byref(_lib.SwbNetOpt(_lib.NB_CAPM + 1, 0)), ctypes.byref(so), sh) == -1
    assert "dgen_size_with_batt_net" in _lib.last_error()
    assert fn(*args, lo.data_ptr(), None, None, None, ctypes.byref(so), sh) == -1
    assert fn(*args, None, lo.data_ptr(), None, None, ctypes.byref(so), sh) == -1
    assert fn(*args, None, None, None, None, ctypes.byref(_lib.SwbOut()), sh) == -1         # status NULL
    assert fn(*args, None, None, None, None, None, sh) == -1
    for t in (-1, TRACE + 1):
        assert fn(*args, None, None, ctypes.byref(_lib.SwbOpt(0.8, 2.0, t, 0)), None, ctypes.byref(so), sh) == -1
    assert fn(*args[:3], 0, None, None, None, None, ctypes.byref(so), sh) == 0
    with pytest.raises(_lib.DgenError, match="dgen_size_with_batt_net"):
        engine.size_with_batt(batch, net=True, net_cap=_lib.NB_CAPM + 1)
    # opt and nopt NULL: the defaults; status alone is a valid request
    assert fn(*args, None, None, None, None, ctypes.byref(so), sh) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), r["status"])
    # the hourly re-plan is not replayed
    eng = engine_hourly_plan
    _load(eng, pop)
    s4 = subset(pop, np.arange(4))
    b4 = eng.upload_agents(s4.cols, s4.n_scratch)
    s4t = torch.zeros(4, dtype=torch.int32, device=eng.dev)
    assert eng.lib.dgen_size_with_batt_net(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(b4.c_agents), 4, None, None,
                                           None, None, ctypes.byref(_lib.SwbOut(status=s4t.data_ptr())),
                                           eng.stream_handle()) == -1
    assert "dgen_size_with_batt_net" in _lib.last_error()


def test_drop_in_switch_with_net_billing(engine):
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={"net_billing": True})
    old, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing=True)
    assert list(non.columns) == list(old.columns) and list(non.columns)[-8:] == list(bs.CO_COLUMNS)
    ca = (df["state_abbr"] == "CA").to_numpy()
    st_old, st = old["pvb_opt_status"].to_numpy(), non["pvb_opt_status"].to_numpy()
    assert ca.any() and ((st_old[ca] & _lib.ST_HOURLY_FORM) != 0).all() and np.isnan(old["pvb_opt_npv"].to_numpy()[ca]).all()
    assert ((st[ca] & bs.INVALID) == 0).all()
    for c in ("pvb_opt_kw", "pvb_opt_kwh", "pvb_opt_batt_kw", "pvb_opt_npv", "pvb_opt_payback", "pvb_opt_npv_gain"):
        assert np.isfinite(non[c].to_numpy()[ca]).all(), c
    assert (non["pvb_opt_nfev"].to_numpy()[ca] > 1).all()
    had = (st_old & _lib.ST_HOURLY_FORM) == 0    # the agents the key-less call valued keep their bits
    assert had.any() and not had[ca].any()
    for c in non.columns:
        a, b = old[c].to_numpy(), non[c].to_numpy()
        rows = had if c in bs.CO_COLUMNS else np.ones(len(df), bool)
        if a.dtype.kind in "fiu":
            assert same(a[rows], b[rows]), c
        else:
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[rows], b[rows])), c
    with pytest.raises(ValueError):
        ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={"net_billing": True, "net_cap": 0})
