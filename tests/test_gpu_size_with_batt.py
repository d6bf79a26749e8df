"""PV sizing on the with-battery objective on the GPU (dgen_size_with_batt).

The objective is checked point by point against dgen_batt_curve (bit for bit,
every traced evaluation), the search by replaying scipy's bounded minimiser
(tests/swb_helpers.bounded_brent) over the device's own (x, f) trace, the
default bracket against the oracle's PV-only search, the point at system_kw
against curve_ref (the oracle's PV+battery run, tests/test_batt_sizing), then
the storage rate switch inside the bracket, the edges the header names, and
the way up through size_chunk(pv_batt_sizing=...)."""
import ctypes

import numpy as np
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig
from dgen_amd.synth import make_population, subset
from oracle import oracle as orc
from tests import helpers
from tests.swb_helpers import bounded_brent, xatol_of
from tests.test_batt_sizing import _opop, curve_ref
from tests.test_gpu_batt_curve import compare

pytestmark = pytest.mark.gpu

TRACE = _lib.SWB_TRACE_MAX
RES_N = (1, 63, 65, 257)         # one lane; a 64-lane block less one lane, and plus one; five blocks with a ragged tail
RES_SEED, COM_SEED = 20260003, 20260007
FATAL = _lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_HOURLY_FORM
POINT = tuple(k for k in _lib.SWB_FIELDS if k not in ("system_kw", "nfev"))      # dgen_batt_curve's members


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


def _load(eng, pop):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, None if pop.skip_demand_charges else pop.demand)
    eng.set_switches(pop.switches)


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _run(eng, pop, **kw):
    """Device rows are caller rows (no order)."""
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    return batch, _host(eng.size_with_batt(batch, **kw))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    """Bit for bit (NaN payloads and signed zeros included)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def curve_at(eng, pop, batch, x, ratio, hours):
    """Engine.batt_curve, K = 1, of a hand-made sized batch: system_kw = x from
    (tariff0, not switched, status 0), kwh = x / ratio, kw = kwh / hours."""
    out = eng.alloc_outputs(batch.n, hourly=False)
    out["system_kw"].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    out["tariff_final"].copy_(torch.from_numpy(np.ascontiguousarray(pop.cols["tariff0"], np.int32)))
    out["switched"].zero_()
    out["status"].zero_()
    kwh = x / ratio
    d = _host(eng.batt_curve(batch, out, kwh, kwh / hours))
    return {k: v[0] for k, v in d.items()}


def check_objective(eng, pop, batch, r, ratio=0.8, hours=2.0):
    """Every traced evaluation is the dgen_batt_curve point, and so is every
    member at system_kw; returns the valued agents."""
    n = batch.n
    tx, tf, nfev = r["trace_x"], r["trace_f"], r["nfev"]
    assert tx.shape == tf.shape == (n, TRACE)
    col = np.arange(TRACE)[None, :]
    assert np.isnan(tx[col >= nfev[:, None]]).all() and np.isnan(tf[col >= nfev[:, None]]).all()
    assert not np.isnan(tx[col < np.minimum(nfev, TRACE)[:, None]]).any()
    for k in range(int(min(nfev.max(initial=0), TRACE))):
        live = nfev > k
        x = np.where(live, tx[:, k], 1.0)
        c = curve_at(eng, pop, batch, x, ratio, hours)
        val = live & ((c["status"] & FATAL) == 0)
        assert same((-c["npv"])[val], tf[val, k]), f"evaluation {k}"
        assert np.isnan(tf[live & ~val, k]).all(), f"evaluation {k}"
    ok = (r["status"] & FATAL) == 0
    assert (nfev[ok] >= 1).all()
    c = curve_at(eng, pop, batch, np.where(ok, r["system_kw"], 1.0), ratio, hours)
    info = _lib.ST_EMPTY_EC | _lib.ST_ZERO_LOAD | _lib.ST_DEMAND        # the sizing call's bits dgen_batt_curve hands on
    for m in POINT:
        if m == "status":
            assert np.array_equal(r[m][ok] & ~info, c[m][ok]), m
        else:
            assert same(r[m][ok], c[m][ok]), m
    assert same(np.nanmin(tf[ok], axis=1), -r["npv"][ok])
    for m in _lib.SWB_F64:
        assert np.isnan(r[m][~ok]).all() and not np.isnan(r[m][ok]).any(), m
    return ok


def check_search(r, lo, hi):
    """bounded_brent over the lookup trace_x -> trace_f requests exactly
    trace_x, in order, and returns system_kw and nfev."""
    ok = (r["status"] & FATAL) == 0
    assert (r["nfev"][ok] < TRACE).all(), int(r["nfev"][ok].max())
    for i in np.nonzero(ok)[0]:
        m = int(r["nfev"][i])
        table = {}
        for k in range(m):
            table.setdefault(float(r["trace_x"][i, k]), float(r["trace_f"][i, k]))
        xs, xf, nf = bounded_brent(lambda x: table[x], float(lo[i]), float(hi[i]), xatol_of(float(lo[i]), float(hi[i])))
        assert nf == m and same(np.array(xs), r["trace_x"][i, :m]), i
        assert same(np.array([xf]), r["system_kw"][i:i + 1]), i
    return ok


def default_bracket(eng, pop):
    _, naep = eng.profile_sums()
    max_load = pop.cols["load_kwh"] / naep[pop.cols["cf_row"]]
    return max_load * 0.8, max_load * 1.25


@pytest.fixture(scope="module")
def res_case(engine):
    """257 residential NEM agents searched once over the default bracket with
    the full trace (shared, not modified)."""
    pop = _pop("res_1m_nem_tou", max(RES_N), RES_SEED)
    _load(engine, pop)
    batch, r = _run(engine, pop, trace=TRACE)
    lo, hi = default_bracket(engine, pop)
    return {"pop": pop, "batch": batch, "r": r, "lo": lo, "hi": hi}


def test_objective_is_batt_curve_residential(engine, res_case):
    pop, batch, r = res_case["pop"], res_case["batch"], res_case["r"]
    _load(engine, pop)
    for k in _lib.SWB_FIELDS:
        assert r[k].shape == (batch.n,) and r[k].dtype == (np.float64 if k in _lib.SWB_F64 else np.int32), k
    ok = check_objective(engine, pop, batch, r)
    assert ok.all() and (r["status"] == 0).all()
    assert (r["bank_kwh"] > 0).all()


@pytest.mark.parametrize("n", RES_N[:-1])
def test_agents_do_not_depend_on_the_batch(engine, res_case, n):
    pop, r = res_case["pop"], res_case["r"]
    _load(engine, pop)
    _, s = _run(engine, subset(pop, np.arange(n)), trace=TRACE)
    for k, v in s.items():
        assert same(v, r[k][:n]), k
    if n == 1:                                   # an agent of the last, ragged block as its own batch
        _, s = _run(engine, subset(pop, [200]), trace=TRACE)
        for k, v in s.items():
            assert same(v, r[k][200:201]), k


def test_objective_is_batt_curve_commercial(engine):
    """64 commercial agents: 500 V banks, the commercial Cashloan."""
    pop = _pop("com_8m", 64, COM_SEED)
    assert not (pop.cols["flags"] & 1).any()
    _load(engine, pop)
    batch, r = _run(engine, pop, trace=TRACE)
    ok = check_objective(engine, pop, batch, r)
    assert ok.all()
    check_search(r, *default_bracket(engine, pop))
    print("com_8m n=64 nfev:", np.bincount(r["nfev"]))
    assert len(set(r["nfev"])) > 1 and r["nfev"].max() > 4       # the lanes of one wave search for different lengths


def test_search_is_scipy_on_the_device_objective(engine, res_case):
    pop, lo, hi = res_case["pop"], res_case["lo"], res_case["hi"]
    _load(engine, pop)
    _, r = _run(engine, pop, lo=lo, hi=hi, trace=TRACE)
    ok = check_search(r, lo, hi)
    assert ok.all()
    # a far wider bracket (the default one spans little more than the tolerance's floor of 2 kW for a
    # residential agent): long searches of different lengths within a wave, the tolerance above its floor
    lo2, hi2 = lo[:65] * 0.25, hi[:65] * 1000.0
    assert (np.floor((hi2 - lo2) * 1e-3) > 2.0).all()
    sub = subset(pop, np.arange(65))
    batch, r2 = _run(engine, sub, lo=lo2, hi=hi2, trace=TRACE)
    assert check_search(r2, lo2, hi2).all()
    assert check_objective(engine, sub, batch, r2).all()
    assert r2["nfev"].max() > 4
    assert not np.array_equal(r2["system_kw"], r["system_kw"][:65])


def test_default_bracket(engine, res_case):
    pop, r, lo, hi = res_case["pop"], res_case["r"], res_case["lo"], res_case["hi"]
    _load(engine, pop)
    opop, cfg_o = _opop(pop), orc.make_cfg()
    for i in (0, 1, 2, 63, 64, 65, 255, 256):
        tr, _ = orc.brent_trace(opop, cfg_o, i)
        assert same(tr[:1, 0], r["trace_x"][i, :1]), i
    _, e = _run(engine, pop, lo=lo, hi=hi, trace=TRACE)
    for k, v in e.items():
        assert same(v, r[k]), k


def _oracle_at(pop, r, rows, ratio=0.8, hours=2.0):
    opop, cfg_o = _opop(pop), orc.make_cfg()
    ref = {k: np.zeros(len(rows), np.float64 if k in _lib.BATT_CURVE_F64 else np.int32)
           for k in _lib.BATT_CURVE_FIELDS if k != "status"}
    for j, i in enumerate(rows):
        x = float(r["system_kw"][i])
        c = curve_ref(opop, cfg_o, int(i), x, int(pop.cols["tariff0"][i]), 0, x / ratio, x / ratio / hours)
        for m in ref:
            ref[m][j] = c[m]
    return ref


def test_against_the_oracle(engine, res_case):
    pop, r = res_case["pop"], res_case["r"]
    rows = np.arange(65)
    compare({k: r[k][rows] for k in POINT}, _oracle_at(pop, r, rows), "size_with_batt res_1m_nem_tou n=65")
    com = _pop("com_8m", 16, COM_SEED)
    _load(engine, com)
    _, rc = _run(engine, com)
    assert (rc["status"] == 0).all()
    compare({k: rc[k] for k in POINT}, _oracle_at(com, rc, np.arange(16)), "size_with_batt com_8m n=16")


def test_storage_switch_inside_the_bracket(engine):
    pop = helpers.edge_population("res_1m_nem_tou", 66, "short", 31)
    c, sw, cfg_o = pop.cols, pop.switches, orc.make_cfg()
    _load(engine, pop)
    lo, hi = default_bracket(engine, pop)
    # from the rows alone: a row edge strictly between the banks of the bracket's ends
    inside = np.zeros(66, bool)
    for i in np.nonzero(c["sw_storage_cnt"] > 0)[0]:
        row = sw[int(c["sw_storage_off"][i])]
        v = 240.0 if c["flags"][i] & 1 else 500.0
        b_lo, _ = orc.batt_size(lo[i] / 0.8 / 2.0, lo[i] / 0.8, v, cfg_o)
        b_hi, _ = orc.batt_size(hi[i] / 0.8 / 2.0, hi[i] / 0.8, v, cfg_o)
        inside[i] = any(b_lo < float(e) < b_hi for e in (row["min_kw"], row["max_kw"]))
    assert inside.sum() >= 8, int(inside.sum())
    batch, r = _run(engine, pop, lo=lo, hi=hi, trace=TRACE)
    ok = check_objective(engine, pop, batch, r)
    assert (ok & inside).sum() >= 8
    check_search(r, lo, hi)
    # some agent's evaluations were billed under both tariffs
    both = 0
    for i in np.nonzero(ok & inside)[0]:
        seen = set()
        for k in range(int(r["nfev"][i])):
            x = float(r["trace_x"][i, k])
            bank, _ = orc.batt_size(x / 0.8 / 2.0, x / 0.8, 240.0 if c["flags"][i] & 1 else 500.0, cfg_o)
            row = sw[int(c["sw_storage_off"][i])]
            seen.add(bool(bank > 0.0 and float(row["min_kw"]) <= bank < float(row["max_kw"])))
        both += len(seen) == 2 and int(row["tariff"]) != int(c["tariff0"][i])
    assert both >= 1


def test_lives_1_and_50_and_other_ratios(engine, res_case):
    pop, n = res_case["pop"], 66
    sub = subset(pop, np.arange(n))
    life = sub.cols["econ_life"].copy()
    life[[1, 64]], life[[2, 65]], life[3] = 1, 50, 51
    sub.cols["econ_life"] = life
    _load(engine, pop)
    batch, r = _run(engine, sub, trace=TRACE)
    assert r["status"][3] == _lib.ST_YEARS and r["nfev"][3] == 0 and (np.delete(r["status"], 3) == 0).all()
    check_objective(engine, sub, batch, r)
    rest = np.setdiff1d(np.arange(n), [1, 2, 3, 64, 65])
    for k, v in r.items():                       # the other rows' bits alone
        assert same(v[rest], res_case["r"][k][rest]), k
    rows = np.array([1, 2, 64, 65])
    compare({k: r[k][rows] for k in POINT}, _oracle_at(sub, r, rows), "size_with_batt lives 1 and 50")
    # a larger, longer bank
    sub = subset(pop, np.arange(65))
    batch, q = _run(engine, sub, ratio=0.4, hours=4.0, trace=TRACE)
    assert check_objective(engine, sub, batch, q, 0.4, 4.0).all()
    check_search(q, res_case["lo"][:65], res_case["hi"][:65])
    assert np.array_equal(q["power_kw"], q["bank_kwh"] * ((q["system_kw"] / 0.4 / 4.0) / (q["system_kw"] / 0.4)))
    assert not np.array_equal(q["npv"], res_case["r"]["npv"][:65])
    compare({k: q[k][:16] for k in POINT}, _oracle_at(sub, q, np.arange(16), 0.4, 4.0), "size_with_batt 0.4 / 4 h")


def test_battery_off_searches_the_pv_only_bills(engine, res_case):
    pop = subset(res_case["pop"], np.arange(65))
    _load(engine, res_case["pop"])
    engine.set_battery(False)
    try:
        batch, r = _run(engine, pop, trace=TRACE)
    finally:
        engine.set_battery(True)
    assert (r["status"] == 0).all() and (r["bank_kwh"] == 0).all() and (r["power_kw"] == 0).all()
    assert np.isfinite(r["npv"]).all() and (r["switched"] == 0).all()
    out = engine.alloc_outputs(batch.n, hourly=False)
    out["system_kw"].copy_(torch.from_numpy(r["system_kw"]))
    out["tariff_final"].copy_(torch.from_numpy(np.ascontiguousarray(pop.cols["tariff0"], np.int32)))
    out["switched"].zero_()
    out["status"].zero_()
    c = _host(engine.batt_curve(batch, out, np.zeros(batch.n)))
    for m in POINT:
        assert same(r[m], c[m][0]), m
    check_search(r, res_case["lo"][:65], res_case["hi"][:65])


def test_uncovered_forms_end_the_search(engine):
    pop = _pop("metering_mix", 65, 20260011)
    _load(engine, pop)
    batch, r = _run(engine, pop, trace=TRACE)
    ok = check_objective(engine, pop, batch, r)
    mo = pop.tariffs["mo"]
    hourly = np.isin(mo[pop.cols["tariff0"]], (2, 3)) & (pop.cols["sw_storage_cnt"] == 0)
    assert hourly.any() and ok.any()
    assert (r["status"][hourly] & _lib.ST_HOURLY_FORM).all() and (r["nfev"][hourly] == 1).all()
    dead = ~ok
    assert ((r["status"][dead] & _lib.ST_HOURLY_FORM) != 0).all() and (r["nfev"][dead] >= 1).all()
    assert (r["nfev"][dead] < TRACE).all()        # a dead lane stops counting: nowhere near the 500-evaluation limit
    assert set(mo[r["tariff"][ok]]) <= {0, 1, 4} and np.isin(mo[r["tariff"][dead]], (2, 3)).all()
    check_search(r, *default_bracket(engine, pop))
    # the covered agents alone, as their own batch: the same bits
    _, s = _run(engine, subset(pop, np.nonzero(ok)[0]), trace=TRACE)
    for k, v in s.items():
        assert same(v, r[k][ok]), k


def test_bad_brackets_flag_single_agents(engine, res_case):
    pop, lo, hi = subset(res_case["pop"], np.arange(65)), res_case["lo"][:65].copy(), res_case["hi"][:65].copy()
    _load(engine, res_case["pop"])
    bad = [3, 10, 11, 30, 63, 64]
    lo[3] = hi[3]
    lo[10], hi[10] = hi[10], lo[10]
    lo[11] = np.nan
    hi[30] = np.inf
    lo[63] = 0.0
    lo[64] = -1.0
    _, r = _run(engine, pop, lo=lo, hi=hi, trace=TRACE)
    assert (r["status"][bad] == _lib.ST_BOUNDS).all() and (r["nfev"][bad] == 0).all()
    for m in _lib.SWB_F64 + ["trace_x", "trace_f"]:
        assert np.isnan(r[m][bad]).all(), m
    assert np.array_equal(r["tariff"][bad], pop.cols["tariff0"][bad]) and (r["switched"][bad] == 0).all()
    good = np.setdiff1d(np.arange(65), bad)
    for k, v in r.items():
        assert same(v[good], res_case["r"][k][good]), k
    # no load: the default bracket is empty
    zero = subset(res_case["pop"], np.arange(4))
    zero.cols["load_kwh"] = zero.cols["load_kwh"].copy()
    zero.cols["load_kwh"][2] = 0.0
    _, z = _run(engine, zero)
    assert z["status"][2] == _lib.ST_BOUNDS | _lib.ST_ZERO_LOAD and np.isnan(z["npv"][2])
    for k, v in z.items():
        assert same(np.delete(v, 2), np.delete(res_case["r"][k][:4], 2)), k


def test_arguments_and_repeat(engine, engine_hourly_plan, res_case):
    pop, batch = res_case["pop"], res_case["batch"]
    _load(engine, pop)
    again = _host(engine.size_with_batt(batch, trace=TRACE))
    for k, v in again.items():
        assert same(v, res_case["r"][k]), k
    want = ("npv", "nfev")
    part = _host(engine.size_with_batt(batch, want=want))
    assert tuple(part) == want + ("status",)
    for k in part:
        assert same(part[k], res_case["r"][k]), k
    n = batch.n
    for t in (-1, TRACE + 1):
        with pytest.raises(_lib.DgenError, match="dgen_size_with_batt"):
            engine.size_with_batt(batch, trace=t)
    with pytest.raises(ValueError):
        engine.size_with_batt(batch, lo=res_case["lo"])
    with pytest.raises(ValueError):
        engine.size_with_batt(batch, lo=res_case["lo"][:5], hi=res_case["hi"][:5])
    with pytest.raises(ValueError):
        engine.size_with_batt(batch, want=("npv", "nope"))
    st = torch.zeros(n, dtype=torch.int32, device=engine.dev)
    lo = torch.ones(n, dtype=torch.float64, device=engine.dev)
    args = (engine.ctx, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents), n)
    fn, sh = engine.lib.dgen_size_with_batt, engine.stream_handle()
    so = _lib.SwbOut(status=st.data_ptr())
    assert fn(*args, lo.data_ptr(), None, None, ctypes.byref(so), sh) == -1
    assert "dgen_size_with_batt" in _lib.last_error()
    assert fn(*args, None, lo.data_ptr(), None, ctypes.byref(so), sh) == -1
    assert fn(*args, None, None, None, ctypes.byref(_lib.SwbOut()), sh) == -1        # status NULL
    assert fn(*args, None, None, None, None, sh) == -1
    for t in (-1, TRACE + 1):
        assert fn(*args, None, None, ctypes.byref(_lib.SwbOpt(0.8, 2.0, t, 0)), ctypes.byref(so), sh) == -1
    assert fn(*args[:3], 0, None, None, None, ctypes.byref(so), sh) == 0
    # opt NULL and non-positive ratio / hours: 0.8 and 2.0; status alone is a valid request
    assert fn(*args, None, None, None, ctypes.byref(so), sh) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), res_case["r"]["status"])
    dflt = _host(engine.size_with_batt(batch, ratio=0.0, hours=float("nan")))
    for k, v in dflt.items():
        assert same(v, res_case["r"][k]), k
    # the hourly re-plan and the Li-ion loss model are not replayed
    sub = subset(pop, np.arange(4))
    for eng, own in ((engine_hourly_plan, False), (None, True)):
        if own:
            from dgen_amd.engine import Engine
            eng = Engine(0, EngineConfig(batt_loss_model=1))
        try:
            _load(eng, pop)
            b4 = eng.upload_agents(sub.cols, sub.n_scratch)
            with pytest.raises(_lib.DgenError, match="dgen_size_with_batt"):
                eng.size_with_batt(b4)
        finally:
            if own:
                eng.close()


def test_drop_in_switch(engine):
    from dgen_amd.columnar import columnize_frame
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing=True)
    arr, _ = ff.size_chunk(df, None, table, "simple", hourly="array", pv_batt_sizing=True)
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing=True, max_rows=64)
    off, o_off = ff.size_chunk(df, None, table, "simple", hourly="none")
    assert list(non.columns)[-8:] == list(bs.CO_COLUMNS)
    assert list(off.columns) == [c for c in non.columns if c not in bs.CO_COLUMNS]
    assert not any(c in o_off for c in bs.CO_COLUMNS)
    for c in off.columns:                        # the frame's other columns: the bits of a call without the option
        a, b = off[c].to_numpy(), non[c].to_numpy()
        if a.dtype.kind in "fiu":
            assert np.array_equal(a, b, equal_nan=True), c
        else:
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)), c
    # Engine.size_with_batt of the frame's columns, caller order
    eng = ff.get_engine()
    src = ff._source(store)
    b = columnize_frame(df, src, table)
    ff._device_tables(eng, src, b)
    batch = eng.upload_agents(b.frame_columns)
    r = _host(eng.size_with_batt(batch))
    members = {"kw": "system_kw", "kwh": "bank_kwh", "batt_kw": "power_kw", "npv": "npv", "payback": "payback_raw",
               "nfev": "nfev", "status": "status"}
    for c in bs.CO_COLUMNS:
        a = non[c].to_numpy()
        assert a.dtype == (np.int64 if c in ("pvb_opt_nfev", "pvb_opt_status") else np.float64), c
        assert same(a, arr[c].to_numpy()) and same(a, sub[c].to_numpy()), c
        m = members.get(c[len(bs.CO_PREFIX):])
        if m is not None:
            assert same(a, r[m].astype(a.dtype)), c
    st, gain = non["pvb_opt_status"].to_numpy(), non["pvb_opt_npv_gain"].to_numpy()
    valid = (st & bs.INVALID) == 0
    assert valid.any() and np.isfinite(non["pvb_opt_npv"].to_numpy()[valid]).all()
    assert np.isfinite(gain).any() and not np.isfinite(gain[~valid]).any()
    with pytest.raises(ValueError):
        ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={"pv_to_batt": 0.8})
    spec, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={"ratio": 0.4, "hours": 4.0})
    assert not np.array_equal(spec["pvb_opt_kwh"].to_numpy(), non["pvb_opt_kwh"].to_numpy(), equal_nan=True)
