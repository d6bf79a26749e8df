"""Year-1 monthly bill breakdown on the GPU: dgen_bill_months against the numpy
restatement of its definition (tests/test_bill_metrics.bill_months_ref) at the
device's own sizes -- the kWh members and the peak bit for bit, the dollars
within the project's tolerance -- against the engine's own year-1 bills (which
the parity tests pin to the oracle), against the oracle directly for the
battery case, the edges the header names, and its way up through
Engine.bill_months, dgen_amd.bill_metrics and the drop-in switch
size_frame / size_chunk(bill_metrics=True)."""
import ctypes

import numpy as np
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import bill_metrics as blm
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig
from dgen_amd.synth import make_population, subset
from oracle import oracle as orc
from tests.helpers import oracle_tariffs
from tests.test_bill_metrics import bill_months_ref

pytestmark = pytest.mark.gpu

# the project's tolerances (tests/test_gpu_parity.py): 1e-6 relative / 1e-6 absolute on dollars
RTOL = ATOL = 1e-6
KWH = ("import_kwh", "export_kwh", "billed_kwh", "peak_kw")          # bit for bit without a battery
DOLLARS = ("energy_charge", "export_credit", "fixed_charge", "demand_flat", "demand_tou", "total", "carry")
MIX_N = (1, 63, 65, 257)   # one lane; a 64-lane block less one lane, and plus one; five blocks with a ragged tail


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


def _load(eng, pop):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand)
    eng.set_switches(pop.switches)


def _size(eng, pop):
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    return batch, out


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _seqsum(a):
    """[12, n] -> [n]: the months added in month order."""
    return np.cumsum(a, axis=0)[-1]


def agent_hours(pop, i, kw, ssum):
    """ld and pv of agent i at kw, formed as the header defines them."""
    c = pop.cols
    lr, cr = int(c["load_row"][i]), int(c["cf_row"][i])
    ls = float(c["load_kwh"][i]) / float(ssum[lr])
    cs6 = (((float(kw) * 1000.0) * 0.96) / 1000.0) / 1e6
    return pop.shapes[lr].astype(np.float64) * ls, pop.cfs[cr].astype(np.float64) * cs6


def agent_ts(pop, i, mo):
    """The agent's TS sell rates under a tariff of metering option mo, or None."""
    c = pop.cols
    wr = int(c["wholesale_row"][i])
    if mo != 2 or (int(c["flags"][i]) & 2) or wr < 0 or pop.wholesale is None:
        return None
    return (pop.wholesale[wr] * float(c["price_mult"][i])).astype(np.float32).astype(np.float64)


def reference(pop, otar, kw, tix, ssum, cfg_o, demand, battery=False):
    """bill_months_ref of every agent at kw[i] under tariff tix[i]: {member:
    [12, n]}.  battery: g is the oracle's dispatch (orc.batt_dispatch) at the
    bank orc.batt_size gives, else the PV output."""
    n = len(kw)
    res = {k: np.zeros((12, n)) for k in _lib.BILL_FIELDS}
    for i in range(n):
        load, pv = agent_hours(pop, i, kw[i], ssum)
        g = pv
        if battery:
            bank, power = orc.batt_size(kw[i] / 0.8 / 2.0, kw[i] / 0.8, 240.0 if pop.cols["flags"][i] & 1 else 500.0, cfg_o)
            if bank > 0.0:
                g, _ = orc.batt_dispatch(load, pv, bank, power, cfg_o)
        t = otar[int(tix[i])]
        r = bill_months_ref(load, g, t, cfg_o, agent_ts(pop, i, int(t.mo)), demand=demand)
        for k in _lib.BILL_FIELDS:
            res[k][:, i] = r[k]
    return res


def compare(dev, ref, what, exact=True):
    """The kWh members and the peak bit for bit (exact: without a battery),
    every dollar member within RTOL / ATOL; prints the worst figures."""
    worst = {}
    for k in _lib.BILL_FIELDS:
        a, r = dev[k], ref[k]
        assert a.shape == r.shape and a.dtype == np.float64, (what, k)
        worst[k] = float((np.abs(a - r) / np.maximum(np.abs(r), 1.0)).max())
    print(f"{what}: worst relative " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in KWH:
        if exact:
            assert np.array_equal(dev[k], ref[k]), (what, k, worst[k])
        else:
            assert np.allclose(dev[k], ref[k], rtol=RTOL, atol=ATOL), (what, k, worst[k])
    for k in DOLLARS:
        assert np.allclose(dev[k], ref[k], rtol=RTOL, atol=ATOL), (what, k, worst[k])


def _case(eng, cfg_name, n, seed):
    """A population sized once on the device (battery on), its three bills under
    tariff_final in device order, and the references at the device's sizes."""
    pop = _pop(cfg_name, n, seed)
    _load(eng, pop)
    batch, out = _size(eng, pop)
    assert batch.perm is None
    o = _host({k: out[k] for k in ("system_kw", "x_last", "tariff_final", "status", "bill_w_batt", "bill_wo_batt",
                                    "first_with", "first_without", "batt_kwh")})
    d = {c: _host(v) for c, v in blm.bill_outputs(eng, batch, out).items()}
    ssum, _ = eng.profile_sums()
    cfg_o = orc.make_cfg()
    demand = eng.cfg.skip_demand_charges == 0
    otar = oracle_tariffs(pop.tariffs, pop.demand)
    tf = o["tariff_final"]
    ref = {"baseline": reference(pop, otar, np.zeros(n), tf, ssum, cfg_o, demand),
           "pvonly": reference(pop, otar, o["x_last"], tf, ssum, cfg_o, demand),
           "with_batt": reference(pop, otar, o["system_kw"], tf, ssum, cfg_o, demand, battery=True)}
    return {"pop": pop, "batch": batch, "out": out, "o": o, "dev": d, "ref": ref, "ssum": ssum, "otar": otar,
            "demand": demand}


def _check_case(c, what):
    o, d = c["o"], c["dev"]
    ok = o["status"] == 0
    assert ok.any()
    for case in blm.CASES:
        assert np.array_equal(d[case]["status"] == 0, ok), (what, case)
        dv = {k: d[case][k][:, ok] for k in _lib.BILL_FIELDS}
        rf = {k: c["ref"][case][k][:, ok] for k in _lib.BILL_FIELDS}
        compare(dv, rf, f"{what} {case}", exact=case != "with_batt")
        assert np.isnan(d[case]["total"][:, ~ok]).all()
    # the engine's own year-1 bills (pinned to the oracle by the parity tests): no agent left out
    tw = _seqsum(d["with_batt"]["total"])[ok]
    assert np.allclose(tw, o["bill_w_batt"][ok, 1], rtol=RTOL, atol=0.0), what
    tb = _seqsum(d["baseline"]["total"])[ok]
    assert np.allclose(tb, o["bill_wo_batt"][ok, 1], rtol=RTOL, atol=0.0), what
    assert not d["baseline"]["export_kwh"][:, ok].any()
    print(f"{what}: {int(ok.sum())} of {ok.size} agents; worst sum(total) vs bill_w_batt[1] "
          f"{np.abs(tw / o['bill_w_batt'][ok, 1] - 1).max():.2e}, vs bill_wo_batt[1] "
          f"{np.abs(tb / o['bill_wo_batt'][ok, 1] - 1).max():.2e}")


@pytest.fixture(scope="module")
def mix_case(engine):
    return _case(engine, "metering_mix", max(MIX_N), 20260031)


@pytest.fixture(scope="module")
def res_case(engine):
    return _case(engine, "res_1m_nem_tou", 65, 20260003)


@pytest.mark.parametrize("n", MIX_N)
def test_metering_mix_matches_the_restatement(engine, mix_case, n):
    c = mix_case
    pop = c["pop"]
    if n == max(MIX_N):
        tf = c["o"]["tariff_final"]
        mos = {int(pop.tariffs["mo"][t]) for t in tf}
        assert mos == {0, 1, 2, 3, 4}, mos
        ts = [agent_ts(pop, i, int(pop.tariffs["mo"][tf[i]])) is not None for i in range(n)]
        assert any(ts) and not all(ts)
        assert (c["ref"]["pvonly"]["carry"] > 0).any() and (c["ref"]["pvonly"]["export_kwh"] > 0).any()
        _check_case(c, f"metering_mix n={n}")
        return
    # an agent's bill does not depend on its batch: the shared reference holds
    sub = subset(pop, np.arange(n))
    _load(engine, pop)
    batch = engine.upload_agents(sub.cols, sub.n_scratch)
    o = c["o"]
    for case, kw, batt in (("baseline", np.zeros(n), False), ("pvonly", o["x_last"][:n], False),
                           ("with_batt", o["system_kw"][:n], True)):
        d = _host(engine.bill_months(batch, kw, o["tariff_final"][:n], battery=batt))
        assert sorted(d) == sorted(_lib.BILL_FIELDS + ["status"])
        for k in _lib.BILL_FIELDS:
            assert d[k].shape == (12, n)
            assert np.array_equal(d[k], c["dev"][case][k][:, :n], equal_nan=True), (n, case, k)
        assert np.array_equal(d["status"], c["dev"][case]["status"][:n])


def test_residential_nem_tou_matches_the_restatement(res_case):
    assert (res_case["o"]["batt_kwh"] > 0).all()
    _check_case(res_case, "res_1m_nem_tou n=65")


def test_kwh_per_kw_tiers_match_the_restatement(engine):
    c = _case(engine, "com_kwkw", 65, 20260021)
    units = {int(c["pop"].tariffs["unit"][t]) for t in c["o"]["tariff_final"]}
    assert units & {1, 3}, units
    _check_case(c, "com_kwkw n=65")


def test_demand_charges_match_the_restatement(engine_dc):
    c = _case(engine_dc, "com_dc_batt", 65, 20260007)
    assert c["demand"] and (c["ref"]["pvonly"]["demand_flat"] > 0).any() and (c["ref"]["pvonly"]["demand_tou"] > 0).any()
    _check_case(c, "com_dc_batt n=65")


def test_battery_off_equals_the_search_bills(engine, mix_case):
    """After set_battery(False) no storage switch follows the search: pvonly at
    x_last is first_with, baseline first_without, under tariff_final; and the
    battery form is the plain form bit for bit."""
    pop, n = mix_case["pop"], 130
    sub = subset(pop, np.arange(n))
    _load(engine, pop)
    engine.set_battery(False)
    try:
        batch, out = _size(engine, sub)
        o = _host({k: out[k] for k in ("x_last", "system_kw", "tariff_final", "status", "first_with", "first_without")})
        d = {c: _host(v) for c, v in blm.bill_outputs(engine, batch, out).items()}
        plain = _host(engine.bill_months(batch, out["system_kw"], out["tariff_final"], battery=False))
    finally:
        engine.set_battery(True)
    ok = o["status"] == 0
    assert ok.sum() >= n - 2
    assert np.allclose(_seqsum(d["pvonly"]["total"])[ok], o["first_with"][ok], rtol=RTOL, atol=0.0)
    assert np.allclose(_seqsum(d["baseline"]["total"])[ok], o["first_without"][ok], rtol=RTOL, atol=0.0)
    for k in _lib.BILL_FIELDS:
        assert np.array_equal(d["with_batt"][k], plain[k], equal_nan=True), k


@pytest.mark.parametrize("cfg_name,n,seed", [("res_1m_nem_tou", 65, 20260003), ("com_8m", 64, 20260007)])
def test_battery_case_against_the_oracle(engine, res_case, cfg_name, n, seed):
    """sum_m total of the battery form against orc.ur5 on orc.batt_dispatch's
    system output at the device's system_kw (year 1: factors 1)."""
    if cfg_name == "res_1m_nem_tou":
        c = res_case
        pop, kw, tf = c["pop"], c["o"]["system_kw"], c["o"]["tariff_final"]
        tot = _seqsum(c["dev"]["with_batt"]["total"])
        assert (c["o"]["status"] == 0).all()
    else:
        pop = _pop(cfg_name, n, seed)
        _load(engine, pop)
        batch, out = _size(engine, pop)
        d = _host(engine.bill_months(batch, out["system_kw"], out["tariff_final"], battery=True, want=("total",)))
        assert not d["status"].any() and not (pop.cols["flags"] & 1).any()
        kw, tf, tot = out["system_kw"].cpu().numpy(), out["tariff_final"].cpu().numpy(), _seqsum(d["total"])
    ssum, _ = engine.profile_sums()
    cfg_o = orc.make_cfg()
    otar = oracle_tariffs(pop.tariffs, pop.demand)
    for i in range(n):
        load, pv = agent_hours(pop, i, kw[i], ssum)
        bank, power = orc.batt_size(kw[i] / 0.8 / 2.0, kw[i] / 0.8, 240.0 if pop.cols["flags"][i] & 1 else 500.0, cfg_o)
        assert bank > 0.0
        sysgen, _ = orc.batt_dispatch(load, pv, bank, power, cfg_o)
        t = otar[int(tf[i])]
        want = orc.ur5(t, cfg_o, sysgen, load, agent_ts(pop, i, int(t.mo)), 1, 0.0, 0.0, 0.0)["bill_w"][1]
        assert abs(tot[i] - want) <= RTOL * abs(want), (cfg_name, i, tot[i], want)


def test_zero_kw_bad_kw_and_bad_tariff(engine, res_case):
    c = res_case
    pop, batch, n = c["pop"], c["batch"], 65
    _load(engine, pop)
    nt = int(pop.tariffs.size)
    kw = c["o"]["x_last"].copy()
    tf = c["o"]["tariff_final"].astype(np.int32).copy()
    kw[[3, 64]] = [np.nan, -1.0]
    kw[10] = np.inf
    tf[[5, 63]] = [-1, nt]
    kw[20] = 0.0
    d = _host(engine.bill_months(batch, kw, tf))
    st = d["status"]
    assert (st[[3, 64, 10]] == _lib.ST_BOUNDS).all() and (st[[5, 63]] == _lib.ST_TARIFF).all()
    bad = np.array([3, 5, 10, 63, 64])
    others = np.setdiff1d(np.arange(n), np.append(bad, 20))
    assert not st[others].any() and st[20] == 0
    for k in _lib.BILL_FIELDS:
        assert np.isnan(d[k][:, bad]).all(), k
        assert np.array_equal(d[k][:, others], c["dev"]["pvonly"][k][:, others]), k      # the neighbours are intact
        assert np.array_equal(d[k][:, 20], c["dev"]["baseline"][k][:, 20]), k            # kw = 0: the no-system bill
    assert not d["export_kwh"][:, 20].any()


def test_null_members_two_runs_and_arguments(engine, res_case):
    c = res_case
    _load(engine, c["pop"])
    batch, n = c["batch"], c["batch"].n
    kw, tf = c["out"]["x_last"], c["out"]["tariff_final"]
    again = _host(engine.bill_months(batch, kw, tf))
    for k in _lib.BILL_FIELDS:
        assert np.array_equal(again[k], c["dev"]["pvonly"][k]), k
    bufs = {k: torch.full((12, n), -7.0, dtype=torch.float64, device=engine.dev) for k in _lib.BILL_FIELDS}
    st_buf = torch.full((n,), -7, dtype=torch.int32, device=engine.dev)
    wanted = ("total", "carry", "peak_kw")
    bo = _lib.BillOut(status=st_buf.data_ptr(), **{k: bufs[k].data_ptr() for k in wanted})
    L, st = engine.lib, engine.stream_handle()
    args = (engine.ctx, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents), kw.data_ptr(), tf.data_ptr())
    assert L.dgen_bill_months(*args, n, None, ctypes.byref(bo), st) == 0, _lib.last_error()        # NULL opt: no battery
    torch.cuda.synchronize()
    for k in _lib.BILL_FIELDS:
        a = bufs[k].cpu().numpy()
        if k in wanted:
            assert np.array_equal(a, c["dev"]["pvonly"][k]), k
        else:
            assert (a == -7).all(), k
    assert not st_buf.cpu().numpy().any()
    assert L.dgen_bill_months(*args, 0, None, ctypes.byref(bo), st) == 0                          # n = 0: no launch
    assert L.dgen_bill_months(*args, -1, None, ctypes.byref(bo), st) == -1                        # DGEN_E_ARG
    assert L.dgen_bill_months(*args, n, None, None, st) == -1
    assert L.dgen_bill_months(*args, n, None, ctypes.byref(_lib.BillOut()), st) == -1 and "status" in _lib.last_error()
    with pytest.raises(ValueError):
        engine.bill_months(batch, kw, tf, want=("bill",))
    with pytest.raises(ValueError):
        engine.bill_months(batch, kw[:-1], tf)


@pytest.mark.parametrize("cfg_kw", [{"batt_update_hours": 1}, {"batt_loss_model": 1}], ids=["hourly_replan", "loss_model"])
def test_unsupported_dispatch_configurations_are_refused(res_case, cfg_kw):
    from dgen_amd.engine import Engine
    pop = res_case["pop"]
    eng = Engine(0, EngineConfig(**cfg_kw))
    try:
        _load(eng, pop)
        sub = subset(pop, np.arange(4))
        batch = eng.upload_agents(sub.cols, sub.n_scratch)
        kw = res_case["o"]["system_kw"][:4]
        with pytest.raises(_lib.DgenError):
            eng.bill_months(batch, kw, battery=True)
        assert "dgen_bill_months" in _lib.last_error()
        d = _host(eng.bill_months(batch, kw))            # the plain form does not depend on the dispatch
        for k in _lib.BILL_FIELDS:
            assert np.isfinite(d[k]).all(), k
    finally:
        eng.close()


def test_what_if_and_default_tariff(engine, res_case):
    c = res_case
    pop, batch, n = c["pop"], c["batch"], c["batch"].n
    _load(engine, pop)
    kw = c["out"]["x_last"]
    k = int(np.flatnonzero(pop.tariffs["flags"] == 0)[-1])
    a = _host(blm.what_if(engine, batch, kw, k))
    b = _host(engine.bill_months(batch, kw, np.full(n, k, np.int32)))
    own = _host(engine.bill_months(batch, kw))            # tariff=None: the batch's tariff0
    t0 = _host(engine.bill_months(batch, kw, pop.cols["tariff0"]))
    for m in _lib.BILL_FIELDS + ["status"]:
        assert np.array_equal(a[m], b[m], equal_nan=True), m
        assert np.array_equal(own[m], t0[m], equal_nan=True), m
    assert not a["status"].any() and not np.array_equal(a["total"], own["total"])
    assert (a["fixed_charge"] == float(pop.tariffs["fixed"][k])).all()


def test_state_monthly_sums_a_member(engine, res_case):
    _load(engine, res_case["pop"])
    n = res_case["batch"].n
    d = engine.bill_months(res_case["batch"], res_case["out"]["x_last"], res_case["out"]["tariff_final"],
                           want=("total", "import_kwh"))
    rng = np.random.default_rng(3)
    w, perm, seg_off = rng.uniform(0.0, 20.0, n), rng.permutation(n), [0, 20, 21, 50, n]
    got = blm.state_monthly(engine, d, w, perm, seg_off, members=("total", "import_kwh")).cpu().numpy()
    assert got.shape == (4, 12, 2)
    want = np.zeros_like(got)
    for q, k in enumerate(("total", "import_kwh")):
        for s in range(4):
            ix = perm[seg_off[s]:seg_off[s + 1]]
            want[s, :, q] = (res_case["dev"]["pvonly"][k][:, ix] * w[ix]).sum(axis=1)
    # the project's tolerance for fp64 segment sums (tests/test_gpu_aggregate.py)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9), np.abs(got - want).max()
    with pytest.raises(ValueError):
        blm.state_monthly(engine, d, w, perm, seg_off, members=("carry",))


def test_drop_in_switch(engine):
    from dgen_amd.columnar import columnize_frame
    from dgen_amd.engine import profile_order
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", bill_metrics=True)
    arr, _ = ff.size_chunk(df, None, table, "simple", hourly="array", bill_metrics=True)      # planes on the host
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", bill_metrics=True, max_rows=25)   # 4 sub-batches
    off, o_off = ff.size_chunk(df, None, table, "simple", hourly="none")
    # exactly COLUMNS, at the end; every other column the bits of the switch off
    assert list(non.columns) == list(off.columns) + list(blm.COLUMNS)
    assert not any(c in o_off for c in blm.COLUMNS)
    assert "baseline_net_hourly" in arr.columns and "baseline_net_hourly" not in non.columns
    numeric = [c for c in off.columns if getattr(off[c].dtype, "kind", "O") in "fiub"]
    assert {"system_kw", "npv", "payback_period", "batt_kwh", "naep"} <= set(numeric)
    for c in numeric:
        assert np.array_equal(non[c].to_numpy(), off[c].to_numpy(), equal_nan=True), c
    for c in ("cash_flow", "utility_bill_w_sys_pv_only", "utility_bill_w_sys_pv_batt", "cf_energy_value_pv_batt"):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(non[c].tolist(), off[c].tolist())), c
    for c in blm.COLUMNS:
        a = non[c].to_numpy()
        assert a.dtype == (np.int64 if "max_month" in c else np.float64), c
        assert np.array_equal(a, arr[c].to_numpy()), c
        assert np.array_equal(a, sub[c].to_numpy()), c
    # the columns are annual() of the engine calls, and the with_batt total is the frame's year-1 bill
    eng = ff.get_engine()
    cols = columnize_frame(df, store, table).frame_columns
    batch = eng.upload_agents(cols, order=profile_order(cols))
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    d = blm.bill_outputs(eng, batch, out)
    a = blm.annual(d["with_batt"])
    torch.cuda.synchronize()
    assert np.array_equal(a["total"].cpu().numpy(), non["bill_total_with_batt"].to_numpy())
    assert np.array_equal(a["max_month"].cpu().numpy(), non["bill_max_month_with_batt"].to_numpy())
    y1 = np.array([v[1] for v in non["utility_bill_w_sys_pv_batt"].tolist()])
    assert np.allclose(non["bill_total_with_batt"].to_numpy(), y1, rtol=RTOL, atol=0.0)
    y0 = np.array([v[1] for v in non["utility_bill_wo_sys_pv_batt"].tolist()])
    assert np.allclose(non["bill_total_baseline"].to_numpy(), y0, rtol=RTOL, atol=0.0)
    tot = non["bill_energy_pvonly"] - non["bill_credit_pvonly"] + non["bill_fixed_pvonly"] + non["bill_demand_pvonly"]
    assert (non["bill_total_pvonly"].to_numpy() >= tot.to_numpy() - 1e-6).all()          # the floor only adds
