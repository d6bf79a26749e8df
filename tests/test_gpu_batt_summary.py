"""Battery dispatch summary on the GPU: dgen_batt_summary against the numpy
reference on the oracle's dispatch (tests/test_batt_metrics.summary_ref) at the
device's own sizes, its grid-to-load sum against the scan's with-battery plane
bit for bit, the edges the header names, and its way up through
Engine.batt_summary, dgen_amd.batt_metrics and the drop-in switch
size_frame / size_chunk(batt_metrics=True)."""
import ctypes

import numpy as np
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import batt_metrics as bm
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig
from dgen_amd.synth import make_population, subset
from oracle import oracle as orc
from tests.test_batt_metrics import summary_ref
from tests.test_grid_metrics import MONTH_START

pytestmark = pytest.mark.gpu

# the project's tolerances (tests/test_gpu_parity.py): 1e-6 relative on energy, 1e-6 absolute on fractions
RTOL = ATOL = 1e-6
RES_N = (1, 63, 65, 257)         # one lane; a 64-lane block less one lane, and plus one; five blocks with a ragged tail
RES_SEED, COM_SEED = 20260003, 20260007      # seeds at which the reference leaves out <= 1 % of the agents (CPU check)


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


def _load(eng, pop):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs)
    eng.set_switches(pop.switches)


def _size(eng, pop, hourly=False, f64=False):
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    out = eng.alloc_outputs(batch.n, hourly=hourly, hourly_f64=f64)
    eng.size(batch, out)
    return batch, out


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def agent_hours(pop, i, kw, ssum):
    """load and pv of agent i at kw, formed as the header defines them."""
    c = pop.cols
    lr, cr = int(c["load_row"][i]), int(c["cf_row"][i])
    ls = float(c["load_kwh"][i]) / float(ssum[lr])
    cs6 = (((float(kw) * 1000.0) * 0.96) / 1000.0) / 1e6
    return pop.shapes[lr].astype(np.float64) * ls, pop.cfs[cr].astype(np.float64) * cs6


def reference(pop, kw, ssum, cfg_o, battery=True, midday=_lib.BATT_SUMMARY_MIDDAY):
    """summary_ref of every agent at kw[i]: ({member: [12, n]}, ambiguous [n],
    bank [n], power [n]).  ambiguous: the reference puts some hour's tested
    quantity within 1 % of a band's width of its threshold -- 1e-11 around the
    two SOC thresholds, 1e-8 kW around the surplus / deficit thresholds, 1e-11
    x power around the discharge power threshold -- so rounding decides the
    hour's count."""
    n = len(kw)
    res = {k: np.zeros((12, n), np.float64 if k in _lib.BATT_SUMMARY_F64 else np.int32) for k in _lib.BATT_SUMMARY_FIELDS}
    amb, banks, powers = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    for i in range(n):
        load, pv = agent_hours(pop, i, kw[i], ssum)
        bank = power = 0.0
        if battery:
            bank, power = orc.batt_size(kw[i] / 0.8 / 2.0, kw[i] / 0.8, 240.0 if pop.cols["flags"][i] & 1 else 500.0, cfg_o)
        r = summary_ref(load, pv, bank, power, cfg_o, midday)
        for k in _lib.BATT_SUMMARY_FIELDS:
            res[k][:, i] = r[k]
        h = r["_hours"]
        amb[i] = (np.abs(h["soc"] - (cfg_o.batt_max_soc - 1e-9)).min() <= 1e-11
                  or np.abs(h["soc"] - (cfg_o.batt_min_soc + 1e-9)).min() <= 1e-11
                  or np.abs(h["sur"] - 1e-6).min() <= 1e-8 or np.abs(h["sur"] - (power + 1e-6)).min() <= 1e-8
                  or np.abs(h["nn"] - 1e-6).min() <= 1e-8
                  or (power > 0.0 and np.abs(h["d"] - power * (1.0 - 1e-9)).min() <= 1e-11 * power))
        banks[i], powers[i] = bank, power
    return res, amb, banks, powers


def compare(dev, ref, amb, what):
    """kWh members 1e-6 relative, SOC members 1e-6 absolute, counts exact on
    the agents the reference does not call ambiguous (at most 1 % may be)."""
    worst = {}
    for k in _lib.BATT_SUMMARY_F64:
        a, r = dev[k], ref[k]
        assert a.shape == r.shape and a.dtype == np.float64, (what, k)
        err = np.abs(a - r)
        worst[k] = float(err.max()) if k.startswith("soc") else float((err / np.maximum(np.abs(r), 1.0)).max())
    print(f"{what}: worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert amb.sum() * 100 <= amb.size, (what, int(amb.sum()), amb.size)
    keep = ~amb
    diff = {k: int((dev[k][:, keep] != ref[k][:, keep]).any(axis=0).sum()) for k in _lib.BATT_SUMMARY_I32}
    print(f"{what}: agents left out {int(amb.sum())} of {amb.size}; agents with a differing count: {diff}")
    for k in _lib.BATT_SUMMARY_F64:
        if k.startswith("soc"):
            assert np.allclose(dev[k], ref[k], rtol=0.0, atol=ATOL), (what, k, worst[k])
        else:
            assert np.allclose(dev[k], ref[k], rtol=RTOL, atol=ATOL), (what, k, worst[k])
    for k in _lib.BATT_SUMMARY_I32:
        assert dev[k].dtype == np.int32
        assert np.array_equal(dev[k][:, keep], ref[k][:, keep]), (what, k, diff[k])


@pytest.fixture(scope="module")
def res_case(engine):
    """The 257-agent residential NEM population sized once on the device, its
    summary, and the reference at the device's sizes (computed once, shared)."""
    pop = _pop("res_1m_nem_tou", max(RES_N), RES_SEED)
    _load(engine, pop)
    batch, out = _size(engine, pop, hourly=True, f64=True)
    d = _host(engine.batt_summary(batch, out))
    kw, st = out["system_kw"].cpu().numpy(), out["status"].cpu().numpy()
    assert (st == 0).all()
    ssum, _ = engine.profile_sums()
    cfg_o = orc.make_cfg()
    ref, amb, bank, power = reference(pop, kw, ssum, cfg_o)
    return {"pop": pop, "batch": batch, "out": out, "dev": d, "kw": kw, "ssum": ssum, "ref": ref, "amb": amb,
            "bank": bank, "power": power}


@pytest.mark.parametrize("n", RES_N)
def test_residential_population_matches_the_reference(engine, res_case, n):
    pop = res_case["pop"]
    if n == pop.cols["load_kwh"].size:
        dev, kw = res_case["dev"], res_case["kw"]
        assert np.allclose(res_case["out"]["batt_kwh"].cpu().numpy(), res_case["bank"], rtol=1e-12, atol=0.0)
        assert (res_case["bank"] > 0).all() and (res_case["ref"]["hours_soc_bound"].sum(axis=0) > 0).any()
    else:
        sub = subset(pop, np.arange(n))
        _load(engine, pop)
        batch, out = _size(engine, sub)
        dev = _host(engine.batt_summary(batch, out))
        kw = out["system_kw"].cpu().numpy()
        # an agent's size does not depend on its batch: the shared reference holds
        assert np.array_equal(kw, res_case["kw"][:n])
    assert all(v.shape == (12, n) for v in dev.values()) and sorted(dev) == sorted(_lib.BATT_SUMMARY_FIELDS)
    ref = {k: v[:, :n] for k, v in res_case["ref"].items()}
    amb = res_case["amb"][:n]
    if n < 100:                  # fewer than 100 agents: 1 % is none of them
        assert not amb.any()
    compare(dev, ref, amb, f"res n={n}")
    # the month's load is what PV, battery and grid delivered
    tot = dev["pv_to_load_kwh"] + dev["batt_to_load_kwh"] + dev["grid_to_load_kwh"]
    for i in range(min(n, 8)):
        load, _ = agent_hours(pop, i, kw[i], res_case["ssum"])
        want = np.array([load[MONTH_START[m]:MONTH_START[m + 1]].sum() for m in range(12)])
        assert np.allclose(tot[:, i], want, rtol=1e-9), i


def test_commercial_population_matches_the_reference(engine):
    """500 V banks (ceil(500 / 3.6) cells in series)."""
    pop = _pop("com_8m", 64, COM_SEED)
    assert not (pop.cols["flags"] & 1).any()
    _load(engine, pop)
    batch, out = _size(engine, pop)
    dev = _host(engine.batt_summary(batch, out))
    assert (out["status"].cpu().numpy() == 0).all()
    ref, amb, bank, _ = reference(pop, out["system_kw"].cpu().numpy(), engine.profile_sums()[0], orc.make_cfg())
    assert np.allclose(out["batt_kwh"].cpu().numpy(), bank, rtol=1e-12, atol=0.0) and (bank > 0).all()
    assert not amb.any()
    compare(dev, ref, amb, "com n=64")


def test_replay_equals_the_scan(engine, res_case):
    """grid_to_load_kwh is the with-battery plane's monthly import, bit for
    bit: both are sequential fp64 sums of batt_hour's g2l in hour order."""
    _load(engine, res_case["pop"])           # the session's engine holds the tables of whichever test ran last
    out = res_case["out"]
    assert out["net_with_batt"].dtype == torch.float64
    scan = engine.plane_digest(out["net_with_batt"], want=("import_kwh", "export_kwh"))
    d = engine.batt_summary(res_case["batch"], out, want=("grid_to_load_kwh",))
    torch.cuda.synchronize()
    assert not scan["export_kwh"].any().item()
    assert (scan["import_kwh"] > 0).all().item()
    assert torch.equal(d["grid_to_load_kwh"], scan["import_kwh"])


def test_two_runs_are_bit_identical_and_midday_window(engine, res_case):
    _load(engine, res_case["pop"])
    batch, out = res_case["batch"], res_case["out"]
    a = _host(engine.batt_summary(batch, out))
    for k, v in res_case["dev"].items():
        assert np.array_equal(a[k], v), k
    w = _host(engine.batt_summary(batch, out, midday=(0, 23)))
    for k in ("surplus", "pv_to_batt", "pv_to_grid"):
        assert np.array_equal(w[f"{k}_mid_kwh"], w[f"{k}_kwh"]), k
        assert np.array_equal(w[f"{k}_kwh"], a[f"{k}_kwh"]), k
        assert (a[f"{k}_mid_kwh"] <= a[f"{k}_kwh"]).all(), k
    one = _host(engine.batt_summary(batch, out, want=("surplus_mid_kwh",), midday=(12, 12)))
    assert (one["surplus_mid_kwh"] <= a["surplus_mid_kwh"]).all() and (one["surplus_mid_kwh"] > 0).any()
    with pytest.raises(ValueError):
        engine.batt_summary(batch, out, midday=(15, 11))
    with pytest.raises(ValueError):
        engine.batt_summary(batch, out, midday=(0, 24))
    with pytest.raises(ValueError):
        engine.batt_summary(batch, out, want=("soc",))


def test_state_monthly_sums_the_kwh_members(engine, res_case):
    _load(engine, res_case["pop"])
    n = res_case["batch"].n
    d = engine.batt_summary(res_case["batch"], res_case["out"], want=bm.KWH_MEMBERS)
    rng = np.random.default_rng(3)
    w, perm, seg_off = rng.uniform(0.0, 20.0, n), rng.permutation(n), [0, 40, 41, 200, n]
    got = bm.state_monthly(engine, d, w, perm, seg_off).cpu().numpy()
    assert got.shape == (4, 12, len(bm.KWH_MEMBERS)) and len(bm.KWH_MEMBERS) == 10
    want = np.zeros_like(got)
    for q, k in enumerate(bm.KWH_MEMBERS):
        for s in range(4):
            ix = perm[seg_off[s]:seg_off[s + 1]]
            want[s, :, q] = (res_case["dev"][k][:, ix] * w[ix]).sum(axis=1) / 1000.0
    assert want[..., 0].min() > 0
    # the project's tolerance for fp64 segment sums (tests/test_gpu_aggregate.py)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9), np.abs(got - want).max()
    with pytest.raises(ValueError):
        bm.state_monthly(engine, d, w, perm, seg_off, members=("soc_min",))


def test_null_members_and_arguments(engine, res_case):
    _load(engine, res_case["pop"])
    batch, out = res_case["batch"], res_case["out"]
    n = batch.n
    bufs = {k: torch.full((12, n), -7.0, dtype=torch.float64, device=engine.dev) for k in _lib.BATT_SUMMARY_F64}
    bufs.update({k: torch.full((12, n), -7, dtype=torch.int32, device=engine.dev) for k in _lib.BATT_SUMMARY_I32})
    wanted = ("pv_to_batt_kwh", "soc_end", "hours_empty")
    so = _lib.BattSummaryOut(**{k: bufs[k].data_ptr() for k in wanted})
    co = engine.c_outputs(out)
    L, st = engine.lib, engine.stream_handle()
    args = (engine.ctx, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents), ctypes.byref(co))
    assert L.dgen_batt_summary(*args, n, None, ctypes.byref(so), st) == 0, _lib.last_error()      # NULL opt: 11..15
    torch.cuda.synchronize()
    for k in _lib.BATT_SUMMARY_FIELDS:
        a = bufs[k].cpu().numpy()
        if k in wanted:
            assert np.array_equal(a, res_case["dev"][k]), k
        else:
            assert (a == -7).all(), k
    assert L.dgen_batt_summary(*args, 0, None, ctypes.byref(so), st) == 0                        # n = 0: no launch
    assert L.dgen_batt_summary(*args, -1, None, ctypes.byref(so), st) == -1                      # DGEN_E_ARG
    assert L.dgen_batt_summary(*args, n, None, None, st) == -1
    for lo, hi in ((12, 11), (-1, 5), (3, 24)):
        opt = _lib.BattSummaryOpt(lo, hi)
        assert L.dgen_batt_summary(*args, n, ctypes.byref(opt), ctypes.byref(so), st) == -1, (lo, hi)
        assert "midday" in _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bufs["soc_end"].cpu().numpy(), res_case["dev"]["soc_end"])


def test_flagged_agent_writes_zeros_and_leaves_its_neighbours(engine, res_case):
    """A life outside 1..50 (DGEN_ST_YEARS): zeros in every member; every other
    agent's summary is the bits of the batch without it."""
    pop = res_case["pop"]
    n, rows = 130, np.array([0, 64, 77, 129])
    sub = subset(pop, np.arange(n))
    life = sub.cols["econ_life"].copy()
    life[rows] = [51, 0, 51, -3]
    sub.cols["econ_life"] = life
    _load(engine, pop)
    batch, out = _size(engine, sub)
    d = _host(engine.batt_summary(batch, out))
    st = out["status"].cpu().numpy()
    assert (st[rows] == _lib.ST_YEARS).all() and (np.delete(st, rows) == 0).all()
    others = np.setdiff1d(np.arange(n), rows)
    for k in _lib.BATT_SUMMARY_FIELDS:
        assert not d[k][:, rows].any(), k
        assert np.array_equal(d[k][:, others], res_case["dev"][k][:, others]), k


def test_battery_off(engine, res_case):
    """dgen_set_battery(0): no flow, the SOC members are batt_init_soc and the
    grid serves every deficit."""
    pop, n = res_case["pop"], 70
    sub = subset(pop, np.arange(n))
    _load(engine, pop)
    engine.set_battery(False)
    try:
        batch, out = _size(engine, sub)
        d = _host(engine.batt_summary(batch, out))
        kw = out["system_kw"].cpu().numpy()
    finally:
        engine.set_battery(True)
    assert np.array_equal(kw, res_case["kw"][:n])
    for k in ("pv_to_batt_kwh", "batt_to_load_kwh", "pv_to_batt_mid_kwh", "hours_charge", "hours_discharge",
              "hours_soc_bound", "hours_discharge_power_bound"):
        assert not d[k].any(), k
    for k in ("soc_min", "soc_max", "soc_end"):
        assert (d[k] == engine.cfg.batt_init_soc).all(), k
    assert np.array_equal(d["pv_to_grid_kwh"], d["surplus_kwh"])
    for i in range(n):
        load, pv = agent_hours(pop, i, kw[i], res_case["ssum"])
        g = np.maximum(load - pv, 0.0)
        want = np.array([np.cumsum(g[MONTH_START[m]:MONTH_START[m + 1]])[-1] for m in range(12)])
        assert np.array_equal(d["grid_to_load_kwh"][:, i], want), i
    ref, amb, _, _ = reference(pop, kw, res_case["ssum"], orc.make_cfg(), battery=False)
    compare(d, ref, amb, "battery off n=70")


@pytest.fixture(scope="module")
def engine_floor():
    from dgen_amd.engine import Engine
    eng = Engine(0, EngineConfig(batt_month_floor=1))
    yield eng
    eng.close()


def test_month_floor_matches_the_reference(engine_floor, res_case):
    pop, n = res_case["pop"], 65
    sub = subset(pop, np.arange(n))
    _load(engine_floor, pop)
    batch, out = _size(engine_floor, sub)
    d = _host(engine_floor.batt_summary(batch, out))
    kw = out["system_kw"].cpu().numpy()
    assert (out["status"].cpu().numpy() == 0).all()
    ref, amb, _, _ = reference(pop, kw, engine_floor.profile_sums()[0], orc.make_cfg(batt_month_floor=1))
    assert not amb.any()
    compare(d, ref, amb, "month floor n=65")
    # the floor changes the dispatch: not the default configuration's summary
    assert np.array_equal(kw, res_case["kw"][:n])
    assert not np.array_equal(d["batt_to_load_kwh"], res_case["dev"]["batt_to_load_kwh"][:, :n])


@pytest.mark.parametrize("cfg_kw", [{"batt_update_hours": 1}, {"batt_loss_model": 1}], ids=["hourly_replan", "loss_model"])
def test_unsupported_dispatch_configurations_are_refused(res_case, cfg_kw):
    from dgen_amd.engine import Engine
    pop = res_case["pop"]
    eng = Engine(0, EngineConfig(**cfg_kw))
    try:
        _load(eng, pop)
        sub = subset(pop, np.arange(4))
        batch = eng.upload_agents(sub.cols, sub.n_scratch)
        out = eng.alloc_outputs(batch.n, hourly=False)
        co = eng.c_outputs(out)
        so = _lib.BattSummaryOut()
        rc = eng.lib.dgen_batt_summary(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), ctypes.byref(co),
                                       batch.n, None, ctypes.byref(so), eng.stream_handle())
        assert rc == -1                                      # DGEN_E_ARG
        assert "dgen_batt_summary" in _lib.last_error()
        with pytest.raises(_lib.DgenError):
            eng.batt_summary(batch, out)
    finally:
        eng.close()


def test_drop_in_switch(engine):
    from dgen_amd.columnar import columnize_frame
    from dgen_amd.engine import profile_order
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    non, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_metrics=True)
    arr, _ = ff.size_chunk(df, None, table, "simple", hourly="array", batt_metrics=True)
    assert list(non.columns)[-len(bm.COLUMNS):] == list(bm.COLUMNS)
    assert "baseline_net_hourly" in arr.columns and "baseline_net_hourly" not in non.columns
    for c in bm.COLUMNS:
        a = non[c].to_numpy()
        assert a.dtype == (np.int64 if c[len(bm.PREFIX):] in bm.COUNT_MEMBERS else np.float64), c
        assert np.array_equal(a, arr[c].to_numpy()), c
    # three sub-batches, and the agents evaluated at the sizes found
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_metrics=True, max_rows=40)
    assert np.isfinite(non["system_kw"].to_numpy()).all()
    fix, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_metrics=True,
                           fixed_kw=non["system_kw"].to_numpy())
    for c in bm.COLUMNS:
        assert np.array_equal(sub[c].to_numpy(), non[c].to_numpy()), c
        assert np.array_equal(fix[c].to_numpy(), non[c].to_numpy()), c
    # the columns are annual() of the engine call
    eng = ff.get_engine()
    cols = columnize_frame(df, store, table).frame_columns
    batch = eng.upload_agents(cols, order=profile_order(cols))
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    d = bm.summary_outputs(eng, batch, out)
    inv = np.empty(batch.n, np.int64)
    inv[batch.perm] = np.arange(batch.n)
    a = bm.annual(d, out["batt_kwh"].index_select(0, torch.as_tensor(inv, device=eng.dev)), eng.cfg)
    torch.cuda.synchronize()
    assert np.array_equal(out["system_kw"].cpu().numpy()[inv], non["system_kw"].to_numpy())
    for k in bm.ANNUAL:
        assert np.array_equal(a[k].cpu().numpy(), non[bm.PREFIX + k].to_numpy()), k
    assert (non["batt_diag_pv_to_batt_kwh"] > 0).any() and (non["batt_diag_equiv_full_cycles"] > 0).any()
    assert ((non["batt_diag_self_sufficiency_frac"] >= 0) & (non["batt_diag_self_sufficiency_frac"] <= 1)).all()
    # the switch off: the frame it always was, column for column
    off, o_off = ff.size_chunk(df, None, table, "simple", hourly="none")
    assert not any(c.startswith(bm.PREFIX) for c in off.columns) and not any(c in o_off for c in bm.COLUMNS)
    assert list(off.columns) == [c for c in non.columns if c not in bm.COLUMNS]
    for k in ("system_kw", "npv", "batt_kwh", "payback_period"):
        assert np.array_equal(off[k].to_numpy(), non[k].to_numpy(), equal_nan=True), k
