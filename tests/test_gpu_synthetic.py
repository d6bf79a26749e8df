"""GPU vs CPU oracle on seeded synthetic populations of every configuration
(SURVEY 8d generator): random legacy / ur_* tariffs with tiers, NEM and net
billing, CA NEM3, DG rate-switch rows, residential and commercial loads.

Sizes are chosen so the oracle (single-thread C) finishes in seconds; the
full-size properties run on the 1M-agent bench population in
test_gpu_properties.py."""
import numpy as np
import pytest
import torch

from dgen_amd.engine import outputs_to_host
from dgen_amd.synth import make_population
from oracle import oracle as orc
from tests import helpers

pytestmark = pytest.mark.gpu

CASES = [("de_res", 300), ("res_1m_nem_tou", 600), ("ca_res_storage", 300), ("com_8m", 200),
         ("national_mixed", 400), ("metering_mix", 400), ("com_kwkw", 240)]


def _small_pop(cfg, n):
    return make_population(cfg, n, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16,
                           n_tariffs=48)


@pytest.mark.parametrize("cfg,n,long_life", [c + (False,) for c in CASES] + [("national_mixed", 300, True)])
def test_synthetic_population_matches_oracle(engine, cfg, n, long_life):
    """long_life: a third of the agents get 33..50-year analysis periods, so the
    batch runs the one-agent-per-wave year-lane kernels (otherwise two agents
    share a wave, 32 lanes each)."""
    pop = _small_pop(cfg, n)
    if long_life:
        life = pop.cols["econ_life"].copy()
        life[::3] = 33 + (np.arange(life[::3].size) % 18)
        pop.cols["econ_life"] = life
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    out = engine.alloc_outputs(batch.n, hourly=True)
    engine.size(batch, out)
    torch.cuda.synchronize()
    o = outputs_to_host(out)
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs,
                                     pop.wholesale)
    cfg_o = orc.make_cfg()
    ref = opop.run(cfg_o, hourly=True)
    n_switch = helpers.check_sized_against_oracle(o, ref, pop.cols)
    if cfg != "ca_res_storage":
        assert n_switch > 0          # the population exercises the DG switch
    if cfg == "com_kwkw":            # kWh/kW tier units on >= 30 % of the agents, all sized
        u = pop.tariffs["unit"][pop.cols["tariff0"]]
        assert np.isin(u, (1, 3)).mean() >= 0.3


@pytest.mark.parametrize("cfg,n", [("national_mixed", 3000), ("ca_res_storage", 2000)])
def test_profile_order_is_invisible(engine, cfg, n):
    """The device layout chosen by profile_order (agents grouped by cf/load row)
    returns, after outputs_to_host(out, perm), exactly the caller-order result."""
    from dgen_amd.engine import profile_order
    pop = _small_pop(cfg, n)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    res = []
    for order in (None, profile_order(pop.cols)):
        batch = engine.upload_agents(pop.cols, pop.n_scratch, order=order)
        if order is not None:
            # grouped by billing path, then load row (engine.profile_order)
            from dgen_amd.engine import path_class
            key = path_class(pop.cols).astype(np.int64)[batch.perm] * (1 << 32) + pop.cols["load_row"][batch.perm]
            assert (np.diff(key) >= 0).all()
        out = engine.alloc_outputs(batch.n, hourly=True)
        engine.size(batch, out)
        torch.cuda.synchronize()
        res.append(outputs_to_host(out, batch.perm))
    a, b = res
    for k in a:
        if a[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("cfg,n", [("ca_res_storage", 2000), ("national_mixed", 3000)])
def test_nb_prebuild_is_invisible(engine, cfg, n, monkeypatch):
    """The first-evaluation tariff's net-billing split built ahead of the
    search by k_nb_env (its LDS-staged, four-days-at-a-time form) is the split
    k_size builds itself with the prebuild off (DGEN_NB_PREBUILD=0): every
    output bit-identical, long lives (one agent per wave) included."""
    from dgen_amd.engine import Engine
    pop = _small_pop(cfg, n)
    life = pop.cols["econ_life"].copy()
    life[::5] = 33 + (np.arange(life[::5].size) % 18)
    pop.cols["econ_life"] = life
    monkeypatch.setenv("DGEN_NB_PREBUILD", "0")
    off = Engine(0)
    monkeypatch.delenv("DGEN_NB_PREBUILD")
    res = []
    try:
        for eng in (engine, off):
            eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
            eng.set_tariffs(pop.tariffs)
            eng.set_switches(pop.switches)
            batch = eng.upload_agents(pop.cols, pop.n_scratch)
            out = eng.alloc_outputs(batch.n, hourly=True)
            eng.size(batch, out)
            torch.cuda.synchronize()
            res.append(outputs_to_host(out))
            del out, batch
    finally:
        off.close()
    a, b = res
    for k in a:
        if a[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("cfg,n,long_life", [("national_mixed", 3000, False), ("national_mixed", 2000, True),
                                             ("metering_mix", 2000, False)])
def test_nem_rows_split_is_invisible(engine, cfg, n, long_life, monkeypatch):
    """A batch with scratch slots sizes its leading bins-only rows (profile
    order) with the bins-only kernels (dgen_set_nem_rows); every output equals
    the whole batch on the net-billing kernels (DGEN_NEM_SPLIT=0), bit for bit."""
    from dgen_amd.engine import profile_order
    pop = _small_pop(cfg, n)
    if long_life:
        life = pop.cols["econ_life"].copy()
        life[::4] = 33 + (np.arange(life[::4].size) % 18)
        pop.cols["econ_life"] = life
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    res = []
    for split in ("1", "0"):
        monkeypatch.setenv("DGEN_NEM_SPLIT", split)
        batch = engine.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
        assert (batch.nem_rows > 0) == (split == "1")
        out = engine.alloc_outputs(batch.n, hourly=True)
        engine.size(batch, out)
        torch.cuda.synchronize()
        res.append(outputs_to_host(out, batch.perm))
    a, b = res
    for k in a:
        if a[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("cfg,nb_scan", [("national_mixed", None), ("national_mixed", True),
                                         ("ca_res_storage", None)])
def test_pipeline_depth_is_invisible(engine, cfg, nb_scan):
    """Chunking the batch across the two-stream pipeline (k_size of chunk j+1
    beside k_hourly_batt / k_batt_finance of chunk j) changes no output bit,
    including a batch size that is not a multiple of the block size; with the
    battery-case split in k_batt_finance (national: few qualify) and in the
    hourly scan (forced, and CA-like: all qualify)."""
    pop = _small_pop(cfg, 3001)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    if nb_scan is not None:
        batch.nb_scan = nb_scan
    res = []
    engine.kernel_times()            # drain calls made by earlier tests
    try:
        for chunks in (1, 7, 16):
            engine.set_pipeline(chunks)
            out = engine.alloc_outputs(batch.n, hourly=True)
            engine.size(batch, out)
            torch.cuda.synchronize()
            res.append(outputs_to_host(out))
            _, _, _, cnt = engine.kernel_times()
            assert cnt == 1
    finally:
        from dgen_amd import _lib
        engine.set_pipeline(_lib.DEFAULT_CHUNKS)
    for r in res[1:]:
        for k in r:
            if r[k] is not None:
                assert np.array_equal(res[0][k], r[k], equal_nan=True), k


@pytest.mark.parametrize("cfg", ["national_mixed", "ca_res_storage"])
def test_hourly_segment_is_invisible(engine, cfg):
    """Sweeping the year in month-segment launches of k_hourly_batt (SOC and
    the annual PV sum carried in the workspace) changes no output bit; mixed
    population with net-billing (mo 2) agents and storage switches, and the
    CA-like one whose battery-case split is built in the scan."""
    from dgen_amd import _lib
    pop = _small_pop(cfg, 3001)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    res = []
    try:
        for months in (1, 12, 5):
            engine.set_hourly_segment(months)
            out = engine.alloc_outputs(batch.n, hourly=True)
            engine.size(batch, out)
            torch.cuda.synchronize()
            res.append(outputs_to_host(out))
    finally:
        engine.set_hourly_segment(_lib.DEFAULT_HOURLY_MONTHS)
    for r in res[1:]:
        for k in r:
            if r[k] is not None:
                assert np.array_equal(res[0][k], r[k], equal_nan=True), k


@pytest.mark.parametrize("cfg", ["de_res", "ca_res_storage"])
def test_pv_only_variant(engine, cfg):
    """dgen_set_battery(0) (SURVEY 8(d) PV-only variant): the search and every
    PV-only output are bit-identical to the reference run's, no battery is
    sized, the with-battery plane is the PV-only net load at kW*, and
    k_batt_finance does not run (npv_pv_batt NaN)."""
    pop = _small_pop(cfg, 300)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    res = []
    try:
        for on in (True, False):
            engine.set_battery(on)
            out = engine.alloc_outputs(batch.n, hourly=True)
            engine.size(batch, out)
            torch.cuda.synchronize()
            res.append(outputs_to_host(out))
    finally:
        engine.set_battery(True)
    a, b = res
    for k in ("system_kw", "x_last", "nfev", "npv", "payback_period", "first_with", "first_without",
              "annual_kwh", "naep", "baseline", "net_pvonly", "cash_flow", "bill_w_pv", "bill_wo_pv"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert (b["batt_kw"] == 0).all() and (b["batt_kwh"] == 0).all() and np.isnan(b["npv_pv_batt"]).all()
    # no battery: with-battery plane = max(load - pv(kW*), 0)
    kw = b["system_kw"]
    shp, cf = pop.shapes[pop.cols["load_row"]].astype(np.float64), pop.cfs[pop.cols["cf_row"]] / 1e6
    load = shp * (pop.cols["load_kwh"] / shp.sum(axis=1))[:, None]
    pv = cf * (((kw * 1000.0) * 0.96) / 1000.0)[:, None]
    ref = np.maximum(load - pv, 0.0).astype(np.float32)
    assert np.allclose(b["net_with_batt"], ref, rtol=1e-5, atol=1e-4)


def test_hourly_f64_planes(engine):
    """dgen_outputs.hourly_f64: the planes as doubles are the values the scan
    computes -- rounding them to float32 gives the float32 planes bit for bit --
    and they match the oracle's fp64 hourly outputs to 1e-12; the per-state
    export reads either tile type."""
    from dgen_amd.attachment import state_hourly
    pop = _small_pop("national_mixed", 300)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    o32 = engine.alloc_outputs(batch.n, hourly=True)
    o64 = engine.alloc_outputs(batch.n, hourly=True, hourly_f64=True)
    engine.size(batch, o32)
    engine.size(batch, o64)
    torch.cuda.synchronize()
    for k in ("baseline", "net_pvonly", "net_with_batt"):
        assert o64[k].dtype == torch.float64
        assert torch.equal(o64[k].to(torch.float32), o32[k]), k
    h = outputs_to_host(o64)
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs,
                                     pop.wholesale)
    ref = opop.run(orc.make_cfg(), hourly=True)
    for i, r in enumerate(ref):
        for k_o, k_r in (("net_pvonly", "adopter_net_hourly_pvonly"),
                         ("net_with_batt", "adopter_net_hourly_with_batt")):
            a, b = h[k_o][i], np.asarray(r[k_r], float)
            assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(b).max())), (i, k_o)
    n = batch.n
    w = tuple(torch.rand(n, dtype=torch.float64, device=engine.dev) for _ in range(3))
    seg = [0, n // 3, n]
    s32 = state_hourly(engine, (o32["baseline"], o32["net_pvonly"], o32["net_with_batt"]), w, None, seg)
    s64 = state_hourly(engine, (o64["baseline"], o64["net_pvonly"], o64["net_with_batt"]), w, None, seg)
    assert torch.allclose(s32, s64, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("cfg", ["ca_res_storage", "metering_mix"])
def test_nb_scan_split_equals_finance_build(engine, cfg):
    """The battery case's net-billing split built in k_hourly_batt's scan
    (dgen_set_nb_scan(1)) bills like the split k_batt_finance builds from the
    system-output plane (0): the same hours, sums re-associated (1e-9), and
    every PV-only / hourly output bit-identical."""
    pop = _small_pop(cfg, 600)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    assert batch.n_scratch > 0
    res = []
    try:
        for on in (True, False):
            batch.nb_scan = on
            out = engine.alloc_outputs(batch.n, hourly=True)
            engine.size(batch, out)
            torch.cuda.synchronize()
            res.append(outputs_to_host(out))
    finally:
        batch.nb_scan = True
    a, b = res
    for k in ("system_kw", "npv", "nfev", "baseline", "net_pvonly", "net_with_batt", "batt_kwh"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("npv_pv_batt", "bill_w_batt", "bill_wo_batt", "cfev_batt"):
        assert np.allclose(a[k], b[k], rtol=1e-9, atol=1e-9, equal_nan=True), k


def test_nb_scan_overflow_repair_pass(engine):
    """A scan-built split that overflows its per-month capacity (forced here
    with a capacity of 2 mixed hours) leaves no system-output plane behind;
    the repair pass writes it and k_batt_finance bills exactly as with the
    split built from the plane (bit-identical), every other output unchanged."""
    from dgen_amd import _lib
    pop = _small_pop("ca_res_storage", 400)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    res = []
    try:
        for on, cap in ((False, 0), (True, 2)):
            batch.nb_scan = on
            out = engine.alloc_outputs(batch.n, hourly=True)
            engine.size(batch, out)                    # sets the engine's nb_scan state
            _lib.check(engine.lib.dgen_set_nb_scan(engine.ctx, cap), "dgen_set_nb_scan")
            engine.size(batch, out)
            torch.cuda.synchronize()
            res.append(outputs_to_host(out))
    finally:
        _lib.check(engine.lib.dgen_set_nb_scan(engine.ctx, _lib.NB_CAPM), "dgen_set_nb_scan")
        engine._nb_scan = True
        batch.nb_scan = True
    a, b = res
    for k, v in a.items():
        if v is not None:
            assert np.array_equal(v, b[k], equal_nan=True), k


@pytest.mark.parametrize("cfg,n", [("res_1m_nem_tou", 300), ("ca_res_storage", 200), ("com_8m", 160),
                                   ("national_mixed", 300)])
def test_hourly_replan_matches_oracle(engine_hourly_plan, cfg, n):
    """The peak-shaving target re-planned every hour over the next 24 hours
    (batt_update_hours = 1, k_hourly_batt<ROLL>) against the oracle's rule:
    the battery-case planes, bills, NPV; the PV-only search is unchanged."""
    eng = engine_hourly_plan
    pop = _small_pop(cfg, n)
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs)
    eng.set_switches(pop.switches)
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    out = eng.alloc_outputs(batch.n, hourly=True)
    eng.size(batch, out)
    torch.cuda.synchronize()
    o = outputs_to_host(out)
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs,
                                     pop.wholesale)
    ref = opop.run(orc.make_cfg(batt_update_hours=1), hourly=True)
    daily = opop.run(orc.make_cfg(), hourly=True, idx=range(min(n, 40)))
    moved = 0
    for i, r in enumerate(ref):
        assert o["status"][i] == 0 and r["status"] == 0, i
        # every agent on the oracle's Brent path (round 5's knife-edge com_8m
        # agent 5 included: certified paths)
        assert helpers.same_path(o, i, r), (i, o["nfev"][i], r["nfev"], o["x_last"][i], r["x_last"])
        assert abs(o["system_kw"][i] - r["system_kw"]) <= 1e-9 * r["system_kw"], i
        assert np.isclose(o["npv"][i], r["npv"], rtol=1e-6, atol=1e-6), (i, o["npv"][i], r["npv"])
        for k in ("batt_kwh", "npv_pv_batt"):
            assert np.isclose(o[k][i], r[k], rtol=1e-6, atol=1e-6), (i, k, o[k][i], r[k])
        N1 = int(pop.cols["econ_life"][i]) + 1
        for k_o, k_r in (("cfev_batt", "cf_energy_value_pv_batt"), ("bill_w_batt", "bill_w_pv_batt")):
            assert np.allclose(o[k_o][i, :N1], r[k_r], rtol=1e-6, atol=1e-5), (i, k_o)
        ref_h = r["adopter_net_hourly_with_batt"]
        assert np.allclose(o["net_with_batt"][i], ref_h, rtol=1e-5,
                           atol=1e-5 * max(1.0, np.abs(ref_h).max())), i
        if i < len(daily):
            moved += not np.allclose(daily[i]["adopter_net_hourly_with_batt"], ref_h)
    assert moved > 0                 # the re-plan interval changes the dispatch


def test_battery_case_independent_of_batch(engine):
    """The battery case's net-billing split is built in the scan for every
    agent that bills net without a TS sell rate (decided per agent, not per
    batch): an agent's battery-case outputs are bit-identical whether it is
    sized in the national batch, in a batch of its own state's (CA) agents or
    alone."""
    from dgen_amd.engine import profile_order
    pop = _small_pop("national_mixed", 1500)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    keys = ("npv_pv_batt", "bill_w_batt", "bill_wo_batt", "cfev_batt", "npv", "system_kw", "batt_kwh")

    def run(idx):
        cols = {k: np.asarray(v)[idx] for k, v in pop.cols.items()}
        batch = engine.upload_agents(cols, order=profile_order(cols))
        out = engine.alloc_outputs(batch.n, hourly=False)
        engine.size(batch, out)
        torch.cuda.synchronize()
        return outputs_to_host(out, batch.perm)

    ca = np.flatnonzero((pop.cols["flags"] & 2) != 0)
    assert ca.size >= 20
    full = run(np.arange(1500))
    part = run(ca)
    for k in keys:
        assert np.array_equal(full[k][ca], part[k], equal_nan=True), k
    for j in list(ca[:4]) + [int(np.flatnonzero((pop.cols["flags"] & 2) == 0)[0])]:
        one = run(np.array([j]))
        for k in keys:
            assert np.array_equal(full[k][j], one[k][0], equal_nan=True), (j, k)


@pytest.mark.parametrize("cfg,n,replan", [("ca_res_storage", 300, 24), ("national_mixed", 400, 24),
                                          ("res_1m_nem_tou", 300, 1)])
def test_li_ion_loss_model_matches_oracle(cfg, n, replan):
    """The Li-ion loss model option (batt_loss_model = 1: converters + cell
    I^2 R at an SOC-dependent open-circuit voltage) in
    k_hourly_batt<LOSS> against the oracle's dispatch, with a resistance large
    enough to move the dispatch."""
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine
    kw = dict(batt_loss_model=1, batt_r_cell=0.02, batt_update_hours=replan)
    eng = Engine(0, EngineConfig(**kw))
    try:
        pop = _small_pop(cfg, n)
        eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
        eng.set_tariffs(pop.tariffs)
        eng.set_switches(pop.switches)
        batch = eng.upload_agents(pop.cols, pop.n_scratch)
        out = eng.alloc_outputs(batch.n, hourly=True)
        eng.size(batch, out)
        torch.cuda.synchronize()
        o = outputs_to_host(out)
    finally:
        eng.close()
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale)
    ref = opop.run(orc.make_cfg(**kw), hourly=True)
    base = opop.run(orc.make_cfg(batt_update_hours=replan), hourly=True)
    moved = 0
    for i, (r, b) in enumerate(zip(ref, base)):
        assert o["status"][i] == 0 and r["status"] == 0, i
        for k in ("npv_pv_batt", "batt_kwh", "first_with", "npv"):
            assert np.isclose(o[k][i], r[k], rtol=1e-6, atol=1e-6), (i, k, o[k][i], r[k])
        N1 = int(pop.cols["econ_life"][i]) + 1
        assert np.allclose(o["bill_w_batt"][i, :N1], r["bill_w_pv_batt"], rtol=1e-6, atol=1e-5), i
        ref_h = r["adopter_net_hourly_with_batt"]
        assert np.allclose(o["net_with_batt"][i], ref_h, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref_h).max())), i
        moved += not np.allclose(ref_h, b["adopter_net_hourly_with_batt"], rtol=1e-9, atol=1e-9)
    assert moved > 0


@pytest.mark.parametrize("replan", [24, 1])
def test_month_floor_matches_oracle(replan):
    """batt_month_floor = 1 (the monthly peak-shaving target floor) in
    k_hourly_batt against the oracle, daily plan and hourly re-plan."""
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine
    kw = dict(batt_month_floor=1, batt_update_hours=replan)
    eng = Engine(0, EngineConfig(**kw))
    try:
        pop = _small_pop("national_mixed", 300)
        eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
        eng.set_tariffs(pop.tariffs)
        eng.set_switches(pop.switches)
        batch = eng.upload_agents(pop.cols, pop.n_scratch)
        out = eng.alloc_outputs(batch.n, hourly=True)
        eng.size(batch, out)
        torch.cuda.synchronize()
        o = outputs_to_host(out)
    finally:
        eng.close()
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale)
    ref = opop.run(orc.make_cfg(**kw), hourly=True)
    base = opop.run(orc.make_cfg(batt_update_hours=replan), hourly=True)
    moved = 0
    for i, (r, b) in enumerate(zip(ref, base)):
        assert o["status"][i] == 0 and r["status"] == 0, i
        assert np.isclose(o["npv_pv_batt"][i], r["npv_pv_batt"], rtol=1e-6, atol=1e-6), i
        ref_h = r["adopter_net_hourly_with_batt"]
        assert np.allclose(o["net_with_batt"][i], ref_h, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref_h).max())), i
        moved += not np.allclose(ref_h, b["adopter_net_hourly_with_batt"], rtol=1e-9, atol=1e-9)
    assert moved > 0
