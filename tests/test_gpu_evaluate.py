"""Evaluation at caller-given sizes on the GPU (dgen_eval_agents,
dgen_objective_curve, size_frame(fixed_kw=...)): against the CPU oracle's
orc_eval_at, against the search's own last evaluation, point by point against
itself, across the call forms, and through the drop-in frame API."""
import ctypes

import numpy as np
import pytest
import torch

from dgen_amd import _lib
from dgen_amd.engine import outputs_to_host
from dgen_amd.synth import make_population
from oracle import oracle as orc
from tests import helpers

pytestmark = pytest.mark.gpu

PV_YEARLY = ("cash_flow", "cfev_pv", "bill_w_pv", "bill_wo_pv")


def _small_pop(cfg, n):
    return make_population(cfg, n, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16,
                           n_tariffs=48)


def _load(eng, pop, demand=None):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, demand)
    eng.set_switches(pop.switches)
    return eng.upload_agents(pop.cols, pop.n_scratch)


def _max_load(pop):
    """load_kwh / naep per agent: the centre of the search's bracket [0.8, 1.25]."""
    naep = (pop.cfs.astype(np.float64) / 1e6).sum(axis=1)
    return pop.cols["load_kwh"] / naep[pop.cols["cf_row"]]


def _sizes(pop, seed):
    u = np.random.default_rng(seed).uniform(0.5, 1.5, len(pop.cols["load_kwh"]))
    return u, u * _max_load(pop)


def _evaluate(eng, batch, kw, hourly=True):
    out = eng.alloc_outputs(batch.n, hourly=hourly)
    eng.evaluate(batch, out, kw)
    torch.cuda.synchronize()
    return outputs_to_host(out)


def _check_against_oracle(o, kw, pop, opop, n_exempt_max):
    """Every agent against orc_eval_at at its size from the initial tariff
    state, with test_synthetic_population_matches_oracle's tolerances."""
    cfg_o = orc.make_cfg()
    n_switch = n_exempt = 0
    for i in range(len(kw)):
        r = opop.eval_at(cfg_o, i, kw[i], kw[i], int(pop.cols["tariff0"][i]), 0, hourly=True)
        assert o["status"][i] == 0 and r["status"] == 0, i
        assert o["nfev"][i] == 1, i
        # the caller's size, bit for bit
        assert o["system_kw"][i].tobytes() == o["x_last"][i].tobytes() == np.float64(kw[i]).tobytes(), i
        assert o["tariff_final"][i] == r["tariff_final"], i
        assert o["switched"][i] == r["switched"], i
        n_switch += int(r["switched"])
        for k in ("npv", "annual_kwh", "first_with", "first_without", "batt_kwh", "batt_kw", "npv_pv_batt"):
            assert np.isclose(o[k][i], r[k], rtol=1e-6, atol=1e-6), (i, k, o[k][i], r[k])
        # np.round(payback, 1) sits on a knife edge when 10 x payback is a
        # half-integer: those (few) agents are compared on the raw value
        t = 10.0 * r["payback_raw"]
        if np.isfinite(t) and abs(t - np.floor(t) - 0.5) <= 1e-6:
            n_exempt += 1
            assert np.isclose(o["payback_raw"][i], r["payback_raw"], rtol=1e-6, atol=1e-6), i
        else:
            assert o["payback_period"][i] == r["payback_period"], (i, o["payback_raw"][i], r["payback_raw"])
        N1 = int(pop.cols["econ_life"][i]) + 1
        for k_o, k_r in (("cash_flow", "cash_flow"), ("cfev_pv", "cf_energy_value_pv_only"),
                         ("bill_w_pv", "bill_w_pv_only"), ("cfev_batt", "cf_energy_value_pv_batt"),
                         ("bill_w_batt", "bill_w_pv_batt")):
            assert np.allclose(o[k_o][i, :N1], r[k_r], rtol=1e-6, atol=1e-5), (i, k_o)
        for k_o, k_r in (("net_pvonly", "adopter_net_hourly_pvonly"),
                         ("net_with_batt", "adopter_net_hourly_with_batt")):
            ref_h = r[k_r]
            assert np.allclose(o[k_o][i], ref_h, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref_h).max())), (i, k_o)
    assert n_exempt <= n_exempt_max, n_exempt
    return n_switch


@pytest.mark.parametrize("cfg,n,long_life", [
    ("res_1m_nem_tou", 130, False), ("ca_res_storage", 130, False), ("com_8m", 130, False),
    ("national_mixed", 130, False), ("metering_mix", 130, False), ("com_kwkw", 130, False),
    ("national_mixed", 130, True), ("res_1m_nem_tou", 1, False)])
def test_evaluate_matches_oracle(engine, cfg, n, long_life):
    """n = 130: two agents per wave with an odd tail; long_life: a third of
    the lives at 33..50 years, one agent per wave; sizes u x load_kwh / naep
    with u uniform in [0.5, 1.5], so well outside the search's bracket too."""
    pop = _small_pop(cfg, n)
    if long_life:
        life = pop.cols["econ_life"].copy()
        life[::3] = 33 + (np.arange(life[::3].size) % 18)
        pop.cols["econ_life"] = life
    u, kw = _sizes(pop, 20261019 + n)
    batch = _load(engine, pop)
    o = _evaluate(engine, batch, kw)
    assert engine.last_paths()["dc_prebuild"] == 0
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale)
    n_switch = _check_against_oracle(o, kw, pop, opop, n // 100)
    if n > 1:
        assert (u < 0.8).any() and (u > 1.25).any()
        if cfg != "ca_res_storage":
            assert n_switch > 0


@pytest.mark.parametrize("net_billing", [False, True])
def test_evaluate_matches_oracle_with_demand_charges(engine_dc, net_billing):
    """The demand-charge instantiations (extension mode): envelopes built
    inside the evaluation over the size's own generation range."""
    from dgen_amd.columnar import assign_scratch
    pop = make_population("com_dc_batt", 130, seed=20260007, n_res_shapes=16, n_com_shapes=32, n_cf=32,
                          n_counties=16, n_tariffs=24)
    if net_billing:
        t = pop.tariffs.copy()
        t["mo"][1::2] = 2
        pop.tariffs = t
        pop.n_scratch = assign_scratch(pop.cols, pop.tariffs, pop.switches)
    _, kw = _sizes(pop, 77)
    batch = _load(engine_dc, pop, pop.demand)
    o = _evaluate(engine_dc, batch, kw)
    assert engine_dc.last_paths()["dc"] == 1 and engine_dc.last_paths()["dc_prebuild"] == 0
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale,
                                     demand=pop.demand)
    _check_against_oracle(o, kw, pop, opop, 1)


def test_evaluate_at_search_end_repeats_the_search_bits(engine):
    """An agent that never switched, evaluated at its search's last x, repeats
    that search's last evaluation: the bins-only NEM bill does not depend on
    the generation range and the build keeps a * b + c as two roundings, so
    the PV-only outputs are the sizing call's bit for bit."""
    pop = _small_pop("res_1m_nem_tou", 600)
    batch = _load(engine, pop)
    mode = engine.cfg.exact_mode()
    engine.set_exact(0)
    try:
        out = engine.alloc_outputs(batch.n, hourly=False)
        engine.size(batch, out)
        torch.cuda.synchronize()
        s = outputs_to_host(out)
    finally:
        engine.set_exact(mode)
    keep = (s["switched"] == 0) & (s["status"] == 0)
    assert keep.sum() * 2 >= batch.n
    e = _evaluate(engine, batch, np.where(keep, s["x_last"], 1.0), hourly=False)
    for k in ("npv", "payback_raw", "first_with", "first_without", "price_per_kwh", "annual_kwh") + PV_YEARLY:
        assert np.array_equal(e[k][keep], s[k][keep], equal_nan=True), k
    assert np.array_equal(e["tariff_final"][keep], s["tariff_final"][keep])
    assert (e["switched"][keep] == 0).all()


SHARED = (("npv", "npv"), ("payback_raw", "payback_raw"), ("first_with", "first_with"),
          ("first_without", "first_without"), ("tariff", "tariff_final"), ("switched", "switched"),
          ("status", "status"))


@pytest.mark.parametrize("K", [3, 64])
def test_curve_columns_equal_single_evaluations(engine, K):
    """Column k of the curve is a K = 1 evaluation at xs[k], bit for bit: the
    points do not see each other (rate-switch state, records).  Points with
    NaN, 0 and -1 get DGEN_ST_BOUNDS and NaN and leave their neighbours alone."""
    pop = _small_pop("national_mixed", 65)
    batch = _load(engine, pop)
    base = _max_load(pop)
    rel = np.linspace(0.4, 1.7, K)
    rng = np.random.default_rng(5)
    xs = np.stack([rng.permutation(rel)[k % K] * base * rng.uniform(0.9, 1.1, batch.n) for k in range(K)])
    bad = {(1, 3): np.nan, (K - 1, 10): 0.0, (0, 64): -1.0, (2, 33): np.inf}
    for (k, i), v in bad.items():
        xs[k, i] = v
    c = {k: v.cpu().numpy() for k, v in engine.objective_curve(batch, xs).items()}
    assert set(c) == set(_lib.CURVE_FIELDS) and all(v.shape == (K, batch.n) for v in c.values())
    n_sw = 0
    for k in sorted({0, 1, 2, K // 2, K - 1}):
        ok = np.isfinite(xs[k]) & (xs[k] > 0)
        o = _evaluate(engine, batch, np.where(ok, xs[k], 1.0), hourly=False)
        for ck, ok_ in SHARED:
            assert np.array_equal(c[ck][k][ok], o[ok_][ok], equal_nan=True), (k, ck)
        assert np.array_equal(c["total_cost"][k][ok], -o["cash_flow"][ok, 0]), k
        n_sw += int(c["switched"][k][ok].sum())
    assert n_sw > 0
    for (k, i) in bad:
        assert c["status"][k, i] & _lib.ST_BOUNDS
        for f in _lib.CURVE_F64:
            assert np.isnan(c[f][k, i]), (k, i, f)
        assert c["tariff"][k, i] == pop.cols["tariff0"][i] and c["switched"][k, i] == 0
    good = np.ones((K, batch.n), bool)
    for (k, i) in bad:
        good[k, i] = False
    assert (c["status"][good] == 0).all() and np.isfinite(c["npv"][good]).all()


def test_curve_null_members_are_not_written(engine):
    pop = _small_pop("national_mixed", 65)
    batch = _load(engine, pop)
    xs = np.stack([0.7 * _max_load(pop), 1.2 * _max_load(pop)])
    full = engine.objective_curve(batch, xs)
    part = engine.objective_curve(batch, xs, want=("npv", "status"))
    torch.cuda.synchronize()
    assert set(part) == {"npv", "status"}
    assert torch.equal(part["npv"], full["npv"]) and torch.equal(part["status"], full["status"])


def test_evaluate_bounds_status_for_a_bad_size(engine):
    """dgen_eval_agents: a size that is NaN, 0 or negative is k_size_w's
    unsized agent with DGEN_ST_BOUNDS; the other agents are untouched."""
    pop = _small_pop("national_mixed", 65)
    batch = _load(engine, pop)
    kw = 0.9 * _max_load(pop)
    ref = _evaluate(engine, batch, kw, hourly=False)
    kw2 = kw.copy()
    kw2[[2, 31, 64]] = [np.nan, 0.0, -3.0]
    o = _evaluate(engine, batch, kw2, hourly=False)
    bad = np.zeros(batch.n, bool)
    bad[[2, 31, 64]] = True
    assert ((o["status"][bad] & _lib.ST_BOUNDS) != 0).all() and (o["nfev"][bad] == 0).all()
    assert np.isnan(o["npv"][bad]).all() and np.isnan(o["system_kw"][bad]).all()
    for k in ("npv", "system_kw", "status", "nfev", "npv_pv_batt", "cash_flow"):
        assert np.array_equal(o[k][~bad], ref[k][~bad], equal_nan=True), k


def _equal_outputs(a, b):
    for k in a:
        if a[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_evaluate_forms(engine):
    """Two pipeline chunks, the battery run off, the with-battery plane alone
    and the planes taken afterwards (dgen_hourly_planes) against one plain
    evaluation with the three planes."""
    pop = _small_pop("national_mixed", 300)
    batch = _load(engine, pop)
    _, kw = _sizes(pop, 3)
    one = _evaluate(engine, batch, kw)
    engine.kernel_times()                # drain earlier calls
    engine.set_pipeline(2)
    try:
        two = _evaluate(engine, batch, kw)
    finally:
        engine.set_pipeline(_lib.DEFAULT_CHUNKS)
    assert engine.kernel_times()[3] == 1     # one timed call, the evaluation in the k_size slot
    _equal_outputs(one, two)
    assert engine.exact_count() == 0
    # PV-only variant
    engine.set_battery(False)
    try:
        nob = _evaluate(engine, batch, kw)
    finally:
        engine.set_battery(True)
    for k in ("npv", "payback_raw", "system_kw", "annual_kwh", "net_pvonly", "baseline") + PV_YEARLY:
        assert np.array_equal(nob[k], one[k], equal_nan=True), k
    # the with-battery plane alone
    out = engine.alloc_outputs(batch.n, hourly="with_batt")
    engine.evaluate(batch, out, kw)
    torch.cuda.synchronize()
    wb = outputs_to_host(out)
    assert wb["baseline"] is None and wb["net_pvonly"] is None
    assert np.array_equal(wb["net_with_batt"], one["net_with_batt"])
    # (this form's scan sums the battery case's bins in another order, as after
    # a sizing call: the oracle-parity tolerance, not bits)
    assert np.allclose(wb["npv_pv_batt"], one["npv_pv_batt"], rtol=1e-6, atol=1e-6)
    for k in ("npv", "payback_raw", "system_kw") + PV_YEARLY:
        assert np.array_equal(wb[k], one[k], equal_nan=True), k
    # planes after an evaluation without them
    out = engine.alloc_outputs(batch.n, hourly=False)
    engine.evaluate(batch, out, kw)
    planes = engine.alloc_outputs(batch.n, hourly=True)
    for name in _lib.OUTPUT_HOURLY:
        out[name] = planes[name]
    engine.hourly_planes(batch, engine.c_outputs(out))
    torch.cuda.synchronize()
    late = outputs_to_host(out)
    for name in _lib.OUTPUT_HOURLY:
        assert np.array_equal(late[name], one[name]), name


def test_entry_point_argument_errors(engine):
    pop = _small_pop("res_1m_nem_tou", 40)
    batch = _load(engine, pop)
    out = engine.alloc_outputs(batch.n, hourly=False)
    co = engine.c_outputs(out)
    kw = engine._to_dev(0.9 * _max_load(pop), torch.float64)
    L, T, A = engine.lib, ctypes.byref(engine.tables), ctypes.byref(batch.c_agents)
    ws, wsb, st = batch.workspace.data_ptr(), batch.workspace.numel(), engine.stream_handle()
    E_ARG = -1
    assert L.dgen_eval_agents(engine.ctx, T, A, ctypes.byref(co), None, batch.n, ws, wsb, batch.n_scratch, st) == E_ARG
    assert L.dgen_eval_agents(engine.ctx, T, A, ctypes.byref(co), kw.data_ptr(), batch.n, ws, wsb - 8,
                              batch.n_scratch, st) == E_ARG
    npv = torch.full((2, batch.n), 7.0, dtype=torch.float64, device=engine.dev)
    cv = _lib.CurveOut(npv=npv.data_ptr())
    xs = torch.stack([kw, kw]).contiguous()
    call = lambda xp, K, outp, nbytes: L.dgen_objective_curve(engine.ctx, T, A, xp, K, batch.n, outp, ws, nbytes,
                                                               batch.n_scratch, st)
    assert call(None, 2, ctypes.byref(cv), wsb) == E_ARG
    assert call(xs.data_ptr(), 2, None, wsb) == E_ARG
    assert call(xs.data_ptr(), 0, ctypes.byref(cv), wsb) == E_ARG
    assert call(xs.data_ptr(), 65, ctypes.byref(cv), wsb) == E_ARG
    assert call(xs.data_ptr(), 2, ctypes.byref(cv), wsb - 8) == E_ARG
    torch.cuda.synchronize()
    assert (npv == 7.0).all()            # nothing was launched
    assert call(xs.data_ptr(), 2, ctypes.byref(cv), wsb) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(npv).all() and not (npv == 7.0).any()
    engine.evaluate(batch, out, kw)
    assert engine.exact_count() == 0


def test_npv_curve_returns_caller_order(engine):
    from dgen_amd import sensitivity
    from dgen_amd.engine import profile_order
    pop = _small_pop("national_mixed", 65)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    plain = engine.upload_agents(pop.cols, pop.n_scratch)
    a = sensitivity.npv_curve(engine, plain, rel=(0.5, 1.0, 1.5))
    ordered = engine.upload_agents(pop.cols, pop.n_scratch, order=profile_order(pop.cols))
    b = sensitivity.npv_curve(engine, ordered, rel=(0.5, 1.0, 1.5))
    assert np.array_equal(a["kw"][1], _max_load(pop)) and a["npv"].shape == (3, 65)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    c = sensitivity.npv_curve(engine, ordered, rel=(1.0,), base=1.5 * _max_load(pop))
    assert np.array_equal(c["npv"][0], a["npv"][2])


def test_size_frame_fixed_kw(monkeypatch):
    """size_frame(fixed_kw=...) is Engine.evaluate on the frame's rows: the
    column form, the array form and a sub-batched call agree bit for bit, and
    the sizes come back as system_kw; a NaN entry raises before any launch."""
    from dgen_amd import financial_functions as ff
    from dgen_amd.columnar import columnize_frame
    from dgen_amd.engine import profile_order
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(200)
    b = columnize_frame(df, store, table)
    cols = b.frame_columns
    naep = (store.cfs.astype(np.float64) / 1e6).sum(axis=1)
    kw = np.random.default_rng(9).uniform(0.5, 1.5, len(df)) * cols["load_kwh"] / naep[cols["cf_row"]]
    df = df.assign(system_kw_given=kw)
    f1, o1 = ff.size_frame(df, store, table, hourly="array", fixed_kw="system_kw_given")
    assert np.array_equal(f1["system_kw"].to_numpy(), kw) and (o1["nfev"] == 1).all()
    f2, o2 = ff.size_frame(df, store, table, hourly="array", fixed_kw=kw, max_rows=64)
    f3, o3 = ff.size_frame(df, store, table, hourly="array")
    assert (o3["system_kw"] != kw).all()     # without fixed_kw the frame is sized
    # Engine.evaluate on the same rows
    eng = ff.get_engine()
    batch = eng.upload_agents(cols, order=profile_order(cols))
    out = eng.alloc_outputs(batch.n, hourly=True, hourly_f64=True)
    eng.evaluate(batch, out, kw[batch.perm])
    torch.cuda.synchronize()
    ref = outputs_to_host(out, batch.perm)
    for name, _ in _lib.OUTPUT_SCALARS:
        assert np.array_equal(o1[name], ref[name], equal_nan=True), name
        assert np.array_equal(o2[name], ref[name], equal_nan=True), name
    for name in _lib.OUTPUT_YEARLY:
        assert np.array_equal(o1[name], ref[name], equal_nan=True), name
        assert np.array_equal(o2[name], ref[name], equal_nan=True), name
    for col, name in (("baseline_net_hourly", "baseline"), ("adopter_net_hourly_pvonly", "net_pvonly"),
                      ("adopter_net_hourly_with_batt", "net_with_batt")):
        assert np.array_equal(np.stack(list(f1[col])), ref[name]), col
        assert np.array_equal(np.stack(list(f2[col])), ref[name]), col
    for c in ("npv", "payback_period", "batt_kwh"):
        assert np.array_equal(f1[c].to_numpy(), f2[c].to_numpy()), c
    # a NaN size: ValueError naming the agent, nothing launched
    calls = []
    monkeypatch.setattr(type(eng), "evaluate", lambda *a, **k: calls.append(1))
    monkeypatch.setattr(type(eng), "size", lambda *a, **k: calls.append(1))
    kw_bad = kw.copy()
    kw_bad[17] = np.nan
    ids = df["agent_id"].tolist() if "agent_id" in df else list(df.index)
    with pytest.raises(ValueError, match=f"agent {ids[17]}"):
        ff.size_frame(df, store, table, fixed_kw=kw_bad)
    assert not calls
