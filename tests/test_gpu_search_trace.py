"""Search trace and certificate audit of the sizing call (dgen_search_trace,
Engine.search_trace, dgen_amd.search_audit) on the device.

The certificate (k_brent_certify) claims, per evaluation of a search it follows,
|f_device - f_oracle| <= f_bound and |x_device - x_oracle| <= x_bound.  The
first test holds it to that against the oracle's own traced search, with no
tolerance: the inequalities are the certificate's claim.  Worst observed / bound
per population as measured on an MI355X (objective f, evaluation point x; the
test prints them, DESIGN.md section 2 has the table): de_res 6.6e-4 / 0,
res_1m_nem_tou 6.1e-4 / 0, ca_res_storage 4.8e-4 / 0, com_8m 8.2e-4 / 1.2e-4,
com_kwkw 5.5e-4 / 8.6e-5, com_dc_batt (demand charges billed) 4.1e-4 / 1.2e-4,
metering_mix 5.2e-4 / 5.6e-5, national_mixed (long lives) 8.4e-4 / 5.3e-5: the
bound holds on all eight, with three orders of magnitude to spare."""
import ctypes

import numpy as np
import pytest
import torch

from dgen_amd import _lib, search_audit
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig
from dgen_amd.engine import Engine, outputs_to_host
from dgen_amd.synth import subset
from tests import search_audit_cases as cases

pytestmark = pytest.mark.gpu

K = _lib.TRACE_MAX
ROWS = ("x", "f", "f_bound", "x_bound")


@pytest.fixture(scope="module")
def engines():
    e = {1: Engine(0, EngineConfig(exact_brent=1)), 0: Engine(0, EngineConfig(skip_demand_charges=0, exact_brent=1))}
    yield e
    for v in e.values():
        v.close()


def _load(eng, pop):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs, pop.demand if not pop.skip_demand_charges else None)
    eng.set_switches(pop.switches)
    eng.set_battery(False)            # only the search matters


def _trace(eng, pop, want=None):
    """Size pop (tables loaded) and lay its search open: (host outputs, host
    trace, agents re-run)."""
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    t = eng.search_trace(batch, out, want)
    torch.cuda.synchronize()
    return outputs_to_host(out), {k: v.cpu().numpy() for k, v in t.items()}, eng.exact_count()


_SIZED = {}


def _sized(engines, cfg, n, long_life):
    """One sizing call and trace per population, shared by the tests."""
    key = (cfg, n, long_life)
    if key not in _SIZED:
        pop = cases.population(cfg, n, long_life)
        eng = engines[pop.skip_demand_charges]
        eng.set_exact(1)
        _load(eng, pop)
        _SIZED[key] = (pop, eng) + _trace(eng, pop) + (eng.profile_sums(),)
    return _SIZED[key]


@pytest.mark.parametrize("cfg,n,long_life", cases.POPULATIONS, ids=cases.IDS)
def test_the_bound_holds_against_the_oracle(engines, cfg, n, long_life):
    pop, _, o, t, _, _ = _sized(engines, cfg, n, long_life)
    _, traces, results = cases.oracle_case(cfg, n, long_life)
    c = search_audit.compare(t, traces)
    cert = t["certified"]
    print(f"\n{cfg} n={n}: worst observed / bound  f {c['worst_f']:.3g}  x {c['worst_x']:.3g}; "
          f"certified {int((cert == 1).sum())}, not settled {int((cert == 0).sum())}, "
          f"agents with >= 3 evaluations compared {c['deep']}, evaluations compared {int(c['compared'].sum())}",
          flush=True)
    assert (cert >= 0).all() and (o["status"] == 0).all()                 # every agent searched
    assert c["x0_equal"].all(), np.flatnonzero(~c["x0_equal"])
    assert (c["compared"] >= 1).all()                                     # evaluation 0 always compares
    bad = np.flatnonzero(c["f_violations"] > 0)
    assert bad.size == 0, (bad, c["ratio_f"][bad])
    sure = cert == 1
    assert sure.any()
    assert c["nfev_equal"][sure].all(), np.flatnonzero(sure & ~c["nfev_equal"])
    assert (c["compared"][sure] == t["nfev"][sure]).all()
    assert (c["x_violations"][sure] == 0).all(), c["ratio_x"][sure & (c["x_violations"] > 0)]
    assert c["deep"] >= 1


@pytest.mark.parametrize("cfg,n,long_life", cases.POPULATIONS, ids=cases.IDS)
def test_the_trace_is_the_search(engines, cfg, n, long_life):
    pop, eng, o, t, _, (_, naep) = _sized(engines, cfg, n, long_life)
    for i in range(n):
        nf = int(t["nfev"][i])
        assert 1 <= nf <= K, (i, nf)
        lo, hi, xatol = search_audit.bracket_of(pop.cols["load_kwh"][i], naep[pop.cols["cf_row"][i]])
        xs, nfev, xf = search_audit.replay_x(t["f"][i, :nf], lo, hi, xatol)
        assert nfev == nf and np.array_equal(np.asarray(xs), t["x"][i, :nf]) and xf == t["system_kw"][i], i
        # rows beyond nfev are NaN, rows within are the search's values
        for k in ("x", "f"):
            assert np.isfinite(t[k][i, :nf]).all() and np.isnan(t[k][i, nf:]).all(), (i, k)
        if t["certified"][i] == 1:
            # the fast search's path stands: the outputs are its values
            assert nf == o["nfev"][i] and t["undecided_at"][i] == -1, i
            assert t["x"][i, nf - 1] == o["x_last"][i] and t["system_kw"][i] == o["system_kw"][i], i
            assert np.isfinite(t["f_bound"][i, :nf]).all() and np.isnan(t["f_bound"][i, nf:]).all(), i
            assert (t["x_bound"][i, :nf] >= 0.0).all() and t["x_bound"][i, 0] == 0.0, i
        else:
            u = int(t["undecided_at"][i])
            assert t["certified"][i] == 0 and 0 <= u <= nf, (i, u)
            for k in ("f_bound", "x_bound"):
                assert np.isfinite(t[k][i, :u]).all() and np.isnan(t[k][i, u:]).all(), (i, k)


@pytest.mark.parametrize("cfg,n,long_life", cases.POPULATIONS, ids=cases.IDS)
def test_consistent_with_the_rerun_and_the_host_model(engines, cfg, n, long_life):
    pop, eng, o, t, k1, (s_sum, naep) = _sized(engines, cfg, n, long_life)
    assert int((t["certified"] == 0).sum()) == k1
    skip = pop.skip_demand_charges
    tb = search_audit.bound_tables(pop.shapes, pop.cfs, pop.wholesale, pop.tariffs, None if skip else pop.demand)
    assert np.allclose(tb["cf_naep"], naep, rtol=1e-14) and np.allclose(tb["shape_sum"], s_sum, rtol=1e-14)
    tb.update(cf_naep=naep, shape_sum=s_sum)          # the engine's own row sums
    M = search_audit.model_of(pop.cols, pop.switches, tb, skip_demand_charges=skip,
                              nm_yearend_sell_rate=eng.cfg.nm_yearend_sell_rate)
    assert np.isfinite(t["model"]).all()
    assert np.allclose(t["model"], M, rtol=1e-12, atol=0.0)
    if cfg in ("national_mixed", "com_dc_batt"):
        # mode 2 re-runs every agent; the certificate's decision is the same array
        eng.set_exact(2)
        try:
            _load(eng, pop)
            o2, t2, k2 = _trace(eng, pop)
        finally:
            eng.set_exact(1)
        assert k2 == n
        for k in t:
            assert np.array_equal(t2[k], t[k], equal_nan=True), k


def test_layout_and_edges(engines):
    eng = engines[1]
    eng.set_exact(1)
    pop = cases._small("national_mixed", 257, long_life=True)
    _load(eng, pop)
    o, t, k1 = _trace(eng, pop)
    assert int((t["certified"] == 0).sum()) == k1 and (t["certified"] >= 0).all()
    # pipeline depth 3: the bits of depth 1
    eng.set_pipeline(3)
    try:
        _, t3, _ = _trace(eng, pop)
    finally:
        eng.set_pipeline(1)
    for k in t:
        assert np.array_equal(t3[k], t[k], equal_nan=True), k
    # an agent's rows in the batch are its rows sized in a smaller batch, and alone
    for idx in (np.arange(65), np.array([0]), np.array([64]), np.array([256]), np.array([131])):
        _, ts, _ = _trace(eng, subset(pop, idx))
        for k in t:
            assert np.array_equal(ts[k], t[k][idx], equal_nan=True), (k, idx[:3])
    # a load that is not finite: no search, and the neighbours' bits stand
    cols = {k: v.copy() for k, v in pop.cols.items()}
    bad = np.array([3, 64, 200])
    cols["load_kwh"][bad] = (np.nan, np.inf, np.nan)
    ob, tbad, _ = _trace(eng, type(pop)(**{**pop.__dict__, "cols": cols}))
    assert (ob["status"][bad] & _lib.ST_BOUNDS).all() and (ob["nfev"][bad] == 0).all()
    assert (tbad["certified"][bad] == -1).all() and (tbad["nfev"][bad] == 0).all()
    assert (tbad["undecided_at"][bad] == -1).all() and np.isnan(tbad["system_kw"][bad]).all()
    for k in ROWS + ("model",):
        assert np.isnan(tbad[k][bad]).all(), k
    rest = np.setdiff1d(np.arange(257), bad)
    for k in t:
        assert np.array_equal(tbad[k][rest], t[k][rest], equal_nan=True), k
    # NULL members are not written: sentinel buffers stay as they are
    batch = eng.upload_agents(pop.cols, pop.n_scratch)
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    buf = {k: torch.full((257, K) if k in ROWS else ((257, 4) if k == "model" else (257,)), -7,
                         dtype=torch.float64 if k in _lib.TRACE_F64 else torch.int32, device=eng.dev)
           for k in _lib.TRACE_FIELDS}
    asked = ("x", "certified")
    to = _lib.SearchTraceOut(**{k: buf[k].data_ptr() for k in asked})
    co = eng.c_outputs(out)
    rc = eng.lib.dgen_search_trace(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), ctypes.byref(co),
                                   batch.n, ctypes.byref(to), eng.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    for k in _lib.TRACE_FIELDS:
        got = buf[k].cpu().numpy()
        if k in asked:
            assert np.array_equal(got, t[k], equal_nan=True), k
        else:
            assert (got == -7).all(), k
    # want: only the members asked for come back
    only = eng.search_trace(batch, out, ("nfev",))
    assert list(only) == ["nfev"] and np.array_equal(only["nfev"].cpu().numpy(), t["nfev"])
    with pytest.raises(ValueError):
        eng.search_trace(batch, out, ("nfev", "npv"))


def test_errors(engines):
    pop = cases.population("de_res", 48, False)
    eng = Engine(0, EngineConfig(exact_brent=1))
    try:
        _load(eng, pop)
        batch = eng.upload_agents(pop.cols, pop.n_scratch)
        out = eng.alloc_outputs(batch.n, hourly=False)

        def refused():
            with pytest.raises(_lib.DgenError) as e:
                eng.search_trace(batch, out)
            assert "(-1)" in str(e.value) and "dgen_search_trace" in str(e.value)      # DGEN_E_ARG

        refused()                                          # no sizing call yet
        eng.size(batch, out)
        assert eng.search_trace(batch, out)["nfev"].shape == (48,)
        co, to = eng.c_outputs(out), _lib.SearchTraceOut()
        args = (eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), ctypes.byref(co))
        assert eng.lib.dgen_search_trace(*args, 47, ctypes.byref(to), eng.stream_handle()) == -1      # a wrong n
        assert "47" in _lib.last_error()
        assert eng.lib.dgen_search_trace(*args, 48, None, eng.stream_handle()) == -1                   # out NULL
        assert eng.lib.dgen_search_trace(*args, 48, ctypes.byref(to), eng.stream_handle()) == 0       # nothing asked
        kw = out["system_kw"].clone()
        eng.evaluate(batch, out, kw)                       # an evaluation records no trace
        refused()
        eng.set_exact(0)                                   # nor does mode 0
        eng.size(batch, out)
        refused()
        eng.set_exact(2)
        eng.size(batch, out)
        torch.cuda.synchronize()
        assert (eng.search_trace(batch, out, ("certified",))["certified"] >= 0).all()
    finally:
        eng.close()


def test_drop_in_switch(engine):
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(100)
    ff._worker_conn = store
    on, agg = ff.size_chunk(df, None, table, "simple", hourly="none", search_audit=True)
    off, agg_off = ff.size_chunk(df, None, table, "simple", hourly="none")
    assert list(on.columns)[-4:] == list(search_audit.COLUMNS)
    assert list(on.columns)[:-4] == list(off.columns)
    assert not any(c in off.columns for c in search_audit.COLUMNS)
    for c in off.columns:
        a, b = on[c], off[c]
        if a.dtype.kind in "fiub":
            assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True), c
    assert agg["net_sum_kw"] == agg_off["net_sum_kw"]
    assert on["search_nfev_fast"].dtype == np.int64 and on["search_certified"].dtype == np.int64
    assert on["search_rerun"].dtype == bool and on["search_bound_usd"].dtype == np.float64
    cert = on["search_certified"].to_numpy()
    assert np.isin(cert, (0, 1)).all() and (cert == 1).any()
    assert np.array_equal(on["search_rerun"].to_numpy(), cert == 0)
    sure = cert == 1
    assert (on["search_nfev_fast"].to_numpy() >= 1).all() and (on["search_nfev_fast"].to_numpy() <= K).all()
    b = on["search_bound_usd"].to_numpy()
    assert np.isfinite(b[sure]).all() and (b[sure] > 0.0).all()
    # sub-batches: the bits of one call, in frame order
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", search_audit=True, max_rows=40)
    for c in search_audit.COLUMNS:
        assert np.array_equal(sub[c].to_numpy(), on[c].to_numpy(), equal_nan=True), c
    # frame order: the engine call's rows gathered through the batch's permutation
    from dgen_amd.columnar import columnize_frame
    from dgen_amd.engine import profile_order
    eng = ff.get_engine()
    cols = columnize_frame(df, store, table).frame_columns
    batch = eng.upload_agents(cols, order=profile_order(cols))
    out = eng.alloc_outputs(batch.n, hourly=False)
    eng.size(batch, out)
    t = eng.search_trace(batch, out, ("nfev", "certified"))
    inv = np.empty(batch.n, np.int64)
    inv[batch.perm] = np.arange(batch.n)
    assert np.array_equal(t["nfev"].cpu().numpy()[inv], on["search_nfev_fast"].to_numpy())
    assert np.array_equal(t["certified"].cpu().numpy()[inv], cert)
    assert batch.perm is not None and not np.array_equal(batch.perm, np.arange(batch.n))
    with pytest.raises(ValueError):
        ff.size_chunk(df, None, table, "simple", hourly="none", search_audit=True, fixed_kw=on["system_kw"].to_numpy())
