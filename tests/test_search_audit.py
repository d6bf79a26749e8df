"""Host side of the search audit (dgen_amd.search_audit), no GPU: the Python
restatement of the bounded Brent fed the oracle's own objective values takes
the oracle's path bit for bit, and the host restatement of the certificate's
error model is finite and positive where every bound table is present."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from dgen_amd import _lib, search_audit
from tests import search_audit_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg,n,long_life", cases.POPULATIONS, ids=cases.IDS)
def test_replay_x_takes_the_oracle_path_bit_for_bit(cfg, n, long_life):
    """replay_x over the f column of the oracle's brent_trace: the oracle's
    x's, nfev and system_kw, bit for bit, for every agent."""
    pop, traces, results = cases.oracle_case(cfg, n, long_life)
    br = cases.brackets(pop)
    nfevs = []
    for i in range(n):
        r, t = results[i], traces[i]
        assert r["status"] == 0, i
        assert len(t) == r["nfev"] and 1 <= r["nfev"] <= search_audit.TRACE_MAX, (i, r["nfev"])   # none truncated
        xs, nfev, xf = search_audit.replay_x(t[:, 1], *br[i])
        assert nfev == r["nfev"], (i, nfev, r["nfev"])
        assert np.array_equal(np.asarray(xs), t[:, 0]), (i, xs, t[:, 0])
        assert xf == r["system_kw"] and xs[-1] == r["x_last"], (i, xf, r["system_kw"])
        nfevs.append(nfev)
    print(f"\n{cfg} n={n}: oracle nfev {min(nfevs)}..{max(nfevs)}, switched "
          f"{sum(int(r['switched']) for r in results)}", flush=True)
    assert max(nfevs) >= 3
    if cfg != "com_dc_batt":
        assert any(int(r["switched"]) for r in results)


def test_replay_x_truncates_a_search_that_does_not_end():
    """32 values that keep the search going: nfev 33, 32 x's, no result; the
    same list cut short stops where it ends."""
    # a bracket 1e12 wide shrinks by golden-section steps at best: > 50 evaluations to reach xatol
    lo, hi, xatol = 1.0, 1e12, 2.0
    f = [-float(k) for k in range(search_audit.TRACE_MAX)]       # every point better than the last
    xs, nfev, xf = search_audit.replay_x(f, lo, hi, xatol)
    assert nfev == search_audit.TRACE_MAX + 1 and len(xs) == search_audit.TRACE_MAX and math.isnan(xf)
    assert all(lo < x < hi for x in xs) and len(set(xs)) == len(xs)
    xs5, nfev5, xf5 = search_audit.replay_x(f[:5], lo, hi, xatol)
    assert nfev5 == 6 and xs5 == xs[:5] and math.isnan(xf5)
    # a bracket within xatol ends at the first evaluation
    xs1, nfev1, xf1 = search_audit.replay_x([3.0], 10.0, 10.5, 2.0)
    assert nfev1 == 1 and xf1 == xs1[0] == 10.0 + 0.3819660112501051 * 0.5


def test_bracket_of_is_the_reference_bracket():
    from tests import helpers
    for kwh, naep in ((9500.0, 1432.7), (250000.0, 1100.0), (3.0, 1900.0), (4.0e7, 1250.5)):
        lo, hi, xatol = search_audit.bracket_of(kwh, naep)
        assert lo == (kwh / naep) * 0.8 and hi == (kwh / naep) * 1.25
        assert xatol == helpers.xatol_of(kwh, naep)


@pytest.mark.parametrize("cfg,n,long_life", cases.POPULATIONS, ids=cases.IDS)
def test_model_of_is_finite_and_positive(cfg, n, long_life):
    pop = cases.population(cfg, n, long_life)
    skip = pop.skip_demand_charges
    tb = search_audit.bound_tables(pop.shapes, pop.cfs, pop.wholesale, pop.tariffs, None if skip else pop.demand)
    M = search_audit.model_of(pop.cols, pop.switches, tb, skip_demand_charges=skip)
    assert M.shape == (n, 4) and np.isfinite(M).all() and (M > 0.0).all()
    assert (M[:, 2] == 512.0 * 2.220446049250313e-16).all()
    assert (M[:, 3] > 1.0).all()                                 # the Lipschitz bound is dollars per kW


def test_model_of_is_not_finite_without_a_bound_table():
    # TS sell-rate agents (net billing, not CA, a wholesale row) need bt_ts_max
    pop = cases.population("metering_mix", 64, False)
    tb = search_audit.bound_tables(pop.shapes, pop.cfs, pop.wholesale, pop.tariffs)
    full = search_audit.model_of(pop.cols, pop.switches, tb)
    M = search_audit.model_of(pop.cols, pop.switches, {**tb, "bt_ts_max": None})
    lost = ~np.isfinite(M).all(axis=1)
    assert lost.any() and not lost.all()
    assert np.array_equal(M[~lost], full[~lost])
    # billed demand charges need the profile maxima and the tariffs' price bounds
    pop = cases.population("com_dc_batt", 48, False)
    tb = search_audit.bound_tables(pop.shapes, pop.cfs, pop.wholesale, pop.tariffs, pop.demand)
    for missing in ("bt_shape_max", "bt_cf_max", "bt_tariff"):
        M = search_audit.model_of(pop.cols, pop.switches, {**tb, missing: None}, skip_demand_charges=0)
        assert not np.isfinite(M).all(axis=1).any(), missing
    # ... and none of them with the demand charges skipped
    M = search_audit.model_of(pop.cols, pop.switches, {**tb, "bt_shape_max": None, "bt_cf_max": None, "bt_tariff": None},
                              skip_demand_charges=1)
    assert np.isfinite(M).all()
    # a switch row outside the tariff table
    pop = cases.population("de_res", 48, False)
    tb = search_audit.bound_tables(pop.shapes, pop.cfs, pop.wholesale, pop.tariffs)
    sw = pop.switches.copy()
    i = int(np.flatnonzero(pop.cols["sw_solar_cnt"] > 0)[0])
    sw["tariff"][pop.cols["sw_solar_off"][i]] = len(pop.tariffs)
    M = search_audit.model_of(pop.cols, sw, tb)
    assert not np.isfinite(M[i]).all()


def test_compare_applies_the_rule():
    nan = math.nan
    row = lambda v: np.array(list(v) + [nan] * (search_audit.TRACE_MAX - len(v)))
    trace = {"x": np.stack([row([10.0, 20.0, 30.0]), row([10.0, 20.0, 30.0]), row([])]),
             "f": np.stack([row([-1.0, -2.0, -3.0]), row([-1.0, -2.0, -3.0]), row([])]),
             "f_bound": np.stack([row([0.5, 0.5, 0.5]), row([0.5, 0.5]), row([])]),
             "x_bound": np.stack([row([0.0, 1.0, 1.0]), row([0.0, 1.0]), row([])]),
             "nfev": np.array([3, 3, 0])}
    ref = [np.array([[10.0, -1.25], [20.5, -2.0], [30.0, -4.0]]),      # third evaluation beyond its bound
           np.array([[10.0, -1.0], [22.0, -2.1], [30.0, -9.0]]),       # x leaves its bound at k = 1: k = 2 not compared
           None]
    c = search_audit.compare(trace, ref)
    assert c["compared"].tolist() == [3, 2, 0]
    assert c["f_violations"].tolist() == [1, 0, 0] and c["x_violations"].tolist() == [0, 1, 0]
    assert c["ratio_f"][0] == 2.0 and c["ratio_x"][0] == 0.5 and c["ratio_x"][1] == 2.0
    assert math.isnan(c["ratio_f"][2]) and c["x0_equal"].tolist() == [True, True, False]
    assert c["worst_f"] == 2.0 and c["worst_x"] == 2.0 and c["agents"] == 2 and c["deep"] == 1


def test_abi_surface():
    assert "dgen_search_trace" in _lib.EXPORTED
    L = _lib.load()
    assert L.dgen_search_trace.restype is ctypes.c_int32 and len(L.dgen_search_trace.argtypes) == 7
    text = open(os.path.join(REPO, "include", "dgen_hip.h")).read()
    m = re.search(r"#define DGEN_TRACE_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.TRACE_MAX == search_audit.TRACE_MAX
    body = re.search(r"typedef struct \{([^}]*)\} dgen_search_trace_out;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*(\w+)", body) == _lib.TRACE_FIELDS
    assert ctypes.sizeof(_lib.SearchTraceOut) == 8 * len(_lib.TRACE_FIELDS)
    src = open(os.path.join(REPO, "dgen_amd", "csrc", "dgen_hip.hip")).read()
    assert float(re.search(r"constexpr double BT_GAMMA = ([\d.]+);", src).group(1)) == search_audit.BT_GAMMA
    # one construction of the model, called by the certificate and by the audit
    assert len(re.findall(r"M\.c0 = g \*", src)) == 1 and len(re.findall(r"= bt_search_of\(", src)) == 2
