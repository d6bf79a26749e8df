"""The demand-charge and kWh/kW fill-in of the PV search on the with-battery
objective, host side: the binding and its option struct against the header,
the drop-in switch's further spec keys, Engine.size_with_batt's keywords, and
a numpy restatement of the entry's candidate rule (candidates_peak, which the
GPU test compares the written set against)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from dgen_amd.engine import SWITCH_DTYPE
from dgen_amd.synth import make_population
from dgen_amd.tariff import attach_peak_records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dgen_hip.h")
LIB = os.path.join(REPO, "dgen_amd", "lib", "libdgen_hip.so")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
int main(void) {
  printf("size %zu\n", sizeof(dgen_swb_peak_opt));
  printf("cap_mixed %zu\n", offsetof(dgen_swb_peak_opt, cap_mixed));
  printf("cap_kept %zu\n", offsetof(dgen_swb_peak_opt, cap_kept));
  printf("max_blocks %zu\n", offsetof(dgen_swb_peak_opt, max_blocks));
  printf("pad %zu\n", offsetof(dgen_swb_peak_opt, pad));
  printf("capm %d\n", DGEN_NB_CAPM);
  printf("capk %d\n", DGEN_BATT_PEAK_CAPK);
  printf("capk_max %d\n", DGEN_BATT_PEAK_CAPK_MAX);
  printf("abi %d\n", DGEN_ABI_VERSION);
  return 0;
}
"""


def candidates_peak(eng_tables, pop, lo, hi, dc_on):
    """dgen_size_with_batt_peak's candidate rule from the rows alone.  eng_tables: the tariff records as
    the engine holds them (Engine.tariff_records: tariff.attach_peak_records applied); dc_on: the engine
    bills demand charges (cfg.skip_demand_charges == 0).  A valid bracket, a life in 1 .. MAXY, tariff0
    inside the table without ST_UNIT, and tariff0 or an in-range storage row's tariff of peak form: kWh/kW
    tier units (1, 3), or -- with dc_on -- a demand record behind it."""
    c, t = pop.cols, eng_tables
    t0 = c["tariff0"]
    inr = (t0 >= 0) & (t0 < t.size)
    t0s = np.where(inr, t0, 0)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lo) & np.isfinite(hi) & (lo > 0.0) & (lo < hi)
    ok &= (c["econ_life"] >= 1) & (c["econ_life"] <= _lib.MAXY) & inr & ((t["flags"][t0s] & _lib.ST_UNIT) == 0)
    form = np.isin(t["unit"], (1, 3)) | (bool(dc_on) & (t["dc"] > 0))
    peak = form[t0s] & inr
    for i in np.nonzero(c["sw_storage_cnt"] > 0)[0]:
        off = int(c["sw_storage_off"][i])
        for r in pop.switches[off:off + int(c["sw_storage_cnt"][i])]:
            tt = int(r["tariff"])
            peak[i] |= 0 <= tt < t.size and bool(form[tt])
    return ok & peak


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


def _records(pop, dc_on):
    recs, _, _ = attach_peak_records(np.ascontiguousarray(pop.tariffs), pop.demand if dc_on else None)
    return recs


def _row(pop, i, tariff, lo_kw=0.0, hi_kw=1e9):
    """Agent i gets one storage row of its own onto `tariff`."""
    rec = np.zeros((), dtype=SWITCH_DTYPE)
    rec["min_kw"], rec["max_kw"], rec["tariff"], rec["one_time_charge"] = lo_kw, hi_kw, tariff, 5.0
    rows = [r for r in pop.switches] + [rec]
    pop.cols["sw_storage_off"] = pop.cols["sw_storage_off"].copy()
    pop.cols["sw_storage_cnt"] = pop.cols["sw_storage_cnt"].copy()
    pop.cols["sw_storage_off"][i], pop.cols["sw_storage_cnt"][i] = len(rows) - 1, 1
    pop.switches = np.stack(rows).astype(SWITCH_DTYPE)


def test_the_binding_is_declared():
    text = open(HEADER).read()
    assert re.search(r"^int32_t\s+dgen_size_with_batt_peak\s*\(", text, flags=re.M)
    assert re.search(r"typedef struct \{ int32_t cap_mixed; int32_t cap_kept; int32_t max_blocks; int32_t pad; \} "
                     r"dgen_swb_peak_opt;", text)
    assert "dgen_size_with_batt_peak" in _lib.EXPORTED
    assert re.search(r"#define\s+DGEN_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14
    if not os.path.exists(LIB):
        pytest.skip("libdgen_hip.so is not built: the symbol is not resolved")
    L = _lib.load(build_if_missing=False)
    fn = L.dgen_size_with_batt_peak
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 10
    assert len(L.dgen_size_with_batt.argtypes) == 9 and len(L.dgen_size_with_batt_net.argtypes) == 10
    assert L.dgen_abi_version() == 14


def test_option_struct_matches_the_header(tmp_path):
    assert [f[0] for f in _lib.SwbPeakOpt._fields_] == ["cap_mixed", "cap_kept", "max_blocks", "pad"]
    assert ctypes.sizeof(_lib.SwbPeakOpt) == 16
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert lay["size"] == 16
    for j, name in enumerate(("cap_mixed", "cap_kept", "max_blocks", "pad")):
        assert lay[name] == getattr(_lib.SwbPeakOpt, name).offset == 4 * j, name
    assert lay["capm"] == _lib.NB_CAPM and lay["capk"] == _lib.BATT_PEAK_CAPK
    assert lay["capk_max"] == _lib.BATT_PEAK_CAPK_MAX and lay["abi"] == 14


def test_spec_keys():
    # the pair is what it was, whatever the peak keys say; co_size_spec admits them on request only
    assert bs.co_size_spec({"peak_billing": True}, peak=True) == (0.8, 2.0)
    assert bs.co_size_spec({"ratio": 0.4, "hours": 4.0, "peak_billing": True, "peak_caps": (8, 100),
                            "peak_blocks": 2}, peak=True) == (0.4, 4.0)
    assert bs.co_size_spec({"ratio": 0.4, "net_billing": True}, peak=True) == (0.4, 2.0)
    for key in bs.PEAK_KEYS:
        with pytest.raises(ValueError, match="unknown keys"):
            bs.co_size_spec({key: None})
    # without peak billing the engine sees the calls it saw
    for spec in (True, {}, {"peak_billing": False}, {"peak_billing": False, "peak_caps": (4, 4), "peak_blocks": 1}):
        assert bs.co_size_options(spec) == {}, spec
    assert bs.co_size_options({"net_billing": True, "peak_billing": False}) == {"net": True}
    # peak implies nothing about net
    assert bs.co_size_options({"peak_billing": True}) == {"peak": True}
    assert bs.co_size_options({"peak_billing": True, "peak_caps": None, "peak_blocks": None}) == {"peak": True}
    assert bs.co_size_options({"net_billing": True, "net_cap": 7, "peak_billing": True}) == \
        {"net": True, "net_cap": 7, "peak": True}
    assert bs.co_size_options({"peak_billing": True, "peak_caps": (1, 1)}) == {"peak": True, "peak_caps": (1, 1)}
    assert bs.co_size_options({"peak_billing": True, "peak_caps": [_lib.NB_CAPM, _lib.BATT_PEAK_CAPK_MAX],
                               "peak_blocks": 3}) == \
        {"peak": True, "peak_caps": (_lib.NB_CAPM, _lib.BATT_PEAK_CAPK_MAX), "peak_blocks": 3}
    assert bs.co_size_options({"peak_billing": True, "peak_caps": (None, 100)}) == \
        {"peak": True, "peak_caps": (None, 100)}
    for bad in ({"peak_billing": 1}, {"peak_billing": "yes"}, {"peak_billing": None},
                {"peak_billing": True, "peak_caps": (0, 1)}, {"peak_billing": True, "peak_caps": (1, 0)},
                {"peak_billing": True, "peak_caps": (_lib.NB_CAPM + 1, 1)},
                {"peak_billing": True, "peak_caps": (1, _lib.BATT_PEAK_CAPK_MAX + 1)},
                {"peak_billing": True, "peak_caps": (8.0, 8)}, {"peak_billing": True, "peak_caps": (True, 8)},
                {"peak_billing": True, "peak_caps": 8}, {"peak_billing": True, "peak_caps": (8,)},
                {"peak_billing": True, "peak_caps": (8, 8, 8)}, {"peak_billing": True, "peak_blocks": 0},
                {"peak_billing": True, "peak_blocks": "2"}, {"peak_billing": True, "peak_blocks": True},
                {"peak_billing": False, "peak_caps": (0, 1)}, {"peak_billing": False, "peak_blocks": 0},
                {"peak_billing": True, "ratio": 0.0}):
        with pytest.raises(ValueError):
            bs.co_size_options(bad)
    for bad in ({"peak": True}, {"peak_billing": True, "cap_kept": 4}, {"peak_billing": True, "peak_cap": 4},
                {"net": True}):
        with pytest.raises(ValueError, match="unknown keys"):
            bs.co_size_spec(bad, peak=True)
        with pytest.raises(ValueError, match="unknown keys"):
            bs.co_size_options(bad)


def test_engine_keywords():
    from dgen_amd.engine import Engine
    p = inspect.signature(Engine.size_with_batt).parameters
    assert p["peak"].default is False and p["peak_caps"].default is None and p["peak_blocks"].default is None
    assert p["net"].default is False
    assert list(p)[:11] == ["self", "batch", "ratio", "hours", "lo", "hi", "trace", "want", "net", "net_cap",
                            "net_blocks"]                  # positional order kept


def test_candidate_rule_on_demand_charge_rows():
    pop = _pop("com_dc_batt", 24, 20260031)
    assert pop.skip_demand_charges == 0 and pop.demand is not None and pop.demand.size
    n = pop.cols["tariff0"].size
    lo, hi = np.full(n, 5.0), np.full(n, 50.0)
    on, off = _records(pop, True), _records(pop, False)
    assert (on["dc"][pop.cols["tariff0"]] > 0).all()
    assert candidates_peak(on, pop, lo, hi, True).all()
    # demand charges not billed: only the unit-1 / unit-3 tariffs are left
    want = np.isin(off["unit"][pop.cols["tariff0"]], (1, 3))
    got = candidates_peak(off, pop, lo, hi, False)
    assert np.array_equal(got, want) and not got.all()
    # the bracket, the life and the flag on tariff0
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[0], hi2[1], lo2[2], lo2[3] = np.nan, np.inf, 0.0, 50.0
    lo2[4], hi2[4] = 50.0, 5.0
    life = pop.cols["econ_life"].copy()
    life[5], life[6], life[7], life[8] = 0, _lib.MAXY + 1, 1, _lib.MAXY
    pop.cols["econ_life"] = life
    on = on.copy()
    t9 = int(pop.cols["tariff0"][9])
    on["flags"][t9] |= _lib.ST_UNIT
    got = candidates_peak(on, pop, lo2, hi2, True)
    out = np.zeros(n, bool)
    out[[0, 1, 2, 3, 4, 5, 6]] = True
    out |= pop.cols["tariff0"] == t9
    assert np.array_equal(got, ~out) and got[7] and got[8]
    t0 = pop.cols["tariff0"].copy()
    t0[10], t0[11] = -1, on.size
    pop.cols["tariff0"] = t0
    got = candidates_peak(on, pop, lo, hi, True)
    assert not got[10] and not got[11]


def test_candidate_rule_on_kwh_per_kw_rows():
    pop = _pop("com_kwkw", 65, 20260033)
    recs = _records(pop, False)
    n = pop.cols["tariff0"].size
    lo, hi = np.full(n, 5.0), np.full(n, 50.0)
    unit = np.isin(recs["unit"][pop.cols["tariff0"]], (1, 3))
    flagged = (recs["flags"][pop.cols["tariff0"]] & _lib.ST_UNIT) != 0
    got = candidates_peak(recs, pop, lo, hi, False)
    assert np.array_equal(got, unit & ~flagged) and got.any() and (~got).any()
    # reference mode: dc_on changes nothing unless a record stands behind the tariff
    assert np.array_equal(candidates_peak(recs, pop, lo, hi, True) & ~got, (recs["dc"][pop.cols["tariff0"]] > 0)
                          & ~unit & ~flagged)
    # a storage row onto a kWh/kW tariff makes a candidate, one beyond the table does not
    kw_t = int(np.nonzero(np.isin(recs["unit"], (1, 3)))[0][0])
    plain = np.nonzero(~got & ~flagged & ~unit)[0]
    assert plain.size >= 2
    _row(pop, plain[0], kw_t)
    _row(pop, plain[1], recs.size + 3)
    got2 = candidates_peak(recs, pop, lo, hi, False)
    assert got2[plain[0]] and not got2[plain[1]]
    got[plain[0]] = True
    assert np.array_equal(got2, got)


def test_candidate_rule_on_metering_mix_rows():
    pop = _pop("metering_mix", 65, 20260023)
    dem = _pop("com_dc_batt", 8, 20260031).demand
    t = pop.tariffs.copy()
    ix = np.arange(t.size)
    t["dc"] = np.where(ix % 2 == 0, 1 + (ix // 2) % dem.size, 0)
    pop.tariffs, pop.demand = t, dem
    recs_on, recs_off = _records(pop, True), _records(pop, False)
    n = pop.cols["tariff0"].size
    lo, hi = np.full(n, 5.0), np.full(n, 50.0)
    t0 = pop.cols["tariff0"]
    ok0 = (recs_on["flags"][t0] & _lib.ST_UNIT) == 0
    on = candidates_peak(recs_on, pop, lo, hi, True)
    off = candidates_peak(recs_off, pop, lo, hi, False)
    unit = np.isin(recs_on["unit"], (1, 3))
    assert np.array_equal(on, ok0 & ((t0 % 2 == 0) | unit[t0]))
    assert np.array_equal(off, ok0 & unit[t0])
    assert len(set(recs_on["mo"][t0[on]])) >= 4          # candidates under the metering options present
    # a storage row onto a demand tariff makes a candidate only while demand charges are billed
    plain = np.nonzero(~on & ok0)[0]
    dc_t = int(np.nonzero((recs_on["dc"] > 0) & ~unit)[0][0])
    assert plain.size >= 2
    _row(pop, plain[0], dc_t)
    _row(pop, plain[1], -1)
    on2 = candidates_peak(recs_on, pop, lo, hi, True)
    off2 = candidates_peak(recs_off, pop, lo, hi, False)
    assert on2[plain[0]] and not on2[plain[1]] and not off2[plain[0]]
    # a flag on tariff0 excludes the agent whatever its rows say
    recs_on = recs_on.copy()
    recs_on["flags"][t0[plain[0]]] |= _lib.ST_UNIT
    assert not candidates_peak(recs_on, pop, lo, hi, True)[plain[0]]
