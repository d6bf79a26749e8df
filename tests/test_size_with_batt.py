"""PV sizing on the with-battery objective, host side: the binding and its
struct layouts against the header, the drop-in switch's spec and columns, the
NaN rules of co_size_summarize on hand-made results, and the test helper
bounded_brent against the oracle's (and, where it imports, scipy's) search."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from oracle import oracle as orc
from tests.swb_helpers import bounded_brent, xatol_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dgen_hip.h")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(dgen_swb_opt) S(dgen_swb_out) O(dgen_swb_opt, hours) O(dgen_swb_opt, trace_n)
  O(dgen_swb_out, system_kw) O(dgen_swb_out, lifetime_savings) O(dgen_swb_out, nfev) O(dgen_swb_out, status)
  O(dgen_swb_out, trace_x) O(dgen_swb_out, trace_f)
  printf("trace_max %d\n", DGEN_SWB_TRACE_MAX);
  return 0;
}
"""


def test_the_binding_is_declared():
    text = open(HEADER).read()
    assert re.search(r"^int32_t\s+dgen_size_with_batt\s*\(", text, flags=re.M)
    assert "dgen_size_with_batt" in _lib.EXPORTED
    L = _lib.load(build_if_missing=True)
    fn = L.dgen_size_with_batt
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 9
    assert _lib.SWB_FIELDS == _lib.SWB_F64 + _lib.SWB_I32 and len(_lib.SWB_FIELDS) == 13
    assert [f for f, _ in _lib.SwbOut._fields_] == _lib.SWB_FIELDS + ["trace_x", "trace_f"]


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert lay["dgen_swb_opt"] == ctypes.sizeof(_lib.SwbOpt) == 24
    assert lay["dgen_swb_out"] == ctypes.sizeof(_lib.SwbOut) == 15 * 8
    assert lay["dgen_swb_opt.hours"] == _lib.SwbOpt.hours.offset
    assert lay["dgen_swb_opt.trace_n"] == _lib.SwbOpt.trace_n.offset
    for f in ("system_kw", "lifetime_savings", "nfev", "status", "trace_x", "trace_f"):
        assert lay[f"dgen_swb_out.{f}"] == getattr(_lib.SwbOut, f).offset, f
    assert lay["trace_max"] == _lib.SWB_TRACE_MAX == 32


def test_spec_and_column_names():
    assert bs.CO_COLUMNS == ("pvb_opt_kw", "pvb_opt_kwh", "pvb_opt_batt_kw", "pvb_opt_npv", "pvb_opt_payback",
                             "pvb_opt_nfev", "pvb_opt_status", "pvb_opt_npv_gain")
    assert not set(bs.CO_COLUMNS) & set(bs.COLUMNS)
    assert bs.co_size_spec(True) == (0.8, 2.0)
    assert bs.co_size_spec({}) == (0.8, 2.0)
    assert bs.co_size_spec({"ratio": 0.4}) == (0.4, 2.0)
    assert bs.co_size_spec({"hours": 4}) == (0.8, 4.0)
    assert bs.co_size_spec({"ratio": 0.4, "hours": 4.0}) == (0.4, 4.0)
    for bad in (False, None, 1, (0.8, 2.0), {"pv_to_batt": 0.8}, {"ratio": 0.0}, {"ratio": -1.0},
                {"hours": float("nan")}, {"hours": float("inf")}):
        with pytest.raises(ValueError):
            bs.co_size_spec(bad)


def test_size_frame_and_size_chunk_take_the_spec():
    import inspect
    from dgen_amd import financial_functions as ff
    for fn in (ff.size_frame, ff.size_chunk):
        p = inspect.signature(fn).parameters["pv_batt_sizing"]
        assert p.default is None


def test_summarize_nan_rules():
    nan = np.nan
    H, B = _lib.ST_HOURLY_FORM, _lib.ST_BOUNDS
    res = {"system_kw": np.array([5.0, nan, 7.0, 8.0, 9.0, 3.0]),
           "bank_kwh": np.array([6.0, nan, 9.0, 10.0, 11.0, 0.0]),
           "power_kw": np.array([3.0, nan, 4.5, 5.0, 5.5, 0.0]),
           "npv": np.array([100.0, nan, 50.0, nan, 70.0, -5.0]),
           "payback_raw": np.array([7.5, nan, 1e99, 3.0, 4.0, 1e99]),
           "nfev": np.array([9, 3, 11, 10, 12, 8], np.int32),
           "status": np.array([0, H, _lib.ST_ZERO_LOAD, 0, 0, _lib.ST_EMPTY_EC], np.int32)}
    npv_ref = np.array([90.0, 10.0, 60.0, 20.0, nan, -6.0])
    st_ref = np.array([0, 0, 0, 0, 0, B], np.int32)
    s = bs.co_size_summarize(res, npv_ref, st_ref)
    assert tuple(s) == bs.CO_COLUMNS
    # valid on both sides: the difference; informational bits do not invalidate
    assert s["pvb_opt_npv_gain"][0] == 10.0 and s["pvb_opt_npv_gain"][2] == -10.0
    # the search invalid (status), its npv NaN, the sizing call's npv NaN, the sizing call's status invalid
    assert np.isnan(s["pvb_opt_npv_gain"][[1, 3, 4, 5]]).all()
    for col, m in (("kw", "system_kw"), ("kwh", "bank_kwh"), ("batt_kw", "power_kw"), ("npv", "npv"),
                   ("payback", "payback_raw"), ("nfev", "nfev"), ("status", "status")):
        assert np.array_equal(s["pvb_opt_" + col], res[m], equal_nan=True), col
    # the same rules on tensors
    torch = pytest.importorskip("torch")
    t = bs.co_size_summarize({k: torch.from_numpy(v) for k, v in res.items()}, torch.from_numpy(npv_ref),
                             torch.from_numpy(st_ref))
    for k in bs.CO_COLUMNS:
        assert np.array_equal(t[k].numpy(), s[k], equal_nan=True), k


def _quadratics(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        lo = float(rng.uniform(0.5, 50.0))
        hi = lo * float(rng.uniform(1.2, 4.0)) + float(rng.choice([0.0, 3000.0]))
        x0 = float(rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo)))     # minima inside and beyond the bracket
        c2 = float(rng.uniform(0.01, 10.0)) * float(rng.choice([1.0, 1.0, -1.0]))
        c1 = float(rng.uniform(-5.0, 5.0))
        yield lo, hi, xatol_of(lo, hi), c2, x0, c1


def test_bounded_brent_reproduces_the_oracle_search():
    """64 random quadratics (convex and concave, minima inside and outside the
    bracket, the tolerance floor of 2 and above it): the x sequence, the
    minimiser and the count of orc.brent_quadratic, bit for bit."""
    seen_tol = set()
    for lo, hi, xatol, c2, x0, c1 in _quadratics(64, 20260101):
        def f(x):
            d = x - x0
            return c2 * d * d + c1 * x
        xs, xf, n = bounded_brent(f, lo, hi, xatol)
        rx, rxf, rn = orc.brent_quadratic(lo, hi, xatol, c2, x0, c1)
        assert n == rn == len(xs) and xf == rxf, (lo, hi, c2, x0, c1)
        assert np.array_equal(np.array(xs), rx), (lo, hi, c2, x0, c1)
        assert xf in xs
        seen_tol.add(xatol > 2.0)
    assert seen_tol == {False, True}


def test_bounded_brent_equals_scipy():
    so = pytest.importorskip("scipy.optimize")
    for lo, hi, xatol, c2, x0, c1 in _quadratics(32, 20260102):
        asked = []

        def f(x):
            asked.append(float(x))
            d = x - x0
            return c2 * d * d + c1 * x
        r = so.minimize_scalar(f, bounds=(lo, hi), method="bounded", options={"xatol": xatol})
        want = list(asked)
        xs, xf, n = bounded_brent(f, lo, hi, xatol)
        assert xs == want and xf == float(r.x) and n == int(r.nfev), (lo, hi, c2, x0, c1)
