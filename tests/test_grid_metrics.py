"""Grid-exchange digest (dgen_plane_digest), the parts that need no GPU: the
entry point is exported and declared, the ctypes structure matches the header
(gcc sizeof / offsetof probe), and the pure-numpy reference the GPU tests
compare with (digest_ref) gives the answers written out here by hand."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from dgen_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# first hour of each calendar month of the non-leap year (+ the year's end)
MONTH_START = np.array([0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365], dtype=np.int64) * 24


def digest_ref(plane_hn):
    """The digest's definition in numpy.  plane_hn: [8760] or [8760, n] (any
    float dtype; the values are taken as float64).  Returns a dict of [12, n]
    arrays: import_kwh, export_kwh, peak_import_kw, peak_export_kw (float64),
    peak_import_hour, peak_export_hour (int32 hour of year, -1 = none).  Per
    month the positive part (np.where(v > 0, v, 0.0); a NaN fails the
    comparison) is summed with np.cumsum(...)[-1], which adds in hour order,
    and np.argmax gives the first hour of the maximum."""
    v = np.asarray(plane_hn).astype(np.float64)
    if v.ndim == 1:
        v = v[:, None]
    assert v.shape[0] == 8760
    n = v.shape[1]
    cols = np.arange(n)
    res = {k: np.zeros((12, n), np.float64) for k in _lib.DIGEST_F64}
    res.update({k: np.full((12, n), -1, np.int32) for k in _lib.DIGEST_I32})
    for m in range(12):
        h0, h1 = int(MONTH_START[m]), int(MONTH_START[m + 1])
        x = v[h0:h1]
        for part, s, pk, hr in ((np.where(x > 0, x, 0.0), "import_kwh", "peak_import_kw", "peak_import_hour"),
                                (np.where(x < 0, -x, 0.0), "export_kwh", "peak_export_kw", "peak_export_hour")):
            res[s][m] = np.cumsum(part, axis=0)[-1]
            a = np.argmax(part, axis=0)
            top = part[a, cols]
            res[pk][m] = top
            res[hr][m] = np.where(top > 0, h0 + a, -1).astype(np.int32)
    return res


def annual_ref(d):
    """digest_ref's months -> the year: sums added in month order, peaks the
    maximum over the months with the first such month's hour."""
    res = {}
    for k in ("import_kwh", "export_kwh"):
        s = d[k][0].copy()
        for m in range(1, 12):
            s = s + d[k][m]
        res[k] = s
    for kw, hour in (("peak_import_kw", "peak_import_hour"), ("peak_export_kw", "peak_export_hour")):
        pk, hr = d[kw][0].copy(), d[hour][0].astype(np.int64)
        for m in range(1, 12):
            better = d[kw][m] > pk
            pk = np.where(better, d[kw][m], pk)
            hr = np.where(better, d[hour][m].astype(np.int64), hr)
        res[kw], res[hour] = pk, hr
    return res


def test_library_exports_plane_digest():
    L = _lib.load(build_if_missing=True)
    assert "dgen_plane_digest" in _lib.EXPORTED
    assert hasattr(L, "dgen_plane_digest")
    assert L.dgen_plane_digest.restype is ctypes.c_int32
    assert len(L.dgen_plane_digest.argtypes) == 6
    text = open(os.path.join(REPO, "include", "dgen_hip.h")).read()
    assert "int32_t dgen_plane_digest(dgen_ctx* ctx, const void* plane, int32_t plane_f64, int64_t n," in text
    assert L.dgen_abi_version() == 14          # additive: no existing struct changed


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(dgen_digest_out)
  O(dgen_digest_out, import_kwh) O(dgen_digest_out, export_kwh) O(dgen_digest_out, peak_import_kw)
  O(dgen_digest_out, peak_export_kw) O(dgen_digest_out, peak_import_hour) O(dgen_digest_out, peak_export_hour)
  return 0;
}
"""


def test_digest_out_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    layout = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert layout["dgen_digest_out"] == ctypes.sizeof(_lib.DigestOut) == 48
    assert [name for name, _ in _lib.DigestOut._fields_] == _lib.DIGEST_FIELDS
    for f in _lib.DIGEST_FIELDS:
        assert layout[f"dgen_digest_out.{f}"] == getattr(_lib.DigestOut, f).offset, f


def hand_column():
    col = np.zeros(8760)
    col[0], col[743], col[10] = 1.5, 2.5, -3.0            # Jan: the month's last hour holds the peak
    col[744] = 7.0                                         # Feb: its first hour; no export
    #                                                        Mar: nothing
    col[2200], col[2300], col[2879] = 4.0, 4.0, -1.0       # Apr: a tie (first wins); export in the last hour
    col[3000], col[3001] = np.nan, 0.25                    # May: a NaN hour adds nothing
    col[3624], col[3625] = -0.0, 0.0                       # Jun: signed zeros are neither import nor export
    col[4344:4348] = [0.1, 0.2, 0.3, -0.6]                 # Jul: (0.1 + 0.2) + 0.3 in hour order
    col[5831] = -9.0                                       # Aug: export alone, in the last hour
    col[5832:5835] = [1e16, 1.0, 1.0]                      # Sep: sequential: each + 1.0 rounds away
    col[7295] = 3.0                                        # Oct: last hour
    col[8015] = 5.0                                        # Nov: last hour
    col[8016], col[8758], col[8759] = 6.0, -2.0, 6.5       # Dec: first hour, and the year's last
    return col


def test_digest_ref_on_a_hand_written_column():
    d = digest_ref(hand_column())
    assert all(v.shape == (12, 1) for v in d.values())
    want = {
        "import_kwh": [4.0, 7.0, 0.0, 8.0, 0.25, 0.0, 0.6000000000000001, 0.0, 1e16, 3.0, 5.0, 12.5],
        "export_kwh": [3.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.6, 9.0, 0.0, 0.0, 0.0, 2.0],
        "peak_import_kw": [2.5, 7.0, 0.0, 4.0, 0.25, 0.0, 0.3, 0.0, 1e16, 3.0, 5.0, 6.5],
        "peak_export_kw": [3.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.6, 9.0, 0.0, 0.0, 0.0, 2.0],
        "peak_import_hour": [743, 744, -1, 2200, 3001, -1, 4346, -1, 5832, 7295, 8015, 8759],
        "peak_export_hour": [10, -1, -1, 2879, -1, -1, 4347, 5831, -1, -1, -1, 8758],
    }
    for k, w in want.items():
        assert d[k][:, 0].tolist() == w, k
    assert d["import_kwh"].dtype == np.float64 and d["peak_import_hour"].dtype == np.int32
    # the +0.0 the empty months report is a positive zero
    assert not np.signbit(d["import_kwh"]).any() and not np.signbit(d["export_kwh"]).any()
    a = annual_ref(d)
    # Python adds left to right: the months in order
    assert a["import_kwh"][0] == 4.0 + 7.0 + 0.0 + 8.0 + 0.25 + 0.0 + 0.6000000000000001 + 0.0 + 1e16 + 3.0 + 5.0 + 12.5
    assert a["export_kwh"][0] == 3.0 + 1.0 + 0.6 + 9.0 + 2.0
    assert (a["peak_import_kw"][0], a["peak_import_hour"][0]) == (1e16, 5832)
    assert (a["peak_export_kw"][0], a["peak_export_hour"][0]) == (9.0, 5831)


def test_month_table_is_whole_days_and_quads():
    assert MONTH_START[0] == 0 and MONTH_START[-1] == _lib.NH
    assert np.all(MONTH_START % 24 == 0) and np.all(np.diff(MONTH_START) // 24 == [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])


def test_drop_in_column_names():
    from dgen_amd import grid_metrics as gm
    assert len(gm.COLUMNS) == 18 and len(set(gm.COLUMNS)) == 18
    for case in ("baseline", "pvonly", "with_batt"):
        for stem in ("grid_import_kwh", "grid_export_kwh", "peak_import_kw", "peak_import_hour",
                     "peak_export_kw", "peak_export_hour"):
            assert f"{stem}_{case}" in gm.COLUMNS
