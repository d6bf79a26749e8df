"""Battery dispatch summary (dgen_batt_summary), the parts that need no GPU: the
entry point is exported and declared, the ctypes structures match the header
(gcc sizeof / offsetof probe), the numpy reference the GPU tests compare with
(summary_ref, built on the oracle's batt_dispatch) gives the answers worked
out by hand below and agrees with an independent hour loop, and
batt_metrics.annual and the drop-in column names are what the documents say."""
import ctypes
import os
import subprocess

import numpy as np

from dgen_amd import _lib
from dgen_amd import batt_metrics as bm
from dgen_amd.config import EngineConfig
from oracle import oracle as orc
from tests.test_grid_metrics import MONTH_START
from tests.test_oracle import _py_target

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = _lib.NH


def summary_ref(load, pv, bank, power, cfg, midday=_lib.BATT_SUMMARY_MIDDAY):
    """dgen_batt_summary's definition for one agent in numpy, on the oracle's
    dispatch (orc.batt_dispatch: system output and grid-to-load per hour).
    load, pv: [8760] kW; bank (kWh), power (kW): the sized battery (0, 0:
    none); cfg: orc.Cfg.  The flows come back from the system output,
    c = pv - sysgen where nn < 0 and d = sysgen - pv elsewhere, and the SOC is
    batt_init_soc plus the cumulative sum of c eta_in / bank - d / (eta_out
    bank).  Returns {member: [12]} (float64 / int32), each month summed with
    np.cumsum(...)[-1] (hour order), plus "_hours": per-hour arrays the GPU
    test's ambiguity bands read (never device output)."""
    load = np.asarray(load, np.float64)
    pv = np.asarray(pv, np.float64)
    bank, power = float(bank), float(power)
    if not bank > 0.0:
        bank = power = 0.0
    sg, g2l = orc.batt_dispatch(load, pv, bank, power, cfg)
    nn = load - pv
    chg = nn < 0.0
    c = np.where(chg, pv - sg, 0.0)
    d = np.where(chg, 0.0, sg - pv)
    if bank > 0.0:
        soc = cfg.batt_init_soc + np.cumsum(c * cfg.batt_eta_in / bank - d / (cfg.batt_eta_out * bank))
    else:
        soc = np.full(NH, cfg.batt_init_soc)
    sur = np.maximum(-nn, 0.0)
    hod = np.arange(NH) % 24
    mid = (hod >= midday[0]) & (hod <= midday[1])
    soc_hi, soc_lo = cfg.batt_max_soc - 1e-9, cfg.batt_min_soc + 1e-9
    full = soc >= soc_hi
    hourly = {
        "pv_kwh": pv, "surplus_kwh": sur, "pv_to_batt_kwh": c, "pv_to_grid_kwh": sur - c,
        "pv_to_load_kwh": np.minimum(load, pv), "batt_to_load_kwh": d, "grid_to_load_kwh": g2l,
        "surplus_mid_kwh": np.where(mid, sur, 0.0), "pv_to_batt_mid_kwh": np.where(mid, c, 0.0),
        "pv_to_grid_mid_kwh": np.where(mid, sur - c, 0.0),
        "hours_charge": c > 0.0, "hours_discharge": d > 0.0,
        "hours_soc_bound": (sur > 1e-6) & full,
        "hours_power_bound": (sur > power + 1e-6) & (soc < soc_hi),
        "hours_empty": (nn > 1e-6) & (soc <= soc_lo),
        "hours_discharge_power_bound": (d > power * (1.0 - 1e-9)) & (power > 0.0),
    }
    res = {k: np.zeros(12, np.float64) for k in _lib.BATT_SUMMARY_F64}
    res.update({k: np.zeros(12, np.int32) for k in _lib.BATT_SUMMARY_I32})
    for m in range(12):
        h0, h1 = int(MONTH_START[m]), int(MONTH_START[m + 1])
        for k, v in hourly.items():
            res[k][m] = np.cumsum(v[h0:h1].astype(res[k].dtype))[-1]
        res["soc_min"][m], res["soc_max"][m], res["soc_end"][m] = soc[h0:h1].min(), soc[h0:h1].max(), soc[h1 - 1]
    res["_hours"] = {"soc": soc, "sur": sur, "nn": nn, "d": d}
    return res


def test_library_exports_batt_summary():
    L = _lib.load(build_if_missing=True)
    assert "dgen_batt_summary" in _lib.EXPORTED
    assert hasattr(L, "dgen_batt_summary")
    assert L.dgen_batt_summary.restype is ctypes.c_int32
    assert len(L.dgen_batt_summary.argtypes) == 8
    text = open(os.path.join(REPO, "include", "dgen_hip.h")).read()
    assert "int32_t dgen_batt_summary(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents," in text
    assert L.dgen_abi_version() == 14          # additive: no existing struct changed


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(dgen_batt_summary_opt) O(dgen_batt_summary_opt, mid_lo) O(dgen_batt_summary_opt, mid_hi)
  S(dgen_batt_summary_out)
FIELDS
  return 0;
}
"""


def test_summary_structs_match_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("FIELDS", "\n".join(f"  O(dgen_batt_summary_out, {f})"
                                                     for f in _lib.BATT_SUMMARY_FIELDS)))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    layout = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert layout["dgen_batt_summary_opt"] == ctypes.sizeof(_lib.BattSummaryOpt) == 8
    assert layout["dgen_batt_summary_opt.mid_lo"] == _lib.BattSummaryOpt.mid_lo.offset == 0
    assert layout["dgen_batt_summary_opt.mid_hi"] == _lib.BattSummaryOpt.mid_hi.offset == 4
    assert layout["dgen_batt_summary_out"] == ctypes.sizeof(_lib.BattSummaryOut) == 8 * 19
    assert [name for name, _ in _lib.BattSummaryOut._fields_] == _lib.BATT_SUMMARY_FIELDS
    assert len(_lib.BATT_SUMMARY_F64) == 13 and len(_lib.BATT_SUMMARY_I32) == 6
    for f in _lib.BATT_SUMMARY_FIELDS:
        assert layout[f"dgen_batt_summary_out.{f}"] == getattr(_lib.BattSummaryOut, f).offset, f


def hand_year():
    """Load 1 kW all year, PV 3 kW in hours 10-13 of every day."""
    load = np.ones(NH)
    pv = np.where((np.arange(NH) % 24 >= 10) & (np.arange(NH) % 24 <= 13), 3.0, 0.0)
    return load, pv


def test_summary_ref_on_a_hand_written_year():
    """Bank 10 kWh / 2.5 kW, eta 0.9408 each way, SOC in [0.10, 0.95] from 0.30.
    A day has 20 deficit hours of 1 kW (hours 0-9, 14-23) and 4 surplus hours
    of 2 kW.  With s the SOC at the day's first hour the plan can deliver
    avail = (s - 0.1) x 10 x 0.9408 kWh; no hour is above the power limit, so
    the target spreads it evenly: dd = avail / 20 in each deficit hour, each
    lowering the SOC by dd / 9.408 = (s - 0.1) / 20.  Ten such hours take the
    SOC to s/2 + 0.05 by hour 10; the surplus (8 kWh, 2 <= 2.5 kW) refills the
    bank to 0.95 with C = (0.95 - s/2 - 0.05) x 10 / 0.9408 kWh (at most 7.97 <
    8), and the evening's ten hours take it to 0.95 - (s - 0.1) / 2: the next
    day starts at s' = 1 - s/2 (0.30, 0.85, 0.575, 0.7125, ... -> 2/3).  So in
    January (31 days):
      batt_to_load = sum of avail = sum (s - 0.1) x 9.408
      pv_to_batt   = sum of C     = sum (0.9 - s/2) / 0.09408
      the bank is full at the end of surplus hour ceil(C / 2) of the day's four
      and of every surplus hour after it: hours_soc_bound = sum 5 - ceil(C / 2),
      2 on days 2, 4 and 6 (s >= 0.67104), 1 on every other day: 34
      soc_max = 0.95; soc_min = the first morning's 0.30 / 2 + 0.05 = 0.20
      midday window 11..15 holds surplus hours 11, 12, 13: surplus_mid = 31 x 6,
      and all of C but hour 10's 2 kWh (C > 2 every day): pv_to_batt_mid =
      pv_to_batt - 62, pv_to_grid_mid = 186 - pv_to_batt_mid."""
    load, pv = hand_year()
    cfg = orc.make_cfg()
    r = summary_ref(load, pv, 10.0, 2.5, cfg)
    s, b2l, p2b, bound = 0.30, 0.0, 0.0, 0
    for _ in range(31):
        C = (0.9 - s / 2) / 0.09408
        assert 2.0 < C < 8.0 and abs(C / 2 - round(C / 2)) > 1e-3
        b2l += (s - 0.1) * 9.408
        p2b += C
        bound += 5 - int(np.ceil(C / 2))
        s = 1.0 - s / 2
    assert bound == 34
    close = lambda a, b: abs(a - b) <= 1e-9 * max(1.0, abs(b))
    assert close(r["batt_to_load_kwh"][0], b2l), (r["batt_to_load_kwh"][0], b2l)
    assert close(r["pv_to_batt_kwh"][0], p2b), (r["pv_to_batt_kwh"][0], p2b)
    assert r["hours_soc_bound"][0] == 34
    assert close(r["soc_max"][0], 0.95) and close(r["soc_min"][0], 0.20)
    assert close(r["soc_end"][0], s - 0.0)                     # the SOC February starts at
    assert r["surplus_kwh"][0] == 31 * 8.0 and r["surplus_mid_kwh"][0] == 31 * 6.0
    assert close(r["pv_to_batt_mid_kwh"][0], p2b - 62.0)
    assert close(r["pv_to_grid_mid_kwh"][0], 186.0 - (p2b - 62.0))
    assert close(r["pv_to_grid_kwh"][0], 248.0 - p2b)
    assert r["pv_kwh"][0] == 31 * 12.0 and r["pv_to_load_kwh"][0] == 31 * 4.0
    assert close(r["grid_to_load_kwh"][0], 31 * 20.0 - b2l)
    assert r["hours_discharge"][0] == 31 * 20 and r["hours_empty"][0] == 0
    assert r["hours_power_bound"][0] == 0 and r["hours_discharge_power_bound"][0] == 0
    # the month's load is what PV, battery and grid delivered
    for m in range(12):
        tot = r["pv_to_load_kwh"][m] + r["batt_to_load_kwh"][m] + r["grid_to_load_kwh"][m]
        assert close(tot, (MONTH_START[m + 1] - MONTH_START[m]) * 1.0), m
    # a 1 kW converter: every surplus hour is power-bound until the bank is full
    q = summary_ref(load, pv, 10.0, 1.0, cfg)
    assert q["pv_to_batt_kwh"][0] <= 31 * 4.0 + 1e-9
    assert (q["hours_power_bound"] + q["hours_soc_bound"] == (MONTH_START[1:] - MONTH_START[:-1]) // 6).all()
    # no bank: nothing flows, the SOC stays where it starts, the grid serves every deficit
    z = summary_ref(load, pv, 0.0, 0.0, cfg)
    assert not z["pv_to_batt_kwh"].any() and not z["batt_to_load_kwh"].any() and not z["hours_charge"].any()
    assert (z["soc_min"] == 0.30).all() and (z["soc_max"] == 0.30).all() and (z["soc_end"] == 0.30).all()
    assert z["grid_to_load_kwh"][0] == 31 * 20.0 and z["pv_to_grid_kwh"][0] == 31 * 8.0
    # the whole day as the window: the midday sums are the full ones
    w = summary_ref(load, pv, 10.0, 2.5, cfg, midday=(0, 23))
    for k in ("surplus", "pv_to_batt", "pv_to_grid"):
        assert np.array_equal(w[f"{k}_mid_kwh"], w[f"{k}_kwh"]), k


def _loop_summary(load, pv, bank, power, cfg, midday=_lib.BATT_SUMMARY_MIDDAY):
    """An hour loop of its own (tests/test_oracle._py_dispatch's form, with the
    flows kept): bisection target per day, branchy dispatch, running sums."""
    d = np.maximum(load - pv, 0.0)
    soc, target = cfg.batt_init_soc, 0.0
    res = {k: np.zeros(12) for k in _lib.BATT_SUMMARY_F64}
    res.update({k: np.zeros(12, np.int64) for k in _lib.BATT_SUMMARY_I32})
    res["soc_min"][:], res["soc_max"][:] = np.inf, -np.inf
    m = 0
    for h in range(NH):
        if h == MONTH_START[m + 1]:
            m += 1
        n = load[h] - pv[h]
        avail = max((soc - cfg.batt_min_soc) * bank * cfg.batt_eta_out, 0.0)
        if h % 24 == 0:
            target = _py_target(d[h:h + 24], power, avail)
        c = x = 0.0
        if n < 0:
            room = max((cfg.batt_max_soc - soc) * bank / cfg.batt_eta_in, 0.0)
            c = min(-n, power, room)
            soc += c * cfg.batt_eta_in / bank
        else:
            x = min(max(n - target, 0.0), power, avail)
            soc -= x / (cfg.batt_eta_out * bank)
        sur = max(-n, 0.0)
        mid = midday[0] <= h % 24 <= midday[1]
        for k, v in (("pv_kwh", pv[h]), ("surplus_kwh", sur), ("pv_to_batt_kwh", c), ("pv_to_grid_kwh", sur - c),
                     ("pv_to_load_kwh", min(load[h], pv[h])), ("batt_to_load_kwh", x),
                     ("grid_to_load_kwh", max(n, 0.0) - x), ("surplus_mid_kwh", sur * mid),
                     ("pv_to_batt_mid_kwh", c * mid), ("pv_to_grid_mid_kwh", (sur - c) * mid),
                     ("hours_charge", c > 0), ("hours_discharge", x > 0),
                     ("hours_soc_bound", sur > 1e-6 and soc >= cfg.batt_max_soc - 1e-9),
                     ("hours_power_bound", sur > power + 1e-6 and soc < cfg.batt_max_soc - 1e-9),
                     ("hours_empty", n > 1e-6 and soc <= cfg.batt_min_soc + 1e-9),
                     ("hours_discharge_power_bound", x > power * (1 - 1e-9) and power > 0)):
            res[k][m] += v
        res["soc_min"][m], res["soc_max"][m] = min(res["soc_min"][m], soc), max(res["soc_max"][m], soc)
        res["soc_end"][m] = soc
    return res


def test_summary_ref_matches_an_independent_hour_loop():
    """The data of tests/test_oracle.test_dispatch_rule_matches_python_restatement:
    evening peaks, a PV bell, days with an hour above the power limit."""
    rng = np.random.default_rng(41)
    hod = np.arange(NH) % 24
    load = 0.6 + 0.9 * np.exp(-((hod - 19) / 2.5) ** 2) + 0.3 * rng.random(NH)
    load[rng.integers(0, NH, 40)] += 4.0
    pv = np.maximum(0.0, np.sin((hod - 6) / 12 * np.pi)) * (2.2 + rng.random(NH))
    cfg = orc.make_cfg()
    days = (MONTH_START[1:] - MONTH_START[:-1]) // 24
    seen = {k: 0 for k in _lib.BATT_SUMMARY_I32}
    for bank, power in ((10.0, 2.5), (3.0, 0.75)):         # the small bank also runs empty
        ref = summary_ref(load, pv, bank, power, cfg)
        loop = _loop_summary(load, pv, bank, power, cfg)
        for k in _lib.BATT_SUMMARY_F64:
            tol = 1e-9 if k.startswith("soc") else 1e-9 * np.maximum(1.0, np.abs(loop[k]))
            assert (np.abs(ref[k] - loop[k]) <= tol).all(), (bank, k, np.abs(ref[k] - loop[k]).max())
        # the two SOC paths differ by rounding (1e-13): an hour within 1e-11 of
        # a count's 1e-9 band edge could fall either way; this year has none
        # (asserted), so the band counts are equal
        h = ref["_hours"]
        assert np.abs(h["soc"] - (cfg.batt_max_soc - 1e-9)).min() > 1e-11
        assert np.abs(h["soc"] - (cfg.batt_min_soc + 1e-9)).min() > 1e-11
        assert np.abs(h["d"] - power * (1.0 - 1e-9)).min() > 1e-11 * power
        for k in ("hours_soc_bound", "hours_power_bound", "hours_empty", "hours_discharge_power_bound"):
            assert np.array_equal(ref[k], loop[k]), (bank, k, ref[k], loop[k])
        # the flow counts have no band: at the moment the bank fills or empties
        # a flow of rounding dust (1e-16 kWh) is an hour in the loop and
        # vanishes in the reference's pv - sysgen (or the other way round);
        # such moments come at most twice a day
        for k in ("hours_charge", "hours_discharge"):
            assert (np.abs(ref[k] - loop[k]) <= 2 * days).all(), (bank, k, ref[k] - loop[k])
        for k in seen:
            seen[k] += int(ref[k].sum())
    assert all(v > 0 for v in seen.values()), seen


def test_annual_reduces_the_months():
    rng = np.random.default_rng(5)
    n = 7
    d = {k: rng.uniform(0.0, 50.0, (12, n)) for k in _lib.BATT_SUMMARY_F64}
    d.update({k: rng.integers(0, 200, (12, n)).astype(np.int32) for k in _lib.BATT_SUMMARY_I32})
    d["soc_min"], d["soc_max"] = rng.uniform(0.1, 0.5, (12, n)), rng.uniform(0.5, 0.95, (12, n))
    d["surplus_mid_kwh"][:, 0] = 0.0            # no midday surplus: the capture ratio is 0, not 0 / 0
    d["pv_to_batt_mid_kwh"][:, 0] = 0.0
    for k in ("pv_to_load_kwh", "batt_to_load_kwh", "grid_to_load_kwh"):
        d[k][:, 1] = 0.0                        # no load at all (a flagged agent's zeros)
    bank = rng.uniform(5.0, 20.0, n)
    bank[2] = 0.0                               # no bank: no cycles
    cfg = EngineConfig()
    a = bm.annual(d, bank, cfg)
    assert sorted(a) == sorted(bm.ANNUAL)
    for k in bm.KWH_MEMBERS + bm.COUNT_MEMBERS:
        want = d[k][0].copy()
        for m in range(1, 12):
            want = want + d[k][m]               # month order
        assert np.array_equal(a[k], want), k
        assert a[k].dtype == d[k].dtype
    assert np.array_equal(a["soc_min"], d["soc_min"].min(axis=0))
    assert np.array_equal(a["soc_max"], d["soc_max"].max(axis=0))
    assert np.array_equal(a["soc_end"], d["soc_end"][11])
    cap = a["capture_mid_frac"]
    assert cap[0] == 0.0 and np.array_equal(cap[1:], a["pv_to_batt_mid_kwh"][1:] / a["surplus_mid_kwh"][1:])
    cyc = a["equiv_full_cycles"]
    assert cyc[2] == 0.0
    ok = bank > 0
    assert np.array_equal(cyc[ok], a["batt_to_load_kwh"][ok] / cfg.batt_eta_out / (bank[ok] * (0.95 - 0.10)))
    ss = a["self_sufficiency_frac"]
    assert ss[1] == 0.0
    load = (a["pv_to_load_kwh"] + a["batt_to_load_kwh"]) + a["grid_to_load_kwh"]
    rows = [0, 2, 3]
    assert np.array_equal(ss[rows], 1.0 - a["grid_to_load_kwh"][rows] / load[rows])
    # torch tensors give the same bits
    import torch
    t = bm.annual({k: torch.from_numpy(v) for k, v in d.items()}, torch.from_numpy(bank), cfg)
    for k in bm.ANNUAL:
        assert np.array_equal(t[k].numpy(), a[k]), k
    # the hand-written year: one equivalent full cycle is 8.5 kWh of cell energy
    load_h, pv_h = hand_year()
    r = summary_ref(load_h, pv_h, 10.0, 2.5, orc.make_cfg())
    y = bm.annual({k: r[k][:, None] for k in _lib.BATT_SUMMARY_FIELDS}, np.array([10.0]), cfg)
    assert abs(y["equiv_full_cycles"][0] - r["batt_to_load_kwh"].sum() / 0.9408 / 8.5) < 1e-9
    assert 0.0 < y["capture_mid_frac"][0] < 1.0 and 0.0 < y["self_sufficiency_frac"][0] < 1.0


def test_drop_in_column_names():
    assert bm.PREFIX == "batt_diag_"
    assert len(bm.COLUMNS) == len(set(bm.COLUMNS)) == 10 + 3 + 6 + 3
    assert all(c.startswith("batt_diag_") for c in bm.COLUMNS)
    for k in _lib.BATT_SUMMARY_FIELDS + ["capture_mid_frac", "equiv_full_cycles", "self_sufficiency_frac"]:
        assert f"batt_diag_{k}" in bm.COLUMNS, k
    from dgen_amd import grid_metrics as gm
    assert not set(bm.COLUMNS) & set(gm.COLUMNS)
    import inspect
    from dgen_amd import financial_functions as ff
    for f in (ff.size_frame, ff.size_chunk):
        assert inspect.signature(f).parameters["batt_metrics"].default is False
