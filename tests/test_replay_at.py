"""Dispatch replay at a caller-given PV size and bank (dgen_replay_at), the
parts that need no GPU: the entry point is exported and declared,
_lib.ReplayPlanes matches the header (gcc sizeof / offsetof probe),
batt_metrics.replay_outputs lays the caller's columns out in the batch's
device order and gathers the results back, batt_metrics.replay_columns is
annual() with the replay's own bank, and the drop-in switches' "dispatch" key
parses, defaults to off and names its columns exactly."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from dgen_amd import _lib
from dgen_amd import batt_metrics as bm
from dgen_amd import batt_sizing as bs
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_replay_at():
    L = _lib.load(build_if_missing=True)
    assert "dgen_replay_at" in _lib.EXPORTED
    assert hasattr(L, "dgen_replay_at")
    assert L.dgen_replay_at.restype is ctypes.c_int32
    assert len(L.dgen_replay_at.argtypes) == 14
    text = open(os.path.join(REPO, "include", "dgen_hip.h")).read()
    assert "int32_t dgen_replay_at(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents," in text
    assert "#define DGEN_ABI_VERSION 14" in text
    assert L.dgen_abi_version() == 14          # additive: no existing struct changed


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(dgen_replay_planes) O(dgen_replay_planes, baseline) O(dgen_replay_planes, pvonly)
  O(dgen_replay_planes, with_batt) O(dgen_replay_planes, f64) O(dgen_replay_planes, pad)
  return 0;
}
"""


def test_replay_planes_match_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    layout = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert layout["dgen_replay_planes"] == ctypes.sizeof(_lib.ReplayPlanes) == 32
    assert [f[0] for f in _lib.ReplayPlanes._fields_] == _lib.REPLAY_PLANES + ["f64", "pad"]
    assert _lib.REPLAY_PLANES == ["baseline", "pvonly", "with_batt"]
    for f in _lib.REPLAY_PLANES + ["f64", "pad"]:
        assert layout[f"dgen_replay_planes.{f}"] == getattr(_lib.ReplayPlanes, f).offset, f


class _Batch:
    def __init__(self, perm):
        self.perm = None if perm is None else np.asarray(perm, np.int64)
        self.n = 5


class _Engine:
    """Engine.replay_at on the host: every output is a function of the device
    row's own inputs, so a wrong permutation shows."""
    cfg = EngineConfig()

    def _to_dev(self, a, dtype):
        return a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, copy=True)).to(dtype)

    def replay_at(self, batch, kw, bank_kwh, bank_kw, want, midday, planes):
        self.seen = (kw.clone(), bank_kwh.clone(), None if bank_kw is None else bank_kw.clone(), want, midday, planes)
        m = torch.arange(1, 13, dtype=torch.float64).view(12, 1)
        d = {"pv_kwh": m * kw.view(1, -1), "hours_charge": (m * bank_kwh.view(1, -1)).to(torch.int32),
             "bank_kwh": bank_kwh * 2.0, "power_kw": bank_kwh if bank_kw is None else bank_kw,
             "status": (kw < 0).to(torch.int32)}
        if planes:
            d["with_batt"] = kw.view(1, -1, 1).expand(_lib.NH // 4, kw.numel(), 4).contiguous()
        return d


@pytest.mark.parametrize("perm", [None, [3, 0, 4, 1, 2]])
def test_replay_outputs_is_in_caller_order(perm):
    eng, batch = _Engine(), _Batch(perm)
    kw = np.array([1.0, 2.0, -3.0, 4.0, 5.0])
    kwh = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    pkw = np.array([0.5, 0.25, 0.125, 1.5, 2.5])
    d = bm.replay_outputs(eng, batch, kw, kwh, pkw, want=("pv_kwh", "hours_charge"), midday=(9, 16), planes="f64")
    p = np.arange(5) if perm is None else np.asarray(perm)
    # device row j was handed caller row perm[j]
    assert np.array_equal(eng.seen[0].numpy(), kw[p]) and np.array_equal(eng.seen[1].numpy(), kwh[p])
    assert np.array_equal(eng.seen[2].numpy(), pkw[p])
    assert eng.seen[3:] == (("pv_kwh", "hours_charge"), (9, 16), "f64")
    # ... and every [n] and [12, n] result is back in caller order
    mth = np.arange(1, 13)[:, None]
    assert np.array_equal(d["pv_kwh"].numpy(), mth * kw[None, :])
    assert np.array_equal(d["hours_charge"].numpy(), (mth * kwh[None, :]).astype(np.int32))
    assert np.array_equal(d["bank_kwh"].numpy(), 2.0 * kwh) and np.array_equal(d["power_kw"].numpy(), pkw)
    assert np.array_equal(d["status"].numpy(), [0, 0, 1, 0, 0])
    # the planes keep the batch's device order (the tiles' column j is device row j)
    assert np.array_equal(d["with_batt"][0, :, 0].numpy(), kw[p])
    # bank_kw None stays None (the library's 2-hour bank)
    d = bm.replay_outputs(eng, batch, torch.from_numpy(kw), torch.from_numpy(kwh))
    assert eng.seen[2] is None and eng.seen[3] is None and eng.seen[5] is None
    assert np.array_equal(d["power_kw"].numpy(), kwh)


def test_replay_columns_on_a_hand_made_month_table():
    """Two agents, every month alike.  Agent 0: 10 kWh of battery-to-load a
    month from a 20 kWh bank, eta_out 0.9408, usable 0.85 of the bank: 120 /
    0.9408 / 17 cycles; midday capture 3 / 4; load 10 + 10 + 20 a month, half
    of it from the grid.  Agent 1 has no bank."""
    cfg = EngineConfig()
    one = np.ones((12, 2))
    d = {k: 0.0 * one for k in _lib.BATT_SUMMARY_F64}
    d.update({k: np.zeros((12, 2), np.int32) for k in _lib.BATT_SUMMARY_I32})
    d["batt_to_load_kwh"] = one * [10.0, 0.0]
    d["pv_to_load_kwh"] = one * [10.0, 5.0]
    d["grid_to_load_kwh"] = one * [20.0, 15.0]
    d["surplus_mid_kwh"] = one * [4.0, 4.0]
    d["pv_to_batt_mid_kwh"] = one * [3.0, 0.0]
    d["soc_min"] = one * [0.1, 0.3]
    d["soc_min"][5, 0] = 0.05
    d["soc_max"] = one * [0.95, 0.3]
    d["soc_end"] = np.arange(12.0)[:, None] * [0.01, 0.0] + 0.3
    d["hours_charge"] = (one * [7, 0]).astype(np.int32)
    d["bank_kwh"] = np.array([20.0, 0.0])
    d["power_kw"] = np.array([5.0, 0.0])
    d["status"] = np.zeros(2, np.int32)
    for prefix in (bm.PREFIX, bs.DIAG_PREFIX, bs.CO_DIAG_PREFIX):
        c = bm.replay_columns(d, cfg, prefix)
        assert list(c) == [prefix + k for k in bm.ANNUAL] and len(c) == 22
        g = lambda k: c[prefix + k]
        assert np.array_equal(g("batt_to_load_kwh"), [120.0, 0.0]) and np.array_equal(g("grid_to_load_kwh"), [240.0, 180.0])
        assert g("hours_charge").dtype == np.int64 and np.array_equal(g("hours_charge"), [84, 0])
        assert np.array_equal(g("soc_min"), [0.05, 0.3]) and np.array_equal(g("soc_max"), [0.95, 0.3])
        assert np.array_equal(g("soc_end"), d["soc_end"][11])
        assert np.array_equal(g("capture_mid_frac"), [36.0 / 48.0, 0.0])
        assert g("equiv_full_cycles")[1] == 0.0
        assert g("equiv_full_cycles")[0] == 120.0 / cfg.batt_eta_out / (20.0 * (cfg.batt_max_soc - cfg.batt_min_soc))
        assert np.array_equal(g("self_sufficiency_frac"), [1.0 - 240.0 / 480.0, 1.0 - 180.0 / 240.0])
    # the same bits from tensors, and the same as annual() on the members with the replay's bank
    t = bm.replay_columns({k: torch.from_numpy(v) for k, v in d.items()}, cfg)
    a = bm.annual({k: d[k] for k in _lib.BATT_SUMMARY_FIELDS}, d["bank_kwh"], cfg)
    for k in bm.ANNUAL:
        assert np.array_equal(t[bm.PREFIX + k], c[bs.CO_DIAG_PREFIX + k]), k
        assert np.array_equal(t[bm.PREFIX + k], a[k]), k


def test_dispatch_spec_key_parses_and_defaults_to_off():
    for spec in (True, None, {}, {"pv_to_batt": (0.8,)}, ((0.8,), (2.0,)), {"dispatch": False}):
        assert bs.dispatch(spec) is False, spec
    assert bs.dispatch({"dispatch": True}) is True
    assert bs.dispatch({"pv_to_batt": (0.4, 0.8), "net_billing": True, "dispatch": True}) is True
    # the key is no part of the grid, of the (ratio, hours) pair or of the search's keywords
    assert bs.grid({"dispatch": True}) == bs.grid({})
    assert bs.grid({"pv_to_batt": (0.4,), "hours": (4.0,), "dispatch": True}) == ((0.4,), (4.0,))
    with pytest.raises(ValueError):
        bs.grid({"dispatch": True, "dispatched": True})
    assert bs.co_size_spec({"ratio": 1.2, "hours": 4.0, "dispatch": True}, peak=True) == (1.2, 4.0)
    assert bs.co_size_options({"dispatch": True}) == {}
    assert bs.co_size_options({"dispatch": True, "net_billing": True, "net_cap": 8}) == {"net": True, "net_cap": 8}
    with pytest.raises(ValueError):          # a bool in both specs
        bs.co_size_options({"dispatch": 1})
    with pytest.raises(ValueError):
        bs.grid({"dispatch": 1})
    with pytest.raises(ValueError):
        bs.grid({"pv_to_batt": (0.8,), "dispatch": "yes"})
    with pytest.raises(ValueError):          # the keys the two-argument form always admitted are unchanged
        bs.co_size_spec({"dispatch": True})
    for f in (ff.size_frame, ff.size_chunk):
        assert inspect.signature(f).parameters["batt_sizing"].default is None
        assert inspect.signature(f).parameters["pv_batt_sizing"].default is None


def test_dispatch_column_names():
    assert bs.DIAG_PREFIX == "batt_opt_diag_" and bs.CO_DIAG_PREFIX == "pvb_opt_diag_"
    for spec in (True, {}, {"dispatch": False}, ((0.8,), (2.0,))):
        assert bs.columns_of(spec) == bs.COLUMNS
        assert bs.co_columns_of(spec if isinstance(spec, (dict, bool)) else True) == bs.CO_COLUMNS
    on = bs.columns_of({"dispatch": True})
    assert on[:7] == bs.COLUMNS and len(on) == 7 + 22
    assert on[7:] == tuple("batt_opt_diag_" + c[len(bm.PREFIX):] for c in bm.COLUMNS)
    co = bs.co_columns_of({"ratio": 1.2, "dispatch": True})
    assert co[:8] == bs.CO_COLUMNS and len(co) == 8 + 22
    assert co[8:] == tuple("pvb_opt_diag_" + c[len(bm.PREFIX):] for c in bm.COLUMNS)
    for k in _lib.BATT_SUMMARY_FIELDS + ["capture_mid_frac", "equiv_full_cycles", "self_sufficiency_frac"]:
        assert f"batt_opt_diag_{k}" in on and f"pvb_opt_diag_{k}" in co, k
    assert len(set(on) | set(co) | set(bm.COLUMNS)) == 29 + 30 + 22
