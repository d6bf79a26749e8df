"""Evaluation at caller-given sizes (dgen_eval_agents, dgen_objective_curve),
the parts that need no GPU: both entry points are exported and declared with
the header's argument counts, the ctypes curve structure matches the header
(gcc sizeof / offsetof probe), the build guard knows the one-agent-per-wave
fallback of every 32-lane k_eval_w instantiation, and sensitivity's size grid
and order mapping on plain numpy."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from dgen_amd import _lib, sensitivity, spill_guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_args(name):
    """Number of parameters of `name`'s declaration in include/dgen_hip.h."""
    text = open(os.path.join(REPO, "include", "dgen_hip.h")).read()
    m = re.search(r"int32_t " + name + r"\(([^;]*)\);", text)
    assert m, name
    return len(m.group(1).split(","))


def test_library_exports_the_evaluation_entry_points():
    L = _lib.load(build_if_missing=True)
    for name, n_args in (("dgen_eval_agents", 10), ("dgen_objective_curve", 11)):
        assert name in _lib.EXPORTED
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int32
        assert len(fn.argtypes) == n_args == _header_args(name), name
    assert L.dgen_abi_version() == 14          # additive: no existing struct changed


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(dgen_curve_out)
  O(dgen_curve_out, npv) O(dgen_curve_out, payback_raw) O(dgen_curve_out, first_with)
  O(dgen_curve_out, first_without) O(dgen_curve_out, total_cost) O(dgen_curve_out, tariff)
  O(dgen_curve_out, switched) O(dgen_curve_out, status)
  return 0;
}
"""


def test_curve_out_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    layout = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert layout["dgen_curve_out"] == ctypes.sizeof(_lib.CurveOut) == 64
    assert [name for name, _ in _lib.CurveOut._fields_] == _lib.CURVE_FIELDS
    for f in _lib.CURVE_FIELDS:
        assert layout[f"dgen_curve_out.{f}"] == getattr(_lib.CurveOut, f).offset, f


TAIL = "EEv11dgen_tables11dgen_agents12dgen_outputs8dgen_cfglllPvPcPKdi14dgen_curve_outi"


@pytest.mark.parametrize("targs,macro", [
    ("ILi32ELb0ELb0ELb0", "DGEN_NO2_EVAL"),
    ("ILi32ELb0ELb1ELb0", "DGEN_NO2_EVAL"),
    ("ILi32ELb1ELb1ELb0", "DGEN_NO2_EVAL_DC"),
    ("ILi32ELb1ELb0ELb0", "DGEN_NO2_EVAL_DC"),
    ("ILi32ELb1ELb1ELb1", "DGEN_NO2_EVAL_PK"),
])
def test_guard_withdraws_a_flagged_eval_kernel(targs, macro):
    """A fabricated hit on a 32-lane k_eval_w instantiation maps to the
    kernel's own macro (not k_size_w's) and is never fatal."""
    sym = "_ZN9dgen_srch8k_eval_w" + targs + TAIL
    macros, fatal = spill_guard.remedies({sym: [(".LBB0_1", ["scratch_store_dword off, v1, s32"])]})
    assert macros == [macro] and fatal == []


def test_guard_has_no_remedy_for_the_one_agent_eval_kernel():
    sym = "_ZN9dgen_srch8k_eval_wILi64ELb0ELb0ELb0" + TAIL
    macros, fatal = spill_guard.remedies({sym: [(".LBB0_1", ["v_accvgpr_write_b32 a1, v2"])]})
    assert macros == [] and fatal == [sym]


def test_eval_macros_reach_the_kernel_source():
    """Every macro the guard can define for k_eval_w guards an instantiation
    and is honoured by the launcher."""
    text = open(os.path.join(REPO, "dgen_amd", "csrc", "dgen_hip.hip")).read()
    for macro in ("DGEN_NO2_EVAL", "DGEN_NO2_EVAL_DC", "DGEN_NO2_EVAL_PK"):
        assert macro in spill_guard.REMEDY.values()
        assert len(re.findall(r"#if !" + macro + r"\b", text)) == 2, macro


def test_size_grid_is_rel_times_base():
    base = np.array([2.0, 3.5, 10.0])
    xs = sensitivity.size_grid(base, (0.5, 1.0, 1.5, 2.0))
    assert xs.shape == (4, 3) and xs.dtype == np.float64
    for k, r in enumerate((0.5, 1.0, 1.5, 2.0)):
        assert np.array_equal(xs[k], r * base)
    assert sensitivity.size_grid(base).shape == (len(sensitivity.DEFAULT_REL), 3)
    assert sensitivity.DEFAULT_REL[0] == 0.5 and sensitivity.DEFAULT_REL[-1] == 1.5
    with pytest.raises(ValueError):
        sensitivity.size_grid(base, ())
    with pytest.raises(ValueError):
        sensitivity.size_grid(base, np.ones(_lib.CURVE_MAX_POINTS + 1))


def test_order_mapping_round_trips():
    perm = np.array([3, 0, 4, 1, 2])                 # device row j holds caller agent perm[j]
    caller = np.arange(10.0).reshape(2, 5)
    dev = sensitivity.to_device_order(caller, perm)
    assert np.array_equal(dev[:, 0], caller[:, 3]) and np.array_equal(dev[:, 2], caller[:, 4])
    assert np.array_equal(sensitivity.to_caller_order(dev, perm), caller)
    assert sensitivity.to_device_order(caller, None) is caller
    assert sensitivity.to_caller_order(dev, None) is dev
    one = np.array([10.0, 11.0, 12.0, 13.0, 14.0])
    assert np.array_equal(sensitivity.to_caller_order(sensitivity.to_device_order(one, perm), perm), one)


def test_fixed_kw_values_name_the_bad_agent():
    import pandas as pd
    from dgen_amd.financial_functions import _fixed_kw_values
    df = pd.DataFrame({"agent_id": [11, 12, 13], "kw_given": [4.0, 5.5, 7.0]})
    assert np.array_equal(_fixed_kw_values(df, "kw_given"), [4.0, 5.5, 7.0])
    assert np.array_equal(_fixed_kw_values(df, np.array([1.0, 2.0, 3.0])), [1.0, 2.0, 3.0])
    for bad in (np.nan, 0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="agent 12"):
            _fixed_kw_values(df, [4.0, bad, 7.0])
    with pytest.raises(ValueError):
        _fixed_kw_values(df, [1.0, 2.0])
    with pytest.raises(KeyError):
        _fixed_kw_values(df, "no_such_column")
