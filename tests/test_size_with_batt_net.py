"""The net-billing fill-in of the PV search on the with-battery objective, host
side: the binding and its option struct against the header, the drop-in
switch's further spec keys, and Engine.size_with_batt's keywords."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dgen_hip.h")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "dgen_hip.h"
int main(void) {
  printf("size %zu\n", sizeof(dgen_swb_net_opt));
  printf("cap %zu\n", offsetof(dgen_swb_net_opt, cap));
  printf("max_blocks %zu\n", offsetof(dgen_swb_net_opt, max_blocks));
  printf("capm %d\n", DGEN_NB_CAPM);
  printf("abi %d\n", DGEN_ABI_VERSION);
  return 0;
}
"""


def test_the_binding_is_declared():
    text = open(HEADER).read()
    assert re.search(r"^int32_t\s+dgen_size_with_batt_net\s*\(", text, flags=re.M)
    assert "dgen_size_with_batt_net" in _lib.EXPORTED
    L = _lib.load(build_if_missing=True)
    fn = L.dgen_size_with_batt_net
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 10
    assert len(L.dgen_size_with_batt.argtypes) == 9          # the first call's prototype is as it was
    assert L.dgen_abi_version() == _lib.ABI_VERSION == 14


def test_option_struct_matches_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert lay["size"] == ctypes.sizeof(_lib.SwbNetOpt) == 8
    assert lay["cap"] == _lib.SwbNetOpt.cap.offset == 0
    assert lay["max_blocks"] == _lib.SwbNetOpt.max_blocks.offset == 4
    assert lay["capm"] == _lib.NB_CAPM and lay["abi"] == 14


def test_spec_keys():
    # the pair is what it was, whatever the net keys say
    assert bs.co_size_spec({"net_billing": True}) == (0.8, 2.0)
    assert bs.co_size_spec({"ratio": 0.4, "hours": 4.0, "net_billing": True, "net_cap": 8, "net_blocks": 2}) == (0.4, 4.0)
    # without net billing the engine sees the call it always saw
    for spec in (True, {}, {"ratio": 0.4}, {"net_billing": False}, {"net_billing": False, "net_cap": 4}):
        assert bs.co_size_options(spec) == {}, spec
    assert bs.co_size_options({"net_billing": True}) == {"net": True}
    assert bs.co_size_options({"net_billing": True, "net_cap": None, "net_blocks": None}) == {"net": True}
    assert bs.co_size_options({"net_billing": True, "net_cap": 1}) == {"net": True, "net_cap": 1}
    assert bs.co_size_options({"net_billing": True, "net_cap": _lib.NB_CAPM, "net_blocks": 3}) == \
        {"net": True, "net_cap": _lib.NB_CAPM, "net_blocks": 3}
    for bad in ({"net_billing": 1}, {"net_billing": "yes"}, {"net_billing": None},
                {"net_billing": True, "net_cap": 0}, {"net_billing": True, "net_cap": -1},
                {"net_billing": True, "net_cap": _lib.NB_CAPM + 1}, {"net_billing": True, "net_cap": 8.0},
                {"net_billing": True, "net_cap": True}, {"net_billing": True, "net_blocks": 0},
                {"net_billing": True, "net_blocks": "2"}, {"net_billing": False, "net_cap": 0},
                {"net_billing": True, "net": True}, {"net_billing": True, "ratio": 0.0}, False, None, 1):
        with pytest.raises(ValueError):
            bs.co_size_options(bad)
    for bad in ({"net": True}, {"net_billing": True, "cap": 4}, {"peak_billing": True}):
        with pytest.raises(ValueError, match="unknown keys"):
            bs.co_size_spec(bad)


def test_engine_keywords():
    from dgen_amd.engine import Engine
    p = inspect.signature(Engine.size_with_batt).parameters
    assert p["net"].default is False and p["net_cap"].default is None and p["net_blocks"].default is None
    assert list(p)[:8] == ["self", "batch", "ratio", "hours", "lo", "hi", "trace", "want"]     # positional order kept
