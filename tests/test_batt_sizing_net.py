"""Battery size what-if under net billing, host side: curve_ref
(tests/test_batt_sizing) on net-billing agents against Population.run at the
reference's point -- the checker the device entry dgen_batt_curve_net is held
to -- and the Python plumbing of net= / "net_billing" on hand-made curves."""
import ctypes

import numpy as np
import pytest

from dgen_amd import _lib
from dgen_amd import batt_sizing as bs
from dgen_amd.synth import make_population
from oracle import oracle as orc
from tests.test_batt_sizing import _opop, curve_ref


@pytest.mark.parametrize("config,seed", [("ca_res_storage", 20260021), ("metering_mix", 20260023)])
def test_curve_ref_reproduces_the_driver_on_net_billing_agents(config, seed):
    """16 agents each: at (kW* / 0.8, kW* / 0.8 / 2) curve_ref is the driver's
    PV+battery run bit for bit where the final tariff bills hourly imports
    (options 2 and 3, the TS sell rate included), from the sticky state."""
    pop = make_population(config, 16, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16,
                          n_tariffs=48)
    opop, cfg = _opop(pop), orc.make_cfg()
    ref = opop.run(cfg)
    n_net = n_ts = 0
    for i, r in enumerate(ref):
        if r["status"] != 0:
            continue
        t = opop.tariffs[r["tariff_final"]]
        if t.mo not in (2, 3):
            continue
        n_net += 1
        a = opop.agents[i]
        n_ts += int(t.mo == 2 and not a.is_ca and bool(a.wholesale))
        kw = r["system_kw"]
        e = kw / 0.8
        c = curve_ref(opop, cfg, i, kw, r["tariff_final"], r["switched"], e, e / 2.0)
        assert c["npv"] == r["npv_pv_batt"], (i, c["npv"], r["npv_pv_batt"])
        assert np.array_equal(c["bill_w"], r["bill_w_pv_batt"]) and np.array_equal(c["bill_wo"], r["bill_wo_pv_batt"])
        assert c["bank_kwh"] == r["batt_kwh"] and c["power_kw"] == r["batt_kw"]
        assert c["tariff"] == r["tariff_final"] and c["switched"] == r["switched"]
    print(f"{config}: {n_net} net-billing agents of {len(ref)}, {n_ts} on the TS sell rate")
    assert n_net >= (16 if config == "ca_res_storage" else 2)


# ---- host plumbing ----------------------------------------------------------
class _Batch:
    perm = None

    def __init__(self, n):
        self.n = n


class _FakeEngine:
    """Engine.batt_curve's signature over a hand-made curve: agent 1's points
    are flagged ST_HOURLY_FORM unless net=True."""

    def __init__(self):
        self.calls = []

    def _to_dev(self, a, dtype):
        import torch
        return torch.as_tensor(np.asarray(a)).to(dtype)

    def batt_curve(self, batch, out, kwh, kw=None, want=None, net=False, net_cap=None):
        import torch
        self.calls.append({"net": net, "net_cap": net_cap, "K": int(kwh.shape[0])})
        K, n = kwh.shape
        npv = torch.arange(K * n, dtype=torch.float64).view(K, n)
        st = torch.zeros((K, n), dtype=torch.int32)
        if not net:
            st[:, 1] = _lib.ST_HOURLY_FORM
            npv[:, 1] = float("nan")
        d = {"npv": npv, "payback_raw": npv * 0.5, "bank_kwh": kwh.clone(), "power_kw": kwh / 2.0, "status": st,
             "total_cost": npv, "bill_w_year1": npv, "bill_wo_year1": npv, "lifetime_savings": npv,
             "tariff": st, "switched": st}
        return {k: d[k] for k in (want or _lib.BATT_CURVE_FIELDS)}


def test_grid_accepts_the_net_billing_key():
    assert bs.grid({"hours": [1, 4], "net_billing": True}) == ((0.8,), (1, 4))
    assert bs.grid({"net_billing": False}) == ((bs.REF_PV_TO_BATT,), (bs.REF_HOURS,))
    assert bs.net_billing({"net_billing": True}) and not bs.net_billing({"hours": [1]})
    assert not bs.net_billing(True) and not bs.net_billing(([0.8], [2.0])) and not bs.net_billing({"net_billing": 0})
    with pytest.raises(ValueError):
        bs.grid({"net_biling": True})


def test_net_is_threaded_to_the_engine_and_fills_the_flagged_agent():
    torch = pytest.importorskip("torch")
    eng, batch = _FakeEngine(), _Batch(3)
    out = {"system_kw": torch.tensor([4.0, 7.3, 2.0], dtype=torch.float64)}
    off = bs.annual_columns(eng, batch, out, {"pv_to_batt": (0.4, 1.6)})
    on = bs.annual_columns(eng, batch, out, {"pv_to_batt": (0.4, 1.6), "net_billing": True})
    assert [c["net"] for c in eng.calls] == [False, True] and all(c["K"] == 3 for c in eng.calls)
    assert all(c["net_cap"] is None for c in eng.calls)
    assert off["batt_opt_point"].tolist() == [2, -1, 2] and on["batt_opt_point"].tolist() == [2, 2, 2]
    assert off["batt_opt_status"][1] == _lib.ST_HOURLY_FORM and on["batt_opt_status"][1] == 0
    assert np.isnan(off["batt_opt_npv"][1]) and on["batt_opt_npv"][1] == 7.0
    for k in bs.COLUMNS:                        # the other agents' columns do not move
        assert np.array_equal(off[k][[0, 2]], on[k][[0, 2]]), k
    kwh = np.ones((2, 3))
    bs.curve_outputs(eng, batch, out, kwh)
    bs.curve_outputs(eng, batch, out, kwh, net=True)
    bs.curve_outputs(eng, batch, out, kwh, net=True, net_cap=7)
    assert [(c["net"], c["net_cap"]) for c in eng.calls[2:]] == [(False, None), (True, None), (True, 7)]


def test_an_engine_without_the_keyword_still_serves_the_default_call():
    """Without net the call carries no new keyword (a caller's stand-in for
    Engine.batt_curve with the earlier signature keeps working)."""
    torch = pytest.importorskip("torch")

    class Old:
        _to_dev = _FakeEngine._to_dev

        def batt_curve(self, batch, out, kwh, kw=None, want=None):
            return _FakeEngine().batt_curve(batch, out, kwh, kw, want)

    out = {"system_kw": torch.tensor([4.0, 7.3], dtype=torch.float64)}
    s = bs.annual_columns(Old(), _Batch(2), out, True)
    assert s["batt_opt_point"].tolist() == [9, -1]
    with pytest.raises(TypeError):
        bs.annual_columns(Old(), _Batch(2), out, {"net_billing": True})


def test_abi_binding_is_declared():
    assert "dgen_batt_curve_net" in _lib.EXPORTED
    assert [n for n, _ in _lib.BattNetOpt._fields_] == ["cap", "pad"] and ctypes.sizeof(_lib.BattNetOpt) == 8
    assert _lib.NB_CAPM == 192
    import inspect
    from dgen_amd.engine import Engine
    p = inspect.signature(Engine.batt_curve).parameters
    assert p["net"].default is False and p["net_cap"].default is None
    with open(_lib._build.HDR) as f:
        hdr = f.read()
    assert "int32_t dgen_batt_curve_net(" in hdr and "dgen_batt_net_opt" in hdr
    assert f"#define DGEN_NB_CAPM {_lib.NB_CAPM}" in hdr
