"""The battery dispatch kernels on constructed edge days (tests/dispatch_refs.py:
dark days, days without a deficit, tied deficits, spikes above the power limit,
a largest deficit that brackets it, zero-load hours), in waves whose lanes sit
on different patterns on every calendar day: the scan (k_hourly_batt, every
form) against the oracle at the fp64 planes' bound, holes in a wave, the launch
shape, and the replay at caller-given banks.  Which branch each day reaches is
shown on the CPU, from the reference alone (tests/test_dispatch_refs.py)."""
import numpy as np
import pytest
import torch

from dgen_amd import _lib
from dgen_amd.engine import hourly_agent_major, outputs_to_host
from oracle import oracle as orc
from tests import dispatch_refs as dr
from tests import helpers

pytestmark = pytest.mark.gpu

N_ALL = (1, 63, 64, 65, 130)
FORMS = {"daily": {}, "hourly": {"batt_update_hours": 1},
         "daily-floor": {"batt_month_floor": 1}, "hourly-floor": {"batt_month_floor": 1, "batt_update_hours": 1},
         "daily-loss": {"batt_loss_model": 1, "batt_r_cell": 0.02},
         "hourly-loss": {"batt_loss_model": 1, "batt_r_cell": 0.02, "batt_update_hours": 1}}
CASES = ([("daily", "res_1m_nem_tou", n) for n in N_ALL] + [("daily", "ca_res_storage", 130),
         ("hourly", "res_1m_nem_tou", 65), ("hourly", "ca_res_storage", 65)] +
         [(f, "res_1m_nem_tou", 65) for f in list(FORMS)[2:]])


def _load(eng, pop, order):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs)
    eng.set_switches(pop.switches)
    return eng.upload_agents(pop.cols, pop.n_scratch, order=order)


def _evaluate(eng, batch, kw, f64=True):
    """kw in caller order; the outputs come back in caller order."""
    out = eng.alloc_outputs(batch.n, hourly=True, hourly_f64=f64)
    eng.evaluate(batch, out, kw[batch.perm])
    torch.cuda.synchronize()
    return out


def _pattern_at(pop, i, h):
    row = int(pop.cols["load_row"][i])
    return dr.PATTERNS[dr.edge_tables()[2][row, h // 24]] if row < dr.NP else "synthetic"


def _check_against_oracle(o, pop, kw, cfg_o, what):
    """The planes at 1e-12 x max(1, |ref| max) (test_hourly_f64_planes' bound),
    the battery scalars and yearly arrays at check_sized_against_oracle's
    tolerances.  Returns the worst plane ratio."""
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale)
    worst = 0.0
    for i in range(len(kw)):
        r = opop.eval_at(cfg_o, i, kw[i], kw[i], int(pop.cols["tariff0"][i]), 0, hourly=True)
        assert o["status"][i] == 0 and r["status"] == 0, (what, i)
        for k_o, k_r in (("net_pvonly", "adopter_net_hourly_pvonly"), ("net_with_batt", "adopter_net_hourly_with_batt")):
            ref = np.asarray(r[k_r], float)
            err = np.abs(o[k_o][i] - ref)
            scale = max(1.0, float(np.abs(ref).max()))
            worst = max(worst, float(err.max()) / scale)
            h = int(err.argmax())
            assert err.max() <= 1e-12 * scale, (what, i, k_o, float(err.max()) / scale, "hour", h, "day", h // 24,
                                                 "pattern", _pattern_at(pop, i, h))
        for k in ("batt_kwh", "batt_kw", "npv_pv_batt"):
            assert np.isclose(o[k][i], r[k], rtol=1e-6, atol=1e-6), (what, i, k, o[k][i], r[k])
        N1 = int(pop.cols["econ_life"][i]) + 1
        for k_o, k_r in (("cfev_batt", "cf_energy_value_pv_batt"), ("bill_w_batt", "bill_w_pv_batt")):
            assert np.allclose(o[k_o][i, :N1], r[k_r], rtol=1e-6, atol=1e-5), (what, i, k_o)
    return worst


@pytest.mark.parametrize("form,config,n", CASES, ids=[f"{f}-{c}-{n}" for f, c, n in CASES])
def test_scan_matches_oracle_on_edge_days(engine, engine_hourly_plan, form, config, n):
    """Engine.evaluate (k_eval_w, k_hourly_batt, k_batt_finance_w; no search)
    against orc_eval_at per agent; the float32 planes are the float64 planes
    rounded, bit for bit.

    Measured worst plane ratios on one MI355X: daily 5.7e-16, hourly 3.9e-16,
    daily-floor 8.3e-15, hourly-floor 2.3e-15, daily-loss 6.8e-16, hourly-loss
    5.6e-16.

    hourly-floor found a discontinuity of the rule (agent 11, hour 1416: 1.1e-2
    of the plane's maximum): the re-plan planned only where avail > 0, and a
    plan made on rounding dust of stored energy raised the month floor to the
    window's largest deficit while avail = 0 did not; the device forms the
    load one rounding away from the oracle's, enough to flip the dust.  Under
    the floor every deficit hour now plans (oracle and kernel alike)."""
    from dgen_amd.config import EngineConfig
    from dgen_amd.engine import Engine
    pop, kw, order = dr.edge_population(config, n)
    own = form not in ("daily", "hourly")
    eng = Engine(0, EngineConfig(**FORMS[form])) if own else (engine if form == "daily" else engine_hourly_plan)
    try:
        batch = _load(eng, pop, order)
        o64 = _evaluate(eng, batch, kw, True)
        o32 = _evaluate(eng, batch, kw, False)
        for k in ("baseline", "net_pvonly", "net_with_batt"):
            assert o64[k].dtype == torch.float64 and torch.equal(o64[k].to(torch.float32), o32[k]), k
        o = outputs_to_host(o64, batch.perm)
        if "hourly" in form or "loss" in form:   # replay_at has the daily plan without the loss model only
            with pytest.raises(_lib.DgenError):
                eng.replay_at(batch, kw[batch.perm], kw[batch.perm] / 0.8, None, planes="f64")
        else:
            eng.replay_at(batch, kw[batch.perm], kw[batch.perm] / 0.8, None, want=(), planes="f64")
            torch.cuda.synchronize()
    finally:
        if own:
            eng.close()
    worst = _check_against_oracle(o, pop, kw, orc.make_cfg(**FORMS[form]), (form, config, n))
    print(f"{form} {config} n={n}: worst plane ratio {worst:.3e}")


def test_holes_in_a_wave(engine):
    """Every seventh agent of the 130 gets a size dgen_eval_agents flags
    DGEN_ST_BOUNDS (NaN, 0, -1: test_gpu_evaluate.py's contract); every other
    agent is bit-identical to its run in the batch without holes."""
    pop, kw, order = dr.edge_population("res_1m_nem_tou", 130)
    batch = _load(engine, pop, order)
    ref = outputs_to_host(_evaluate(engine, batch, kw), batch.perm)
    bad = np.zeros(130, bool)
    bad[batch.perm[::7]] = True                  # every seventh lane of the device order
    kw2 = kw.copy()
    kw2[bad] = np.resize([np.nan, 0.0, -1.0], int(bad.sum()))
    o = outputs_to_host(_evaluate(engine, batch, kw2), batch.perm)
    assert ((o["status"][bad] & _lib.ST_BOUNDS) != 0).all() and (o["nfev"][bad] == 0).all()
    assert np.isnan(o["npv"][bad]).all() and np.isnan(o["system_kw"][bad]).all()
    for k, v in o.items():
        if v is not None:
            assert np.array_equal(v[~bad], ref[k][~bad], equal_nan=True), k


def test_tiny_and_huge_banks_share_a_wave(engine):
    """One wave on one row (the staircase's), neighbouring lanes at PV sizes a
    factor 50 apart: a bank whose power limit is below most deficits beside one
    that covers most days' whole need."""
    pop, _, _ = dr.edge_population("res_1m_nem_tou", 64)
    row = dr.PATTERNS.index("staircase")
    ssum = float(np.sum(pop.shapes[row].astype(np.float64)))
    pop.cols["load_row"][:] = row
    pop.cols["cf_row"][:] = row
    pop.cols["load_kwh"][:] = ssum * (1.0 + 0.01 * np.arange(64))
    kw = np.where(np.arange(64) % 2 == 0, 0.4, 20.0)
    load, pv = dr.agent_hours(pop.cols["load_row"], pop.cols["cf_row"], pop.cols["load_kwh"], kw)
    bp = np.array([dr.reference_bank(k) for k in kw])
    lab = dr.classify_days(load, pv, bp[:, 0], bp[:, 1], orc.make_cfg())["label"]
    # the small bank's power limit binds on most days, the large bank's on few
    assert np.isin(lab[0::2], dr.SATURATED).mean() > 0.5 and np.isin(lab[1::2], (dr.FITS, dr.UNSAT)).mean() > 0.5
    batch = _load(engine, pop, np.arange(64))
    o = outputs_to_host(_evaluate(engine, batch, kw), batch.perm)
    worst = _check_against_oracle(o, pop, kw, orc.make_cfg(), "tiny / huge")
    print(f"tiny / huge banks in one wave: worst plane ratio {worst:.3e}")


@pytest.mark.parametrize("config", ["res_1m_nem_tou", "ca_res_storage"])
def test_launch_shape_is_invisible_on_edge_days(engine, engine_hourly_plan, config):
    """set_hourly_segment(1 / 5 / 12) changes no output bit, and the scan's
    planes are replay_at's at the bank the scan reports, bit for bit;
    replay_at refuses the hourly re-plan (and the loss model:
    test_scan_matches_oracle_on_edge_days tries it on every engine it opens)."""
    pop, kw, order = dr.edge_population(config, 130)
    batch = _load(engine, pop, order)
    res = []
    try:
        for months in (12, 1, 5):
            engine.set_hourly_segment(months)
            res.append(_evaluate(engine, batch, kw))
    finally:
        engine.set_hourly_segment(_lib.DEFAULT_HOURLY_MONTHS)
    host = [outputs_to_host(r) for r in res]
    for k in ("baseline", "net_pvonly", "net_with_batt", "npv_pv_batt", "batt_kwh"):
        assert np.isfinite(host[0][k]).all(), k
    for h in host[1:]:
        for k, v in h.items():
            if v is not None:                    # NaN equals NaN only
                assert np.array_equal(v, host[0][k], equal_nan=True), k
    out = res[0]
    got = engine.replay_at(batch, kw[batch.perm], out["batt_kwh"], out["batt_kw"], want=(), planes="f64")
    torch.cuda.synchronize()
    assert not got["status"].any().item()
    assert torch.equal(got["bank_kwh"], out["batt_kwh"]) and torch.equal(got["power_kw"], out["batt_kw"])
    for k, k_o in (("baseline", "baseline"), ("pvonly", "net_pvonly"), ("with_batt", "net_with_batt")):
        assert torch.equal(got[k], out[k_o]), k
    b2 = _load(engine_hourly_plan, pop, order)
    with pytest.raises(_lib.DgenError):
        engine_hourly_plan.replay_at(b2, kw[b2.perm], kw / 0.8, None, planes="f64")


@pytest.mark.parametrize("shift", dr.REPLAY_SHIFTS)
def test_replay_at_caller_given_banks(engine, shift):
    """replay_at on the constructed rows with banks {none, one string, the
    reference's, three times it} at 1 and 4 hours, mixed within each wave
    (dispatch_refs.replay_banks): the with-battery plane against the oracle's
    dispatch, the kWh and SOC members against summary_ref, the hour counts
    under tests/test_gpu_replay_at.py's ambiguity rule, which may leave out at
    most 10 % of the agents (tests/test_dispatch_refs.py shows the reference
    alone stays inside that)."""
    from tests.test_batt_metrics import summary_ref
    from tests.test_gpu_replay_at import ATOL, FLOW_COUNTS, MEMBERS, PLANE_RTOL, RTOL, _ambiguous, _bound_arrivals
    n = 130
    pop, kw, order = dr.edge_population("res_1m_nem_tou", n)
    a = dr.edge_agents(n)
    kwh, pkw = dr.replay_banks(a, shift)
    batch = _load(engine, pop, order)
    p = batch.perm
    d = engine.replay_at(batch, kw[p], kwh[p], pkw[p], planes="f64")
    torch.cuda.synchronize()
    inv = np.argsort(p)
    wb = hourly_agent_major(d["with_batt"]).cpu().numpy()[inv]
    dev = {k: d[k].cpu().numpy()[..., inv] for k in MEMBERS + ["bank_kwh", "power_kw", "status"]}
    assert not dev["status"].any()
    cfg_o = orc.make_cfg()
    load, pv = dr.agent_hours(a["load_row"], a["cf_row"], a["load_kwh"], kw)
    amb = np.zeros(n, bool)
    und = np.zeros((2, 12, n), np.int64)
    ref = {k: np.zeros((12, n), np.float64 if k in _lib.BATT_SUMMARY_F64 else np.int32) for k in MEMBERS}
    worst = {"plane": 0.0}
    tol = PLANE_RTOL[torch.float64]
    for i in range(n):
        bank, power = (0.0, 0.0) if kwh[i] == 0.0 else orc.batt_size(pkw[i], kwh[i], 240.0, cfg_o)
        assert dev["bank_kwh"][i] == bank and abs(dev["power_kw"][i] - power) <= 1e-12 * power
        r = summary_ref(load[i], pv[i], bank, power, cfg_o)
        for k in MEMBERS:
            ref[k][:, i] = r[k]
        amb[i] = _ambiguous(r["_hours"], power, cfg_o)
        und[:, :, i] = _bound_arrivals(r["_hours"], bank, cfg_o)
        sg, _ = orc.batt_dispatch(load[i], pv[i], bank, power, cfg_o)
        want = np.maximum(load[i] - sg, 0.0)
        scale = max(1.0, float(np.abs(want).max()))
        err = np.abs(wb[i] - want)
        worst["plane"] = max(worst["plane"], float(err.max()) / scale)
        h = int(err.argmax())
        assert np.allclose(wb[i], want, rtol=tol, atol=tol * scale), (shift, i, float(err.max()), _pattern_at(pop, i, h))
    assert amb.sum() <= dr.REPLAY_LEFT_OUT_CAP * n, int(amb.sum())
    keep = ~amb
    for k in _lib.BATT_SUMMARY_F64:
        err = np.abs(dev[k] - ref[k])
        if k.startswith("soc"):
            assert np.allclose(dev[k], ref[k], rtol=0.0, atol=ATOL), (shift, k, float(err.max()))
        else:
            worst[k] = float((err / np.maximum(np.abs(ref[k]), 1.0)).max())
            assert np.allclose(dev[k], ref[k], rtol=RTOL, atol=ATOL), (shift, k, float(err.max()))
    for k in _lib.BATT_SUMMARY_I32:
        if k in FLOW_COUNTS:
            gap = np.abs(dev[k].astype(np.int64) - ref[k])[:, keep]
            room = und[FLOW_COUNTS.index(k)][:, keep]
            print(f"shift {shift} {k}: hours excused {int(gap.sum())}, moments at the bound {int(room.sum())}")
            assert (gap <= room).all(), (shift, k, int(gap.max()))
            assert gap.sum() * 100 <= room.sum(), (shift, k, int(gap.sum()), int(room.sum()))
        else:
            assert np.array_equal(dev[k][:, keep], ref[k][:, keep]), (shift, k)
    print(f"shift {shift}: agents left out {int(amb.sum())} of {n}; worst " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
