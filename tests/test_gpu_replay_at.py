"""Dispatch replay at a caller-given PV size and bank on the GPU
(dgen_replay_at): at the reference's bank it is dgen_batt_summary and the
evaluation's hourly planes bit for bit; at other banks it agrees with the
oracle's dispatch (tests/test_batt_metrics.summary_ref) within the project's
tolerances; its members and planes are consistent with each other bit for bit;
an agent's bits do not depend on its batch or on what else was asked for; a
flagged row gets zeros and disturbs nobody; and the drop-in switches' "dispatch"
key reports the replay at the chosen point.  Populations are dgen_amd.synth's
at n in {1, 63, 64, 65, 257}: the tile address depends on n, 63 / 65 straddle
a wave."""
import ctypes

import numpy as np
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import batt_metrics as bm
from dgen_amd import batt_sizing as bs
from dgen_amd import financial_functions as ff
from dgen_amd.config import EngineConfig
from dgen_amd.engine import hourly_agent_major
from dgen_amd.synth import make_population, subset
from oracle import oracle as orc
from tests.test_batt_metrics import summary_ref

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-6               # the project's tolerances: 1e-6 relative on energy, 1e-6 absolute on fractions
PLANE_RTOL = {torch.float64: 1e-6, torch.float32: 2e-6}
N_ALL = (1, 63, 64, 65, 257)
RES_SEED, COM_SEED = 20260003, 20260007      # tests/test_gpu_batt_summary.py's populations
MEMBERS = _lib.BATT_SUMMARY_FIELDS
PLANES = _lib.REPLAY_PLANES
OUT_PLANE = {"baseline": "baseline", "pvonly": "net_pvonly", "with_batt": "net_with_batt"}


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


def _load(eng, pop):
    eng.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    eng.set_tariffs(pop.tariffs)
    eng.set_switches(pop.switches)


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _sizes(pop):
    """A PV size per agent from its own columns (no sizing call): the year's
    load over 1400 full-load hours, scaled 0.4 .. 1.4 -- midday surplus and
    evening deficit in every agent."""
    n = pop.cols["load_kwh"].size
    f = 0.4 + (np.arange(n) % 11) / 10.0
    return pop.cols["load_kwh"].astype(np.float64) / 1400.0 * f


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def res_pop():
    return _pop("res_1m_nem_tou", max(N_ALL), RES_SEED)


@pytest.fixture(scope="module")
def res_case(engine, res_pop):
    """The 257 residential agents replayed once at an off-reference bank (1.2
    kWh per kW at 4 h), summary and fp64 planes: the bits the independence,
    consistency and flag tests compare with."""
    _load(engine, res_pop)
    batch = engine.upload_agents(res_pop.cols, res_pop.n_scratch)
    assert batch.perm is None
    kw = _sizes(res_pop)
    kwh = kw * 1.2
    d = engine.replay_at(batch, kw, kwh, kwh / 4.0, planes="f64")
    torch.cuda.synchronize()
    assert not d["status"].any().item() and (d["bank_kwh"] > 0).all().item()
    return {"batch": batch, "kw": kw, "kwh": kwh, "pkw": kwh / 4.0, "d": d}


@pytest.fixture(scope="module")
def engine_floor():
    from dgen_amd.engine import Engine
    eng = Engine(0, EngineConfig(batt_month_floor=1))
    yield eng
    eng.close()


# ---------------------------------------------------------------------------
# 1. at the reference's bank: the existing calls, bit for bit
# ---------------------------------------------------------------------------
CASES = [("res", n) for n in N_ALL] + [("com", 64), ("floor", 65), ("off", 65)]


@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}{n}" for k, n in CASES])
def test_replay_equals_the_existing_calls_at_the_reference_bank(engine, engine_floor, res_pop, kind, n):
    """Engine.evaluate at kw, then batt_summary and the three planes of that
    evaluation, against replay_at(kw, kw / 0.8, kw / 0.8 / 2): array_equal in
    every member and plane, fp64 and fp32."""
    eng = engine_floor if kind == "floor" else engine
    if kind == "com":
        pop = _pop("com_8m", 64, COM_SEED)
        assert not (pop.cols["flags"] & 1).any()          # 500 V banks
        sub = pop
    else:
        pop, sub = res_pop, subset(res_pop, np.arange(n))
    _load(eng, pop)
    if kind == "off":
        eng.set_battery(False)
    try:
        batch = eng.upload_agents(sub.cols, sub.n_scratch)
        kw = _sizes(sub)
        kwh = kw / 0.8
        for f64, planes in ((True, "f64"), (False, "f32")):
            out = eng.alloc_outputs(batch.n, hourly=True, hourly_f64=f64)
            eng.evaluate(batch, out, kw)
            ref = eng.batt_summary(batch, out)
            got = eng.replay_at(batch, kw, kwh, kwh / 2.0, planes=planes)
            two = eng.replay_at(batch, kw, kwh, None, planes=planes)       # NULL bank_kw: the 2-hour bank
            torch.cuda.synchronize()
            st = out["status"].cpu().numpy()
            assert ((st & (_lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_UNIT)) == 0).all()
            assert np.array_equal(out["system_kw"].cpu().numpy(), kw)
            assert not got["status"].any().item()
            for k in MEMBERS:
                assert got[k].shape == (12, n) and torch.equal(got[k], ref[k]), (kind, n, planes, k)
            for k in PLANES:
                assert got[k].dtype == out[OUT_PLANE[k]].dtype and got[k].shape == (_lib.NH // 4, n, 4)
                assert torch.equal(got[k], out[OUT_PLANE[k]]), (kind, n, planes, k)
            assert torch.equal(got["bank_kwh"], out["batt_kwh"]) and torch.equal(got["power_kw"], out["batt_kw"])
            _same(got, two, (kind, n, planes, "bank_kw None"))
            if kind == "off":
                assert not got["bank_kwh"].any().item() and not got["batt_to_load_kwh"].any().item()
                assert torch.equal(got["with_batt"], got["pvonly"])
            else:
                assert (got["bank_kwh"] > 0).all().item() and (got["batt_to_load_kwh"].sum(0) > 0).all().item()
    finally:
        if kind == "off":
            eng.set_battery(True)


# ---------------------------------------------------------------------------
# 2. at other banks: the oracle
# ---------------------------------------------------------------------------
N_ORC = 65
DURATIONS = (1.0, 2.0, 4.0)


def _string_kwh(cfg_o, volts):
    return cfg_o.batt_q_full * cfg_o.batt_v_nom * np.ceil(volts / cfg_o.batt_v_nom) * 0.001


def _agent_hours(pop, i, kw, ssum):
    """load and pv of agent i at kw, formed as the header defines them."""
    c = pop.cols
    lr, cr = int(c["load_row"][i]), int(c["cf_row"][i])
    ls = float(c["load_kwh"][i]) / float(ssum[lr])
    cs6 = (((float(kw) * 1000.0) * 0.96) / 1000.0) / 1e6
    return pop.shapes[lr].astype(np.float64) * ls, pop.cfs[cr].astype(np.float64) * cs6


def _ambiguous(h, power, cfg_o):
    """tests/test_gpu_batt_summary.py's band rule: the reference puts some
    hour's tested quantity within 1 % of a band's width of its threshold, so
    rounding decides the hour's count."""
    return bool(np.abs(h["soc"] - (cfg_o.batt_max_soc - 1e-9)).min() <= 1e-11
                or np.abs(h["soc"] - (cfg_o.batt_min_soc + 1e-9)).min() <= 1e-11
                or np.abs(h["sur"] - 1e-6).min() <= 1e-8 or np.abs(h["sur"] - (power + 1e-6)).min() <= 1e-8
                or np.abs(h["nn"] - 1e-6).min() <= 1e-8
                or (power > 0.0 and np.abs(h["d"] - power * (1.0 - 1e-9)).min() <= 1e-11 * power))


FLOW_COUNTS = ("hours_charge", "hours_discharge")


def _bound_arrivals(h, bank, cfg_o):
    """[2][12]: per month the moments the reference's bank becomes full /
    becomes empty: hours that end within 1e-11 of batt_max_soc (batt_min_soc)
    and did not start there.  They bound what can flip in the two flow counts,
    which have no band of their own.  A charge clamped by the room left (a
    discharge clamped by the energy left) lands the SOC on the bound up to
    rounding; the next surplus (deficit) hour then sees a room of 0 or of
    rounding dust, 1e-16 kWh.  Dust is an hour of charge on the device and
    vanishes in the reference's pv - sysgen (tests/test_batt_metrics.py says
    so of its own two paths), and the dust hour puts the SOC on the bound
    exactly, so later hours at the bound have no flow on either path.  One
    hour per arrival can differ, no other.  Measured on one MI355X over the
    11,700 agent-months of the three durations: hours_discharge never differs;
    hours_charge differs by 1 in 13 (11 at the sub-string bank, 2 at 0.25 x,
    all at 1 h)."""
    from tests.test_grid_metrics import MONTH_START
    prev = np.concatenate([[cfg_o.batt_init_soc], h["soc"][:-1]])
    res = []
    for bound in (cfg_o.batt_max_soc, cfg_o.batt_min_soc):
        arrive = (bank > 0.0) & (np.abs(h["soc"] - bound) <= 1e-11) & (np.abs(prev - bound) > 1e-11)
        res.append([int(arrive[MONTH_START[m]:MONTH_START[m + 1]].sum()) for m in range(12)])
    return np.array(res)


@pytest.fixture(scope="module")
def orc_case(engine, res_pop):
    """65 residential agents sized once; the replay's PV size is another one."""
    sub = subset(res_pop, np.arange(N_ORC))
    _load(engine, res_pop)
    batch = engine.upload_agents(sub.cols, sub.n_scratch)
    out = engine.alloc_outputs(batch.n, hourly=False)
    engine.size(batch, out)
    torch.cuda.synchronize()
    sized = out["system_kw"].cpu().numpy()
    assert (out["status"].cpu().numpy() == 0).all() and (sized > 0).all()
    kw = 0.7 * sized + 0.3
    assert (np.abs(kw - sized) > 1e-3).all()
    return {"sub": sub, "batch": batch, "out": out, "kw": kw, "ssum": engine.profile_sums()[0]}


@pytest.mark.parametrize("hours", DURATIONS)
def test_other_banks_match_the_oracle(engine, res_pop, orc_case, hours):
    """Bank kWh in {0, 0.4 of a string (below half: still one string), 0.25 x,
    1 x, 3 x the reference's kW / 0.8} at `hours`: kWh members 1e-6 relative,
    SOC members 1e-6 absolute, hour counts equal on the agents the reference
    does not call ambiguous (at most 1 %, as tests/test_gpu_batt_summary.py
    allows).  hours_charge and hours_discharge, which have no band, are equal
    in every month in which the reference's bank never becomes full (empty),
    and elsewhere differ by at most one hour per such moment
    (_bound_arrivals); the hours so excused are counted and may be no more
    than 1 % of the moments, the share the band rule leaves to rounding.  The
    with-battery plane against max(load - sysgen, 0) of the oracle's dispatch,
    1e-6 (fp64) and 2e-6 (fp32) relative; bank_out and power_out are
    dgen_batt_curve's at the same points, bit for bit, in every row (the curve
    is taken with its net-billing and peak fill-ins, so that no row of it is
    left flagged)."""
    sub, batch, kw, ssum = orc_case["sub"], orc_case["batch"], orc_case["kw"], orc_case["ssum"]
    _load(engine, res_pop)
    cfg_o = orc.make_cfg()
    n = batch.n
    volts = np.where(sub.cols["flags"] & 1, 240.0, 500.0)
    ref_kwh = kw / 0.8
    banks = [np.zeros(n), 0.4 * _string_kwh(cfg_o, volts), 0.25 * ref_kwh, ref_kwh, 3.0 * ref_kwh]
    names = ["none", "sub-string", "0.25x", "1x", "3x"]
    # the installed bank at the same points from the what-if call (evaluated at this kw)
    ev = engine.alloc_outputs(n, hourly=False)
    engine.evaluate(batch, ev, kw)
    kwh_pts = np.stack(banks)
    kw_pts = kwh_pts / hours
    curve = _host(engine.batt_curve(batch, ev, kwh_pts, kw_pts, want=("bank_kwh", "power_kw", "status"),
                                    net=True, peak=True))
    worst = {}
    left_out = 0
    for b, (name, kwh) in enumerate(zip(names, banks)):
        pkw = kwh / hours
        d64 = engine.replay_at(batch, kw, kwh, pkw, planes="f64")
        d32 = engine.replay_at(batch, kw, kwh, pkw, want=(), planes="f32")
        torch.cuda.synchronize()
        wb = {torch.float64: hourly_agent_major(d64["with_batt"]).cpu().numpy(),
              torch.float32: hourly_agent_major(d32["with_batt"]).cpu().numpy().astype(np.float64)}
        dev = _host({k: d64[k] for k in MEMBERS + ["bank_kwh", "power_kw", "status"]})
        assert not dev["status"].any()
        assert ((curve["status"][b] & bs.INVALID) == 0).all(), (name, curve["status"][b])
        assert np.array_equal(dev["bank_kwh"], curve["bank_kwh"][b]), name
        assert np.array_equal(dev["power_kw"], curve["power_kw"][b]), name
        amb = np.zeros(n, bool)
        und = np.zeros((2, 12, n), np.int64)
        ref = {k: np.zeros((12, n), np.float64 if k in _lib.BATT_SUMMARY_F64 else np.int32) for k in MEMBERS}
        for i in range(n):
            load, pv = _agent_hours(sub, i, kw[i], ssum)
            bank, power = (0.0, 0.0) if kwh[i] == 0.0 else orc.batt_size(pkw[i], kwh[i], volts[i], cfg_o)
            assert dev["bank_kwh"][i] == bank and abs(dev["power_kw"][i] - power) <= 1e-12 * power
            if name == "sub-string":
                assert bank == _string_kwh(cfg_o, volts[i])
            r = summary_ref(load, pv, bank, power, cfg_o)
            for k in MEMBERS:
                ref[k][:, i] = r[k]
            amb[i] = _ambiguous(r["_hours"], power, cfg_o)
            und[:, :, i] = _bound_arrivals(r["_hours"], bank, cfg_o)
            sg, _ = orc.batt_dispatch(load, pv, bank, power, cfg_o)
            want = np.maximum(load - sg, 0.0)
            for dt, got in wb.items():
                tol = PLANE_RTOL[dt]
                err = float(np.abs(got[i] - want).max())
                worst[dt] = max(worst.get(dt, 0.0), err / max(1.0, float(np.abs(want).max())))
                assert np.allclose(got[i], want, rtol=tol, atol=tol * max(1.0, float(np.abs(want).max()))), \
                    (name, hours, i, dt, err)
        # the reference alone leaves out no more than tests/test_gpu_batt_summary.py allows (1 % of the agents)
        assert amb.sum() * 100 <= amb.size, (name, hours, int(amb.sum()))
        left_out += int(amb.sum())
        keep = ~amb
        for k in _lib.BATT_SUMMARY_F64:
            err = np.abs(dev[k] - ref[k])
            if k.startswith("soc"):
                worst[k] = max(worst.get(k, 0.0), float(err.max()))
                assert np.allclose(dev[k], ref[k], rtol=0.0, atol=ATOL), (name, hours, k, float(err.max()))
            else:
                worst[k] = max(worst.get(k, 0.0), float((err / np.maximum(np.abs(ref[k]), 1.0)).max()))
                assert np.allclose(dev[k], ref[k], rtol=RTOL, atol=ATOL), (name, hours, k, float(err.max()))
        for k in _lib.BATT_SUMMARY_I32:
            if k in FLOW_COUNTS:
                gap = np.abs(dev[k].astype(np.int64) - ref[k])[:, keep]
                room = und[FLOW_COUNTS.index(k)][:, keep]
                worst[k] = max(worst.get(k, 0), int(gap.max()))
                print(f"{name} {hours} h {k}: agent-months that differ {int((gap > 0).sum())} of {gap.size}, "
                      f"hours excused {int(gap.sum())}, worst {int(gap.max())}; moments the bank arrives at the "
                      f"bound {int(room.sum())}, months without one {int((room == 0).sum())}")
                assert (gap <= room).all(), (name, hours, k, int(gap.max()))
                assert gap.sum() * 100 <= room.sum(), (name, hours, k, int(gap.sum()), int(room.sum()))
            else:
                assert np.array_equal(dev[k][:, keep], ref[k][:, keep]), (name, hours, k)
        if name == "none":
            assert not dev["batt_to_load_kwh"].any() and not dev["hours_charge"].any()
        elif name in ("1x", "3x"):
            assert (dev["batt_to_load_kwh"].sum(0) > 0).all()
    print(f"hours={hours}: agents left out {left_out} of {5 * n}; worst " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items() if k not in FLOW_COUNTS))


# ---------------------------------------------------------------------------
# 3. internal consistency, bit for bit
# ---------------------------------------------------------------------------
def test_members_and_planes_are_consistent(engine, res_pop, res_case):
    _load(engine, res_pop)
    batch, kw, kwh, pkw, d = (res_case[k] for k in ("batch", "kw", "kwh", "pkw", "d"))
    dig = engine.plane_digest(d["with_batt"], want=("import_kwh", "export_kwh"))
    load = engine.plane_digest(d["baseline"], want=("import_kwh",))["import_kwh"]
    torch.cuda.synchronize()
    assert torch.equal(dig["import_kwh"], d["grid_to_load_kwh"]) and not dig["export_kwh"].any().item()
    tot = (d["pv_to_load_kwh"] + d["batt_to_load_kwh"]) + d["grid_to_load_kwh"]
    rel = ((tot - load).abs() / load).max().item()
    print(f"pv + battery + grid to load vs the month's load: worst relative {rel:.2e}")
    assert (load > 0).all().item() and rel <= 1e-12
    # fp32 planes: the float rounding of the fp64 planes
    d32 = engine.replay_at(batch, kw, kwh, pkw, want=(), planes="f32")
    for k in PLANES:
        assert d32[k].dtype == torch.float32 and torch.equal(d32[k], d[k].to(torch.float32)), k
    assert (d["pvonly"] >= 0).all().item() and (d["pvonly"] == 0).any().item()      # the clamp is at work
    assert not torch.equal(d["with_batt"], d["pvonly"])
    # no bank: the with-battery plane is the PV-only plane and nothing flows
    z = engine.replay_at(batch, kw, np.zeros(batch.n), pkw, planes="f64")
    torch.cuda.synchronize()
    assert not z["status"].any().item() and not z["bank_kwh"].any().item() and not z["power_kw"].any().item()
    assert torch.equal(z["with_batt"], z["pvonly"])
    assert torch.equal(z["pvonly"], d["pvonly"]) and torch.equal(z["baseline"], d["baseline"])
    for k in ("pv_to_batt_kwh", "batt_to_load_kwh", "pv_to_batt_mid_kwh", "hours_charge", "hours_discharge",
              "hours_soc_bound", "hours_discharge_power_bound"):
        assert not z[k].any().item(), k
    for k in ("soc_min", "soc_max", "soc_end"):
        assert (z[k] == engine.cfg.batt_init_soc).all().item(), k
    assert torch.equal(z["pv_to_grid_kwh"], z["surplus_kwh"])
    # kw = 0: no PV, the bank never charges
    nopv = engine.replay_at(batch, np.zeros(batch.n), kwh, pkw, planes="f64")
    torch.cuda.synchronize()
    assert not nopv["status"].any().item() and torch.equal(nopv["bank_kwh"], d["bank_kwh"])
    assert not nopv["pv_kwh"].any().item() and not nopv["hours_charge"].any().item()
    assert torch.equal(nopv["pvonly"], nopv["baseline"]) and torch.equal(nopv["baseline"], d["baseline"])


# ---------------------------------------------------------------------------
# 4. independence and determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_an_agent_does_not_depend_on_its_batch(engine, res_pop, res_case, n):
    """Agents 40 .. 40 + n - 1 of the 257 as a batch of their own: the bits
    they have in the 257-agent batch (n = 1: one agent alone)."""
    rows = np.arange(40, 40 + n)
    sub = subset(res_pop, rows)
    _load(engine, res_pop)
    batch = engine.upload_agents(sub.cols, sub.n_scratch)
    d = engine.replay_at(batch, res_case["kw"][rows], res_case["kwh"][rows], res_case["pkw"][rows], planes="f64")
    torch.cuda.synchronize()
    big = res_case["d"]
    ix = torch.as_tensor(rows, device=engine.dev)
    for k, v in d.items():
        assert torch.equal(v, big[k].index_select(big[k].dim() - (2 if k in PLANES else 1), ix)), (n, k)


def test_two_runs_and_the_three_forms_are_bit_identical(engine, res_pop, res_case):
    _load(engine, res_pop)
    batch, kw, kwh, pkw, d = (res_case[k] for k in ("batch", "kw", "kwh", "pkw", "d"))
    again = engine.replay_at(batch, kw, kwh, pkw, planes="f64")
    summ = engine.replay_at(batch, kw, kwh, pkw)
    plan = engine.replay_at(batch, kw, kwh, pkw, want=(), planes="f64")
    torch.cuda.synchronize()
    _same(again, d, "second run")
    assert sorted(summ) == sorted(MEMBERS + ["bank_kwh", "power_kw", "status"])
    assert sorted(plan) == sorted(PLANES + ["bank_kwh", "power_kw", "status"])
    _same(summ, d, "summary only")
    _same(plan, d, "planes only")
    # the midday window is opt's
    w = engine.replay_at(batch, kw, kwh, pkw, midday=(0, 23))
    for k in ("surplus", "pv_to_batt", "pv_to_grid"):
        assert torch.equal(w[f"{k}_mid_kwh"], d[f"{k}_kwh"]), k
    with pytest.raises(ValueError):
        engine.replay_at(batch, kw, kwh, pkw, want=())
    with pytest.raises(ValueError):
        engine.replay_at(batch, kw, kwh, pkw, planes="f16")
    with pytest.raises(ValueError):
        engine.replay_at(batch, kw[:-1], kwh, pkw)


def _raw_call(eng, batch, cols, so, po, bank, power, status, opt=None, n=None):
    f = lambda t: None if t is None else t.data_ptr()
    return eng.lib.dgen_replay_at(eng.ctx, ctypes.byref(eng.tables), ctypes.byref(batch.c_agents), f(cols[0]),
                                  f(cols[1]), f(cols[2]), batch.n if n is None else n,
                                  None if opt is None else ctypes.byref(opt),
                                  None if so is None else ctypes.byref(so), None if po is None else ctypes.byref(po),
                                  f(bank), f(power), f(status), eng.stream_handle())


def _sentinels(eng, n):
    bufs = {k: torch.full((12, n), -7.0, dtype=torch.float64, device=eng.dev) for k in _lib.BATT_SUMMARY_F64}
    bufs.update({k: torch.full((12, n), -7, dtype=torch.int32, device=eng.dev) for k in _lib.BATT_SUMMARY_I32})
    bufs.update({k: torch.full((_lib.NH // 4, n, 4), -7.0, dtype=torch.float64, device=eng.dev) for k in PLANES})
    bufs.update({k: torch.full((n,), -7.0, dtype=torch.float64, device=eng.dev) for k in ("bank_kwh", "power_kw")})
    bufs["status"] = torch.full((n,), -7, dtype=torch.int32, device=eng.dev)
    return bufs


def test_null_members_planes_and_arguments(engine, res_pop, res_case):
    """A NULL member, plane or bank column is not written (sentinel-filled
    buffers beside the ones asked for keep their sentinel); argument errors
    return DGEN_E_ARG with a message and launch nothing."""
    _load(engine, res_pop)
    batch, d = res_case["batch"], res_case["d"]
    n = batch.n
    cols = [engine._to_dev(res_case[k], torch.float64) for k in ("kw", "kwh", "pkw")]
    bufs = _sentinels(engine, n)
    wanted = ("pv_to_batt_kwh", "soc_end", "hours_empty", "with_batt", "power_kw", "status")
    so = _lib.BattSummaryOut(**{k: bufs[k].data_ptr() for k in wanted if k in MEMBERS})
    po = _lib.ReplayPlanes(None, None, bufs["with_batt"].data_ptr(), 1, 0)
    assert _raw_call(engine, batch, cols, so, po, None, bufs["power_kw"], bufs["status"]) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for k, v in bufs.items():
        if k in wanted:
            assert torch.equal(v, d[k]), k
        else:
            assert (v == -7).all().item(), k
    # argument errors: nothing is launched
    bufs = _sentinels(engine, n)
    so = _lib.BattSummaryOut(**{k: bufs[k].data_ptr() for k in MEMBERS})
    po = _lib.ReplayPlanes(*[bufs[k].data_ptr() for k in PLANES], 1, 0)
    tail = (bufs["bank_kwh"], bufs["power_kw"], bufs["status"])
    assert _raw_call(engine, batch, cols, None, None, *tail) == -1                      # DGEN_E_ARG
    assert "neither" in _lib.last_error()
    for lo, hi in ((12, 11), (-1, 5), (3, 24)):
        assert _raw_call(engine, batch, cols, so, po, *tail, opt=_lib.BattSummaryOpt(lo, hi)) == -1, (lo, hi)
        assert "midday" in _lib.last_error()
    assert _raw_call(engine, batch, cols, so, po, *tail, n=-1) == -1
    assert _raw_call(engine, batch, cols, so, po, bufs["bank_kwh"], bufs["power_kw"], None) == -1
    assert _raw_call(engine, batch, [None, cols[1], cols[2]], so, po, *tail) == -1
    assert _raw_call(engine, batch, cols, so, _lib.ReplayPlanes(*[bufs[k].data_ptr() for k in PLANES], 2, 0),
                     *tail) == -1
    off8 = _lib.ReplayPlanes(bufs["baseline"].data_ptr(), bufs["pvonly"].data_ptr() + 8, None, 1, 0)
    assert _raw_call(engine, batch, cols, so, off8, *tail) == -1                        # 16-B vector stores
    assert "aligned" in _lib.last_error()
    assert _raw_call(engine, batch, cols, so, po, *tail, n=1 << 27) == -1               # refused before any launch
    assert "2^27" in _lib.last_error()
    assert _raw_call(engine, batch, cols, so, po, *tail, n=0) == 0                      # n = 0: no launch
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert (v == -7).all().item(), k


@pytest.mark.parametrize("cfg_kw", [{"batt_update_hours": 1}, {"batt_loss_model": 1}], ids=["hourly_replan", "loss_model"])
def test_unsupported_dispatch_configurations_are_refused(res_pop, cfg_kw):
    from dgen_amd.engine import Engine
    eng = Engine(0, EngineConfig(**cfg_kw))
    try:
        _load(eng, res_pop)
        sub = subset(res_pop, np.arange(1))
        batch = eng.upload_agents(sub.cols, sub.n_scratch)
        bufs = _sentinels(eng, 1)
        cols = [torch.ones(1, dtype=torch.float64, device=eng.dev) for _ in range(3)]
        so = _lib.BattSummaryOut(**{k: bufs[k].data_ptr() for k in MEMBERS})
        assert _raw_call(eng, batch, cols, so, None, bufs["bank_kwh"], bufs["power_kw"], bufs["status"]) == -1
        assert "dgen_replay_at" in _lib.last_error()
        with pytest.raises(_lib.DgenError):
            eng.replay_at(batch, cols[0], cols[1])
        torch.cuda.synchronize()
        for k, v in bufs.items():
            assert (v == -7).all().item(), k
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 5. flags
# ---------------------------------------------------------------------------
def test_flagged_rows_get_zeros_and_leave_their_neighbours(engine, res_pop, res_case):
    """Every DGEN_ST_BOUNDS case on a row of its own in a 65-agent batch
    (agents 0 .. 64 of the 257; rows 0, 63 and 64 among them): zeros and the
    status bit there, every other row the bits of the clean batch.  kw = 0 and
    a bank_kw of 0 beside bank_kwh = 0 are valid."""
    n = 65
    sub = subset(res_pop, np.arange(n))
    _load(engine, res_pop)
    batch = engine.upload_agents(sub.cols, sub.n_scratch)
    kw, kwh, pkw = (res_case[k][:n].copy() for k in ("kw", "kwh", "pkw"))
    bad = {0: ("kw", np.nan), 5: ("kw", -1.0), 63: ("kw", np.inf), 64: ("kwh", np.nan), 17: ("kwh", -0.5),
           23: ("kwh", np.inf), 31: ("pkw", 0.0), 40: ("pkw", np.nan), 41: ("pkw", -2.0), 62: ("pkw", np.inf),
           50: ("kw", -np.inf)}
    cols = {"kw": kw, "kwh": kwh, "pkw": pkw}
    for r, (c, v) in bad.items():
        cols[c][r] = v
    kw[7] = 0.0                      # valid: no PV
    kwh[9], pkw[9] = 0.0, 0.0        # valid: no bank, its power is not looked at
    kwh[11], pkw[11] = 0.0, np.nan
    rows = np.array(sorted(bad))
    touched = np.array(sorted(list(bad) + [7, 9, 11]))
    others = torch.as_tensor(np.setdiff1d(np.arange(n), touched), device=engine.dev)
    big = res_case["d"]
    for planes in ("f64", "f32"):
        d = engine.replay_at(batch, kw, kwh, pkw, planes=planes)
        torch.cuda.synchronize()
        st = d["status"].cpu().numpy()
        assert (st[rows] == _lib.ST_BOUNDS).all() and not np.delete(st, rows).any()
        ix = torch.as_tensor(rows, device=engine.dev)
        for k, v in d.items():
            if k == "status":
                continue
            dim = v.dim() - (2 if k in PLANES else 1)
            assert not v.index_select(dim, ix).any().item(), (planes, k)
            want = big[k].index_select(dim, others)
            assert torch.equal(v.index_select(dim, others), want.to(v.dtype) if k in PLANES else want), (planes, k)
        assert (d["pv_kwh"][:, 7] == 0).all().item() and (d["bank_kwh"][7] > 0).item()
        assert not d["bank_kwh"][[9, 11]].any().item() and (d["grid_to_load_kwh"][:, [9, 11]] > 0).all().item()
    # bank_kw NULL: its values are not looked at
    d = engine.replay_at(batch, res_case["kw"][:n], res_case["kwh"][:n], None)
    torch.cuda.synchronize()
    assert not d["status"].any().item()


# ---------------------------------------------------------------------------
# 6. the drop-in switches
# ---------------------------------------------------------------------------
def test_drop_in_switch(engine):
    from dgen_amd.columnar import columnize_frame
    from dgen_amd.engine import profile_order
    from dgen_amd.synth import reference_frame
    df, store, table = reference_frame(65)
    ff._worker_conn = store
    r, h = (0.4, 0.8, 1.6), (1.0, 2.0, 4.0)
    spec = {"pv_to_batt": r, "hours": h}
    off, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing=spec)
    on, o_on = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing={**spec, "dispatch": True})
    diag = bs.columns_of({"dispatch": True})[len(bs.COLUMNS):]
    assert list(on.columns) == list(off.columns) + list(diag)
    assert not any(c.startswith(bs.DIAG_PREFIX) for c in off.columns)
    # the key adds columns and changes none: every numeric column of the frame without it is unchanged
    for c in off.columns:
        a, b = off[c].to_numpy(), on[c].to_numpy()
        if a.dtype.kind in "fiub":
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), c
    # the columns are replay_columns of replay_outputs at the best point
    eng = ff.get_engine()
    cols = columnize_frame(df, store, table).frame_columns
    batch = eng.upload_agents(cols, order=profile_order(cols))
    point = on["batt_opt_point"].to_numpy()
    valid = point >= 0
    assert valid.any()
    skw = on["system_kw"].to_numpy()
    rr = np.array([a for a in r for _ in h] + [bs.REF_PV_TO_BATT])      # ratio-major, the reference's point last
    hh = np.array([b for _ in r for b in h] + [bs.REF_HOURS])
    kwh = np.where(valid, skw / rr[np.maximum(point, 0)], 0.0)
    pkw = np.where(valid, kwh / hh[np.maximum(point, 0)], 1.0)
    d = bm.replay_outputs(eng, batch, np.where(valid, skw, 0.0), kwh, pkw)
    torch.cuda.synchronize()
    assert not d["status"].any().item()
    want = bm.replay_columns(d, eng.cfg, bs.DIAG_PREFIX)
    assert np.array_equal(d["bank_kwh"].cpu().numpy()[valid], on["batt_opt_kwh"].to_numpy()[valid])
    for c in diag:
        a = on[c].to_numpy()
        assert a.dtype == (np.int64 if c[len(bs.DIAG_PREFIX):] in bm.COUNT_MEMBERS else np.float64), c
        assert np.array_equal(a[valid], want[c][valid]), c
        assert (np.isnan(a[~valid]) if a.dtype.kind == "f" else a[~valid] == 0).all(), c
    assert (on["batt_opt_diag_batt_to_load_kwh"].to_numpy()[valid] >= 0).all()
    # sub-batches: the same bits
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", batt_sizing={**spec, "dispatch": True}, max_rows=30)
    for c in diag:
        assert np.array_equal(sub[c].to_numpy(), on[c].to_numpy(), equal_nan=True), c
    # the PV size on the with-battery objective, at 1.2 kWh per kW... ratio 1.2 and 4 h
    cspec = {"ratio": 1.2, "hours": 4.0}
    coff, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing=cspec)
    con, _ = ff.size_chunk(df, None, table, "simple", hourly="none", pv_batt_sizing={**cspec, "dispatch": True})
    cdiag = bs.co_columns_of({"dispatch": True})[len(bs.CO_COLUMNS):]
    assert list(con.columns) == list(coff.columns) + list(cdiag)
    for c in bs.CO_COLUMNS:
        assert np.array_equal(coff[c].to_numpy(), con[c].to_numpy(), equal_nan=True), c
    x = con["pvb_opt_kw"].to_numpy()
    ok = ((con["pvb_opt_status"].to_numpy() & bs.INVALID) == 0) & np.isfinite(x)
    assert ok.any()
    e = np.where(ok, x / 1.2, 0.0)
    d = bm.replay_outputs(eng, batch, np.where(ok, x, 0.0), e, np.where(ok, e / 4.0, 1.0))
    torch.cuda.synchronize()
    want = bm.replay_columns(d, eng.cfg, bs.CO_DIAG_PREFIX)
    assert np.array_equal(d["bank_kwh"].cpu().numpy()[ok], con["pvb_opt_kwh"].to_numpy()[ok])
    assert np.array_equal(d["power_kw"].cpu().numpy()[ok], con["pvb_opt_batt_kw"].to_numpy()[ok])
    for c in cdiag:
        a = con[c].to_numpy()
        assert np.array_equal(a[ok], want[c][ok]), c
        assert (np.isnan(a[~ok]) if a.dtype.kind == "f" else a[~ok] == 0).all(), c
