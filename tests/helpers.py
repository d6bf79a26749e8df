"""Shared test helpers: golden fixtures -> product columns / oracle population."""
from __future__ import annotations

import json
import os
from functools import lru_cache

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


@lru_cache(maxsize=None)
def golden_agents():
    with open(os.path.join(GOLDEN, "agents.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "agents.npz"), allow_pickle=False)
    arrays = {k: z[k] for k in z.files}
    return meta, arrays


@lru_cache(maxsize=None)
def golden_tariffs():
    with open(os.path.join(GOLDEN, "tariffs.json")) as f:
        return json.load(f)


@lru_cache(maxsize=None)
def golden_brent():
    with open(os.path.join(GOLDEN, "brent.json")) as f:
        return json.load(f)


def golden_population():
    """PopulationBuilder over the golden agents (product host path)."""
    from dgen_amd.columnar import PopulationBuilder
    meta, arr = golden_agents()
    tariffs = {name: raw for name, raw in meta["tariff_cases"]}
    table = pd.DataFrame(meta["switch_table"])
    b = PopulationBuilder(table)
    ws = arr["wholesale"]
    for i, a in enumerate(meta["agents"]):
        s = a["inputs"]
        b.add(load_row=s["load_row"], cf_row=s["cf_row"], sector_abbr=s["sector_abbr"],
              state_abbr=s["state_abbr"], eia_id=s["eia_id"], tariff_dict=tariffs[s["tariff"]],
              wholesale=ws[s["wholesale_row"]], load_kwh=s["load_kwh_per_customer_in_bin"],
              price_mult=s["elec_price_multiplier"], econ_life=s["economic_lifetime_yrs"],
              loan_term=s["loan_term_yrs"], inflation=s["inflation_rate"],
              pv_deg=s["pv_degradation_factor"], escalator=s["elec_price_escalator"],
              down_payment=s["down_payment_fraction"], tax_rate=s["tax_rate"],
              real_discount=s["real_discount_rate"], itc_frac=s["itc_fraction_of_capex"],
              capex=s["system_capex_per_kw"], capex_combined=s["system_capex_per_kw_combined"],
              batt_capex_kwh=s["batt_capex_per_kwh_combined"], ccm=s["cap_cost_multiplier"],
              vor=s["value_of_resiliency_usd"])
    cols = b.columns()
    return b, cols, arr["shapes"], arr["cfs"], b.wholesale.array()


def oracle_tariffs(records, demand=None):
    """Device tariff records (+ the dgen_demand table) -> orc.Tariff list."""
    from oracle import oracle as orc
    out = []
    for r in records:
        t = orc.Tariff()
        t.P, t.T, t.mo, t.unit = int(r["P"]), int(r["T"]), int(r["mo"]), int(r["unit"])
        t.fixed = float(r["fixed"])
        for k in range(orc.MAXT):
            t.cap[k] = float(r["cap"][k])
        for p in range(orc.MAXP):
            for k in range(orc.MAXT):
                t.buy[p][k] = float(r["buy"][p, k])
                t.sell[p][k] = float(r["sell"][p, k])
        for m in range(12):
            for h in range(24):
                t.wkday[m][h] = int(r["wkday"][m, h])
                t.wkend[m][h] = int(r["wkend"][m, h])
        dc = int(r["dc"])
        if dc > 0:
            d = demand[dc - 1]
            t.dc_on = 1
            for p in range(orc.DCP):
                t.dc_tou_nt[p] = int(d["tou_nt"][p])
                for k in range(orc.DCT):
                    t.dc_tou_cap[p][k] = float(d["tou_cap"][p, k])
                    t.dc_tou_price[p][k] = float(d["tou_price"][p, k])
            for m in range(12):
                t.dc_flat_nt[m] = int(d["flat_nt"][m])
                for k in range(orc.DCT):
                    t.dc_flat_cap[m][k] = float(d["flat_cap"][m, k])
                    t.dc_flat_price[m][k] = float(d["flat_price"][m, k])
                for h in range(24):
                    t.dc_wkday[m][h] = int(d["wkday"][m, h])
                    t.dc_wkend[m][h] = int(d["wkend"][m, h])
        out.append(t)
    return out


def oracle_population(cols, tariff_records, switches, shapes, cfs, wholesale, demand=None):
    """orc.Population mirroring product columns (same tables, same indices)."""
    from oracle import oracle as orc
    n = len(cols["load_kwh"])
    sw_solar, sw_storage = [], []
    for i in range(n):
        for k, dst in (("solar", sw_solar), ("storage", sw_storage)):
            off, cnt = int(cols[f"sw_{k}_off"][i]), int(cols[f"sw_{k}_cnt"][i])
            dst.append([(float(r["min_kw"]), float(r["max_kw"]), float(r["one_time_charge"]),
                         int(r["tariff"])) for r in switches[off:off + cnt]])
    ocols = {
        "load_row": cols["load_row"], "cf_row": cols["cf_row"],
        "wholesale_row": cols["wholesale_row"], "load_kwh": cols["load_kwh"],
        "price_mult": cols["price_mult"], "inflation": cols["inflation"], "pv_deg": cols["pv_deg"],
        "escalator": cols["escalator"], "down_payment": cols["down_payment"],
        "tax_rate": cols["tax_rate"], "real_discount": cols["real_discount"],
        "itc_frac": cols["itc_frac"], "capex": cols["capex"],
        "capex_combined": cols["capex_combined"],
        "batt_capex_kwh_combined": cols["batt_capex_kwh"], "ccm": cols["ccm"], "vor": cols["vor"],
        "is_res": (cols["flags"] & 1).astype(int), "is_ca": ((cols["flags"] >> 1) & 1).astype(int),
        "econ_life": cols["econ_life"], "loan_term": cols["loan_term"], "tariff0": cols["tariff0"],
    }
    return orc.Population(ocols, shapes, cfs, wholesale, oracle_tariffs(tariff_records, demand),
                          sw_solar, sw_storage)


def final_tariff_id(builder, agent_tariff_id, final_index, switched):
    if switched:
        r = builder.switches.row_of_tariff.get(int(final_index))
        if r is not None:
            return r["rate_id_alias"]
    return agent_tariff_id


def golden_rows():
    """The golden agents as reference-style agent rows (pd.Series) + a
    ProfileStore + the rate switch table, as make_golden.py built them."""
    from dgen_amd.profiles import ProfileStore
    meta, arr = golden_agents()
    tariffs = {name: raw for name, raw in meta["tariff_cases"]}
    store = ProfileStore()
    rows = []
    for i, a in enumerate(meta["agents"]):
        s = dict(a["inputs"])
        lr, cr, wr = s.pop("load_row"), s.pop("cf_row"), s.pop("wholesale_row")
        s.pop("tag")
        s["tariff_dict"] = tariffs[s.pop("tariff")]
        s["agent_id"] = i
        s["bldg_id"] = 1000 + lr
        s["solar_re_9809_gid"] = 5000 + cr
        s["tariff_id"] = 900 + i
        s["wholesale_prices"] = arr["wholesale"][wr]
        store.add_load((s["bldg_id"], s["sector_abbr"], s["state_abbr"]), arr["shapes"][lr])
        store.add_solar((s["solar_re_9809_gid"], s["tilt"], s["azimuth"]), arr["cfs"][cr])
        rows.append(pd.Series(s, name=i))
    return rows, store, pd.DataFrame(meta["switch_table"])


@lru_cache(maxsize=None)
def golden_attach():
    """(meta, hourly): attach.json cases + the f32 planes from attach.npz,
    hourly[name] = (baseline, pvonly, with_batt) as float64 [n, n_hours]."""
    with open(os.path.join(GOLDEN, "attach.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "attach.npz"), allow_pickle=False)
    hourly = {}
    for c in meta["cases"]:
        k = c["name"]
        hourly[k] = tuple(z[f"{k}__{p}"].astype(np.float64) for p in ("baseline", "pvonly", "with_batt"))
    return meta, hourly


def _dec(cell):
    """finance_series.json cell -> the Python value the reference saw."""
    f = lambda x: float(x) if isinstance(x, str) and x in ("nan", "inf", "-inf") else x
    if "list" in cell:
        return [f(x) for x in cell["list"]]
    if "array" in cell:
        return np.asarray([f(x) for x in cell["array"]], dtype=float)
    return f(cell["scalar"])


@lru_cache(maxsize=None)
def golden_finance():
    """finance_series.json with the input rows decoded (lists, numpy arrays,
    scalars, non-finite floats) -- cases[k]['rows'] are dicts per agent."""
    with open(os.path.join(GOLDEN, "finance_series.json")) as f:
        meta = json.load(f)
    for c in meta["cases"]:
        c["rows"] = [{k: _dec(v) for k, v in r.items()} for r in c["rows"]]
    return meta


@lru_cache(maxsize=None)
def golden_tariffs_dc():
    """tariffs_dc.json: the reference's compile with SKIP_DEMAND_CHARGES
    flipped (tests/golden/make_golden_demand.py)."""
    with open(os.path.join(GOLDEN, "tariffs_dc.json")) as f:
        return json.load(f)


# tests/golden/market.json column -> device SoA / loop column (dgen_amd.market)
MARKET_COLS = {"load_kwh_per_customer_in_bin": "load_kwh", "customers_in_bin": "customers_in_bin",
               "load_kwh_in_bin": "load_kwh_in_bin", "elec_price_multiplier": "price_mult",
               "elec_price_escalator": "escalator", "pv_degradation_factor": "pv_deg",
               "system_capex_per_kw": "capex", "system_capex_per_kw_combined": "capex_combined",
               "batt_capex_per_kwh_combined": "batt_capex_kwh", "value_of_resiliency_usd": "vor",
               "itc_fraction_of_capex": "itc_frac", "inflation_rate": "inflation",
               "economic_lifetime_yrs": "econ_life", "loan_term_yrs": "loan_term",
               "down_payment_fraction": "down_payment", "real_discount_rate": "real_discount",
               "tax_rate": "tax_rate"}


@lru_cache(maxsize=None)
def golden_market():
    """market.json (tests/golden/make_golden_market.py): agents, the reference's
    input tables as DataFrames, and per year the merged columns (None -> NaN)."""
    with open(os.path.join(GOLDEN, "market.json")) as f:
        meta = json.load(f)
    nan = lambda v: np.array([np.nan if x is None else x for x in v], dtype=np.float64)
    meta["agents"] = pd.DataFrame(meta["agents"])
    T = {k: pd.DataFrame(v) for k, v in meta["tables"].items()}
    meta["tables"] = {"load_growth": T["load_growth"], "elec_price": T["elec"], "pv_tech": T["pv_tech"],
                      "pv_price": T["pv_price"], "pv_plus_batt_price": T["pvb_price"], "vor": T["vor"],
                      "financing": T["fin"], "itc": T["itc"]}
    for y in meta["years"]:
        y["columns"] = {k: nan(v) for k, v in y["columns"].items()}
        if "initial" in y:
            y["initial"]["columns"] = {k: nan(v) for k, v in y["initial"]["columns"].items()}
    return meta


# ---------------------------------------------------------------------------
# Brent paths: the device's fast search bills from
# re-associated sums, a few ulps from the oracle's hour order; scipy's bounded
# Brent divides differences of nearly equal objective values in its parabolic
# step, so such a difference can move the search path.  The certified paths
# (dgen_set_exact, on by default) re-run every agent whose path a bound on that
# difference does not settle in the oracle's arithmetic, so every agent is on
# the oracle's path (same_path); with them off (exact_brent = 0), a divergent
# agent ends within scipy's xatol and equals the oracle's driver evaluated at
# the device's own search end (at_device_point).
# ---------------------------------------------------------------------------
def xatol_of(load_kwh: float, naep: float) -> float:
    """ff:440-444: bracket (0.8, 1.25) x load / naep, xatol = max(2, int(1e-3 x span))."""
    hi_lo = (load_kwh / naep) * 1.25 - (load_kwh / naep) * 0.8
    return max(2.0, float(int(max(hi_lo, 1.0) * 1e-3)))


def same_path(o, i: int, r) -> bool:
    """Device agent i (o: host outputs) took the oracle result r's Brent path."""
    return (int(o["nfev"][i]) == int(r["nfev"])
            and abs(o["system_kw"][i] - r["system_kw"]) <= 1e-9 * max(1.0, abs(r["system_kw"]))
            and abs(o["x_last"][i] - r["x_last"]) <= 1e-9 * max(1.0, abs(r["x_last"])))


def at_device_point(o, i: int, opop, j: int, cfg, r, xatol: float, hourly: bool = False):
    """Oracle outputs of agent j of opop evaluated once at device agent i's
    search end -- its kW, last x and sticky tariff state (tariff_final and
    switched as the device reports them: size with the battery run off, so no
    storage switch follows the search).  The device's kW must be within
    scipy's xatol of the oracle's search result."""
    kw, xl = float(o["system_kw"][i]), float(o["x_last"][i])
    assert abs(kw - r["system_kw"]) <= xatol, ("kW beyond xatol", i, kw, r["system_kw"], xatol)
    e = opop.eval_at(cfg, j, kw, xl, int(o["tariff_final"][i]), int(o["switched"][i]), hourly=hourly)
    e["nfev"] = int(o["nfev"][i])
    return e


# ---------------------------------------------------------------------------
# GPU <-> oracle comparison of a sized batch (DESIGN.md section 2 tolerances)
# ---------------------------------------------------------------------------
def check_sized_against_oracle(o, ref, cols, payback_raw=False):
    """Every agent of the host outputs `o` (outputs_to_host, hourly planes
    included) against the oracle results `ref` (Population.run(hourly=True)):
    status 0 on both sides, the oracle's Brent path (certified paths), the
    scalars, the five yearly arrays over [:N + 1] and the two hourly planes.
    payback_raw: also the unrounded payback, 1e-9 relative.  Returns the
    number of agents that switched rate."""
    n_switch = 0
    for i, r in enumerate(ref):
        assert o["status"][i] == 0 and r["status"] == 0, i
        # every agent on the oracle's Brent path (certified paths)
        assert same_path(o, i, r), (i, o["nfev"][i], r["nfev"], o["system_kw"][i], r["system_kw"])
        assert o["nfev"][i] == r["nfev"], (i, o["nfev"][i], r["nfev"])
        assert o["tariff_final"][i] == r["tariff_final"], i
        assert o["switched"][i] == r["switched"], i
        n_switch += int(r["switched"])
        assert abs(o["system_kw"][i] - r["system_kw"]) <= 1e-9 * max(1.0, r["system_kw"]), i
        for k in ("npv", "annual_kwh", "first_with", "first_without", "batt_kwh", "batt_kw",
                  "npv_pv_batt"):
            assert np.isclose(o[k][i], r[k], rtol=1e-6, atol=1e-6), (i, k, o[k][i], r[k])
        assert o["payback_period"][i] == r["payback_period"], (i, o["payback_raw"][i], r["payback_raw"])
        if payback_raw:
            assert abs(o["payback_raw"][i] - r["payback_raw"]) <= 1e-9 * abs(r["payback_raw"]), \
                (i, o["payback_raw"][i], r["payback_raw"])
        N1 = int(cols["econ_life"][i]) + 1
        for k_o, k_r in (("cash_flow", "cash_flow"), ("cfev_pv", "cf_energy_value_pv_only"),
                         ("bill_w_pv", "bill_w_pv_only"), ("cfev_batt", "cf_energy_value_pv_batt"),
                         ("bill_w_batt", "bill_w_pv_batt")):
            assert np.allclose(o[k_o][i, :N1], r[k_r], rtol=1e-6, atol=1e-5), (i, k_o)
        for k_o, k_r in (("net_pvonly", "adopter_net_hourly_pvonly"),
                         ("net_with_batt", "adopter_net_hourly_with_batt")):
            ref_h = r[k_r]
            assert np.allclose(o[k_o][i], ref_h, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref_h).max())), (i, k_o)
    return n_switch


# ---------------------------------------------------------------------------
# Edge populations: dgen_amd.synth gives every agent one point of the
# financing parameter space (life 25, term 20 / 30, ...); these overwrite the
# financing columns of a small synthetic population with the values where the
# Cashloan arithmetic branches, and lay the lives out by wave pair.
# ---------------------------------------------------------------------------
EDGE_SHORT_LIVES = (1, 2, 3, 6, 7, 8, 16, 25, 31, 32)
EDGE_LONG_LIVES = (1, 2, 7, 32, 33, 49, 50)
# device rows 2k, 2k + 1 share a wave when every life is <= 32: these pairs come first
EDGE_PAIRS = ((1, 32), (32, 1), (32, 32), (1, 1), (7, 8), (25, 2))
EDGE_VALUES = {
    "loan_term": (0, 1, 5, 10, 20, 32, 40),
    "down_payment": (0.0, 0.3, 1.0),
    "tax_rate": (0.0, 0.2574, 0.45),
    "real_discount": (0.0, 0.05, 0.15),
    "inflation": (-0.01, 0.0, 0.025, 0.08),
    "pv_deg": (0.0, 0.005, 0.05),
    "itc_frac": (0.0, 0.3, 1.0),
    "escalator": (-0.03, 0.0, 0.04),
}
EDGE_CAPEX_FACTORS = (0.05, 0.3, 1.0)       # payback in year 1, late, never


def edge_lives(n, lives, rng):
    """econ_life per row.  "short": the EDGE_PAIRS first, then pairs of two
    different EDGE_SHORT_LIVES; "long": EDGE_LONG_LIVES drawn per row (the
    batch then runs one agent per wave)."""
    if lives == "long":
        life = rng.choice(EDGE_LONG_LIVES, n)
        assert life.max() > 32
        return life.astype(np.int32)
    assert lives == "short", lives
    pairs = list(EDGE_PAIRS)
    while 2 * len(pairs) < n:
        a, b = rng.choice(EDGE_SHORT_LIVES, 2, replace=False)
        pairs.append((int(a), int(b)))
    assert n >= 2 * len(EDGE_PAIRS)
    assert sum(a != b for a, b in pairs[:n // 2]) * 4 >= 3 * (n // 2)
    return np.asarray(pairs, np.int32).reshape(-1)[:n].copy()


def edge_population(cfg, n, lives, seed, storage_rows=True):
    """make_population(cfg, n) at the small table sizes of
    test_gpu_synthetic._small_pop with the financing columns overwritten from
    default_rng(seed): EDGE_VALUES per agent, capex and capex_combined scaled
    by one of EDGE_CAPEX_FACTORS, lives laid out by edge_lives.  storage_rows:
    every second agent (the odd rows) gets a storage rate-switch candidate --
    the solar row of another agent of its sector and state class, i.e. of a
    different utility, where the population has one, else its own -- and the
    scratch slots are assigned again."""
    from dgen_amd.columnar import assign_scratch
    from dgen_amd.synth import make_population
    pop = make_population(cfg, n, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16,
                          n_tariffs=48)
    rng = np.random.default_rng(seed)
    c = pop.cols
    c["econ_life"] = edge_lives(n, lives, rng)
    for name, values in EDGE_VALUES.items():
        c[name] = rng.choice(values, n).astype(c[name].dtype)
    f = rng.choice(EDGE_CAPEX_FACTORS, n)
    c["capex"] = c["capex"] * f
    c["capex_combined"] = c["capex_combined"] * f
    assert (c["loan_term"] < c["econ_life"]).any() and (c["loan_term"] > c["econ_life"]).any()
    if storage_rows:
        off, cnt = c["sw_storage_off"].copy(), c["sw_storage_cnt"].copy()
        has = c["sw_solar_cnt"] > 0
        for i in range(1, n, 2):
            same = has & (c["flags"] == c["flags"][i])
            other = np.unique(c["sw_solar_off"][same & (c["sw_solar_off"] != c["sw_solar_off"][i])])
            if other.size:
                off[i], cnt[i] = other[rng.integers(0, other.size)], 1
            elif has[i]:
                off[i], cnt[i] = c["sw_solar_off"][i], 1
        c["sw_storage_off"], c["sw_storage_cnt"] = off, cnt
    pop.n_scratch = assign_scratch(c, pop.tariffs, pop.switches)
    return pop


def edge_coverage(cols, ref, ref_no_storage=None, slots=True, switch=True, early=True):
    """The edges an edge population must reach, from the columns and the
    oracle's results alone (never device output).  slots / switch / early: off
    for populations that cannot hold the edge (no tariff that needs a scratch
    slot; no rate-switch row in reach; no payback within the first year)."""
    n = len(ref)
    raw = np.array([r["payback_raw"] for r in ref])
    none = raw >= 1e98               # SSC's 1e99: no year's cumulative flow turns positive
    assert (~none).sum() * 10 >= n and none.sum() * 10 >= n, (int(none.sum()), n)
    if early:
        assert (raw < 1.0).any()
    life, term = np.asarray(cols["econ_life"]), np.asarray(cols["loan_term"])
    assert (term == 0).any() and (term > life).any() and (np.asarray(cols["down_payment"]) == 1.0).any()
    if slots:
        assert ((np.asarray(cols["pv_deg"]) == 0.0) & (np.asarray(cols["scratch_slot"]) >= 0)).any()
    assert (life == 1).any() and (life == 32).any()
    if switch:
        assert sum(int(r["switched"]) for r in ref) >= 1
    if ref_no_storage is not None:
        if switch:                 # a switch made by the search itself, not only by the battery run
            assert sum(int(r["switched"]) for r in ref_no_storage) >= 1
        moved = sum(r["npv_pv_batt"] != q["npv_pv_batt"] for r, q in zip(ref, ref_no_storage))
        assert moved >= 4, moved
