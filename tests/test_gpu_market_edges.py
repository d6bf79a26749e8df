"""The market-step kernels (k_year_inputs, k_initial_shares, k_max_market_share,
k_diffusion, k_export_weights) at the edges the recorded fixtures never reach:
merge misses in every table, groups past one block of members with NaN / zero
/ Kahan-sensitive weights and a scattered device order, payback ties and curve
gaps, every selection branch of the diffusion step with its inf / NaN pattern,
and an ill-conditioned block against a 50-digit reference.

Everything is bit for bit (equal_nan) against pandas or the oracle
restatements, except the transcendental columns of k_diffusion:

* well-conditioned block (the fixture's ranges): rtol 1e-12, the project's
  tolerance for this kernel;
* ill-conditioned blocks (tests/market_refs.py diffusion_ill): per column
  max(1e-12, 8 x the float64 oracle's own max relative error against the
  mpmath restatement on the same inputs).

  Oracle error as measured (numpy 2.2 / glibc), first year / later years:
    slow (p + q down to 1e-6):  new_market_share, new_adopters, new_market_value,
          new_system_kw 2.5e-10 / 2.1e-10; the three cumulative columns up to
          1.7e-13; every other column below 6e-16 (so their tolerance is 1e-12)
    near (1 - ratio down to 1e-12):  bass_params_teq and teq2 1.7e-6, f 5.2e-5,
          the four new_* columns 1.9e-4 / 2.2e-4, the cumulative columns up to
          1.2e-13, the rest below 3e-16
  Device error against the same mpmath values as measured on the MI355X: equal
  to the oracle's in every printed digit on the cancellation-dominated columns
  (slow: new_* 2.48e-10 / 2.09e-10; near: teq 1.66e-6, f 5.22e-5, new_*
  1.89e-4 / 2.15e-4), so device error / tolerance is 0.125 there and at most
  0.001 on the columns held to 1e-12 (teq 3.3e-16, f 5.1e-16 in the slow
  block).  The test prints the three figures per column.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from dgen_amd import _lib
from dgen_amd import attachment as ga
from dgen_amd import diffusion as gd
from dgen_amd import market as gm
from dgen_amd.dist import group_order
from oracle import attach as oa
from oracle import diffusion as od
from oracle import market as om
from tests import market_refs as mr

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1025]


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ------------------------------------------------------------------ year inputs
YEARS = (2026, 2040, 2050)
SECTORS = ("res", "com", "ind")
COUNTIES = (11, 12, 13, 14, 15)
STATES = ("AA", "BB")


def _year_tables(wholesale=True):
    """The reference's input frames, with holes: 'ind' has no pv_price and no
    financing row; (com, 13) and (res, 12) have no load growth and (res, 14) no price
    trajectory; (BB, ind) has no value of resiliency; county 15 is not in the
    wholesale map (and county 12 only in some years)."""
    rng = np.random.default_rng(77)
    sec_year = [(y, s) for y in YEARS for s in SECTORS]
    sc_year = [(y, s, c) for y in YEARS for s in SECTORS for c in COUNTIES]
    frame = lambda keys, names, **cols: pd.DataFrame({**{n: [k[i] for k in keys] for i, n in enumerate(names)},
                                                      **{c: f(len(keys)) for c, f in cols.items()}})
    u = lambda lo, hi: (lambda m: rng.uniform(lo, hi, m))
    no_ind = [k for k in sec_year if k[1] != "ind"]
    T = {
        "pv_price": frame(no_ind, ["year", "sector_abbr"], system_capex_per_kw=u(900, 3000)),
        "pv_plus_batt_price": frame(sec_year, ["year", "sector_abbr"], system_capex_per_kw=u(1000, 3300),
                                    batt_capex_per_kwh=u(200, 900)),
        "pv_tech": frame(sec_year, ["year", "sector_abbr"], pv_degradation_factor=u(0.003, 0.008)),
        "financing": frame(no_ind, ["year", "sector_abbr"],
                           economic_lifetime_yrs=lambda m: rng.integers(20, 31, m),
                           loan_term_yrs=lambda m: rng.integers(10, 26, m),
                           down_payment_fraction=u(0.1, 0.5), real_discount_rate=u(0.02, 0.09),
                           tax_rate=u(0.2, 0.4)),
        "itc": frame([(y, "solar", s) for y, s in sec_year], ["year", "tech", "sector_abbr"],
                     itc_fraction_of_capex=u(0.0, 0.3)),
        "load_growth": frame([k for k in sc_year if k[1:] not in (("com", 13), ("res", 12))],
                             ["year", "sector_abbr", "county_id"], load_multiplier=u(0.8, 1.4)),
        "elec_price": frame([k for k in sc_year if k[1:] != ("res", 14)], ["year", "sector_abbr", "county_id"],
                            elec_price_multiplier=u(0.7, 1.6)),
        "vor": frame([(st, s) for st in STATES for s in SECTORS if (st, s) != ("BB", "ind")],
                     ["state_abbr", "sector_abbr"], value_of_resiliency_usd=u(0, 5000)),
    }
    if wholesale:
        T["wholesale_row"] = {(c, y): 3 * i + j for i, c in enumerate(COUNTIES[:4]) for j, y in enumerate(YEARS)
                              if (c, y) != (12, 2040)}
    return T


def _year_frame(n):
    rng = np.random.default_rng(100 + n)
    pick = lambda vals: [vals[i] for i in rng.integers(0, len(vals), n)]
    f = pd.DataFrame({"agent_id": np.arange(n) + 5000, "state_abbr": pick(STATES), "sector_abbr": pick(SECTORS),
                      "county_id": pick(COUNTIES), "tech": ["solar"] * n,
                      "load_kwh_per_customer_in_bin_initial": rng.uniform(3e3, 9e5, n),
                      "customers_in_bin_initial": rng.uniform(1, 900, n),
                      "load_kwh_in_bin_initial": rng.uniform(1e4, 9e7, n)})
    if n >= 255:        # every hole is hit at the sizes that can hold them
        f.loc[:6, "sector_abbr"] = ["ind", "com", "res", "ind", "res", "com", "res"]
        f.loc[:6, "county_id"] = [11, 13, 14, 15, 15, 12, 12]
        f.loc[:6, "state_abbr"] = ["BB", "AA", "AA", "AA", "BB", "BB", "AA"]
    return f


def _merged_reference(frame, T, year, inflation):
    """The year's attribute columns as the chain of left merges that builds
    them (apply_load_growth, the price multiplier and escalator, pv tech, pv
    prices, pv + battery prices, value of resiliency, financing and ITC,
    wholesale prices), in that order on one frame."""
    df = frame.copy()
    df["year"] = year
    df = pd.merge(df, T["load_growth"], how="left", on=["year", "sector_abbr", "county_id"])
    res = df["sector_abbr"] == "res"
    df["load_kwh"] = np.where(res, df["load_kwh_per_customer_in_bin_initial"] * df["load_multiplier"],
                              df["load_kwh_per_customer_in_bin_initial"])
    df["customers_in_bin"] = np.where(~res, df["customers_in_bin_initial"] * df["load_multiplier"],
                                      df["customers_in_bin_initial"])
    df["load_kwh_in_bin"] = df["load_kwh_in_bin_initial"] * df["load_multiplier"]
    traj = T["elec_price"]
    mult = traj[traj["year"] == year].reset_index(drop=True)
    cap = min(year, 2040)
    esc = traj[traj["year"] == cap].reset_index(drop=True)
    last = int(traj["year"].max())
    esc["final"] = traj[traj["year"] == last].reset_index(drop=True)["elec_price_multiplier"]
    esc["escalator"] = np.clip((esc["final"] / esc["elec_price_multiplier"]) ** (1.0 / (last - cap)) - 1.0, -.01, .01)
    df = pd.merge(df, mult[["elec_price_multiplier", "sector_abbr", "county_id"]].rename(
        columns={"elec_price_multiplier": "price_mult"}), how="left", on=["sector_abbr", "county_id"])
    df = pd.merge(df, esc[["sector_abbr", "county_id", "escalator"]], how="left", on=["sector_abbr", "county_id"])
    df = pd.merge(df, T["pv_tech"].rename(columns={"pv_degradation_factor": "pv_deg"}), how="left",
                  on=["sector_abbr", "year"])
    df = pd.merge(df, T["pv_price"].rename(columns={"system_capex_per_kw": "capex"}), how="left",
                  on=["sector_abbr", "year"])
    df = pd.merge(df, T["pv_plus_batt_price"].rename(columns={"system_capex_per_kw": "capex_combined",
                                                              "batt_capex_per_kwh": "batt_capex_kwh"}),
                  how="left", on=["year", "sector_abbr"])
    df = df.merge(T["vor"].rename(columns={"value_of_resiliency_usd": "vor"}), how="left",
                  on=["state_abbr", "sector_abbr"])
    df = df.merge(T["financing"].rename(columns={"economic_lifetime_yrs": "econ_life", "loan_term_yrs": "loan_term",
                                                 "down_payment_fraction": "down_payment",
                                                 "real_discount_rate": "real_discount"}),
                  how="left", on=["year", "sector_abbr"])
    df = df.merge(T["itc"].rename(columns={"itc_fraction_of_capex": "itc_frac"}), how="left",
                  on=["year", "tech", "sector_abbr"])
    df["inflation"] = inflation
    if "wholesale_row" in T:
        w = pd.DataFrame([(c, y, r) for (c, y), r in T["wholesale_row"].items()],
                         columns=["county_id", "year", "wholesale_row"])
        df = pd.merge(df, w, how="left", on=["county_id", "year"])
    assert len(df) == len(frame) and df["agent_id"].tolist() == frame["agent_id"].tolist()
    out = {k: df[k].to_numpy(dtype=np.float64) for k in gm.YEAR_OUT_F64 + gm.YEAR_OUT_LOOP}
    for k in gm.YEAR_OUT_I32:
        if k in df:
            out[k] = df[k].fillna(-1).to_numpy(dtype=np.int64)
    return out


def _gather(engine, yi, year, cols):
    """dgen_year_inputs on YearTables.compile(year)'s tables, as YearInputs.apply
    passes them -- without its host check of the financing terms, which refuses
    a financing merge miss before the kernel would see it."""
    L = gm._bind(engine.lib)
    yt = yi.yt
    keep = {k: torch.as_tensor(v, device=engine.dev) for k, v in yt.compile(year).items() if v is not None}
    ws = "wholesale_row" in keep
    tc = gm.YearTablesC(by_sector=keep["by_sector"].data_ptr(), by_sector_county=keep["by_sector_county"].data_ptr(),
                        by_state_sector=keep["by_state_sector"].data_ptr(),
                        wholesale_row=keep["wholesale_row"].data_ptr() if ws else None,
                        n_sector=len(yt.sectors), n_sector_county=len(yt.sector_counties),
                        n_state_sector=len(yt.state_sectors), n_county=len(yt.counties) if ws else 0,
                        inflation_rate=yt.inflation_rate)
    ptr = {k: v.data_ptr() for k, v in cols.items()}
    if not ws:
        ptr["wholesale_row"] = None
    out = gm.YearOut(**ptr)
    _lib.check(L.dgen_year_inputs(engine.ctx, ctypes.byref(yi.keys), ctypes.byref(tc), ctypes.byref(out),
                                  len(yt.k_sector), engine.stream_handle()), "dgen_year_inputs")
    torch.cuda.synchronize(engine.dev)


@pytest.mark.parametrize("wholesale", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_year_inputs_with_merge_misses(engine, n, wholesale):
    frame, T = _year_frame(n), _year_tables(wholesale)
    yt = gm.YearTables(frame, T, 0.025)
    yi = gm.YearInputs(engine, yt, frame["load_kwh_per_customer_in_bin_initial"].to_numpy(),
                       frame["customers_in_bin_initial"].to_numpy(), frame["load_kwh_in_bin_initial"].to_numpy())
    dev = engine.dev
    cols = {k: torch.full((n + 1,), -7.0, dtype=torch.float64, device=dev)
            for k in gm.YEAR_OUT_F64 + gm.YEAR_OUT_LOOP}
    cols.update({k: torch.full((n + 1,), -7, dtype=torch.int32, device=dev) for k in gm.YEAR_OUT_I32})
    if n >= 255:        # the yearly driver refuses the financing miss on the host
        with pytest.raises(ValueError, match="financing terms"):
            yi.apply(YEARS[0], cols, cols)
    missed = set()
    for year in YEARS:
        _gather(engine, yi, year, cols)
        got = {k: v.cpu().numpy() for k, v in cols.items()}
        ref = _merged_reference(frame, T, year, 0.025)
        for k, g in got.items():
            assert g[n] == -7, (year, k)                                   # one past the last agent
            if k == "wholesale_row" and not wholesale:
                assert (g == -7).all(), year                               # no map: the column is left alone
                continue
            if g.dtype.kind == "i":
                assert np.array_equal(g[:n], ref[k]), (year, k)
            else:
                assert _same(g[:n], ref[k]), (year, k)
        missed |= {k for k in gm.YEAR_OUT_F64 + gm.YEAR_OUT_LOOP if np.isnan(ref[k]).any()}
        missed |= {k for k in gm.YEAR_OUT_I32 if k in ref and (ref[k] < 0).any()}
    if n >= 255:        # the holes were all reached: a miss in every table
        assert missed >= {"capex", "down_payment", "real_discount", "tax_rate", "econ_life", "loan_term",
                          "load_kwh", "customers_in_bin", "load_kwh_in_bin", "price_mult", "escalator", "vor"}
        assert not wholesale or "wholesale_row" in missed
        assert not missed & {"capex_combined", "batt_capex_kwh", "pv_deg", "itc_frac", "inflation"}
        # both sides of the load-growth product are present and differ
        res = (frame["sector_abbr"] == "res").to_numpy()
        assert (ref["customers_in_bin"][res] == frame["customers_in_bin_initial"].to_numpy()[res]).all()
        ok = ~res & ~np.isnan(ref["customers_in_bin"])
        assert ok.any() and (ref["customers_in_bin"][ok] != frame["customers_in_bin_initial"].to_numpy()[ok]).all()


# ---------------------------------------------------------------- initial shares
def _seed_direct(engine, c, sentinel=-7.25):
    """dgen_initial_market_shares on sentinel-filled outputs one entry longer
    than needed (device order = c['dev_index'])."""
    L = gm._bind(engine.lib)
    n = len(c["state"])
    perm, seg_off, uniq = group_order(list(zip(c["state"], c["sector"], c["tech"])))
    cap = gm._lookup(pd.DataFrame(c["caps"]), ["state_abbr", "sector_abbr"], [(s, x) for s, x, _ in uniq],
                     list(mr.CAP_COLS), "caps")
    dev = engine.dev
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    scatter = np.empty(n, dtype=np.int64)
    scatter[c["dev_index"]] = np.arange(n)                       # device row -> frame row
    w, cx = put(c["weight"][scatter]), put(c["capex"][scatter])
    idx, seg, caps = put(c["dev_index"][perm]), put(np.asarray(seg_off, np.int64)), put(cap)
    out = {k: torch.full((n + 1,), sentinel, dtype=torch.float64, device=dev) for k in gm.INIT_OUT}
    out["developable_customers_in_state"] = torch.full((len(uniq) + 1,), sentinel, dtype=torch.float64, device=dev)
    out["agent_count"] = torch.full((len(uniq) + 1,), -7, dtype=torch.int64, device=dev)
    ci = gm.InitIn(developable_agent_weight=w.data_ptr(), system_capex_per_kw=cx.data_ptr())
    co = gm.InitOut(**{k: v.data_ptr() for k, v in out.items()})
    _lib.check(L.dgen_initial_market_shares(engine.ctx, ctypes.byref(ci), ctypes.byref(co), idx.data_ptr(),
                                            seg.data_ptr(), caps.data_ptr(), len(uniq), engine.stream_handle()),
               "dgen_initial_market_shares")
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}, uniq, (w, cx)


def test_initial_market_shares_at_group_edges(engine):
    c = mr.initial_shares_case()
    n = len(c["state"])
    di = c["dev_index"]
    ref = om.initial_market_shares(c["state"], c["sector"], c["tech"], c["weight"], c["capex"], c["caps"])
    _, tot, cnt = mr.initial_shares_pandas(c)
    got, uniq, (w, cx) = _seed_direct(engine, c)
    for k in gm.INIT_OUT:
        assert got[k][n] == -7.25, k
        assert _same(got[k][di], ref[k]), k                    # device row dev_index[i] holds frame row i
    G = len(uniq)
    assert G == len(mr.INIT_GROUPS)
    assert got["developable_customers_in_state"][G] == -7.25 and got["agent_count"][G] == -7
    for g, key in enumerate(uniq):
        assert got["developable_customers_in_state"][g] == tot.loc[key], key
        assert got["agent_count"][g] == cnt.loc[key], key
    kind = c["kind"]
    assert np.isposinf(got["adopters_cum_last_year"][di][kind == "all_nan"]).all()
    # the package's wrapper on the same device columns: the same bits
    out = gm.initial_market_shares(engine, c["state"], c["sector"], c["tech"], w, cx, pd.DataFrame(c["caps"]),
                                   dev_index=di)
    assert out["groups"] == uniq
    for k in gm.INIT_OUT + ["developable_customers_in_state"]:
        assert _same(out[k].cpu().numpy(), got[k][:-1]), k
    assert np.array_equal(out["agent_count"].cpu().numpy(), got["agent_count"][:-1])


# -------------------------------------------------------------- max market share
def _curves(kind):
    """'wide': res 0.0-3.0 (no row at 1.3, a NaN share at 0.7), com 0.5-4.0, ind
    without a curve; a third-party-owned row at 5.0 widens the clip range and a
    row of another metric is ignored.  'late': every curve starts at 0.4."""
    rows = []
    add = lambda s, pb, v, bm="host_owned", metric="payback_period": rows.append(
        dict(metric=metric, business_model=bm, sector_abbr=s, payback_period=pb, max_market_share=v))
    if kind == "wide":
        for f in range(0, 31):
            if f != 13:
                add("res", f / 10.0, np.nan if f == 7 else 0.9 - 0.02 * f)
        for f in range(5, 41):
            add("com", f / 10.0, 0.8 - 0.015 * f)
        add("res", 5.0, 0.01, bm="tpo")
        add("res", 30.0, 0.5, metric="percent_monthly_bill_savings")
    else:
        for s, top in (("res", 25), ("com", 33), ("ind", 40)):
            for f in range(4, top + 1):
                add(s, f / 10.0, 0.7 - 0.01 * f + 0.001 * len(s))
    return pd.DataFrame(rows)


PAYBACKS = [np.nan, np.inf, -np.inf, -2.0, 0.0, 0.39, 0.4, 99.0, 0.25, 0.75, 1.25, 3.75, 0.15, 0.35, 2.675,
            0.65, 0.7, 0.74, 1.3, 1.34, 2.96, 3.0, 3.04, 3.3, 4.0, 4.04, 4.96, 5.0, 0.45, 0.55, 2.5, 1.0]


@pytest.mark.parametrize("curve", ["wide", "late"])
@pytest.mark.parametrize("n", SIZES)
def test_max_market_share_bounded_factor_and_share(engine, n, curve):
    mdf = _curves(curve)
    rng = np.random.default_rng(n)
    reps = -(-n // (3 * len(PAYBACKS)))
    pb = np.array((PAYBACKS * 3 * reps)[:n])
    sector = [s for s in ("res", "com", "ind") for _ in PAYBACKS] * reps
    sector = sector[:n]
    if n > 3 * len(PAYBACKS):
        tail = slice(3 * len(PAYBACKS), n)
        pb[tail] = np.round(rng.uniform(-1, 6, n - tail.start), 2)         # two decimals: ties included
    tab, rows, fmin, min_pb, max_pb = gd.mms_table(mdf)
    assert np.isfinite([min_pb, max_pb]).all()
    assert (fmin, min_pb, max_pb) == ((0, 0.0, 5.0) if curve == "wide" else (40, 0.4, 4.0))
    row = np.array([rows.get(s, -1) for s in sector], dtype=np.int32)
    b, f, m = gd.max_market_share_arrays(engine, pb, row, tab, fmin, min_pb, max_pb)
    host = mdf[(mdf.metric == "payback_period") & (mdf.business_model == "host_owned")]
    rb, rf, rm = od.max_market_share(pb, sector, host["sector_abbr"].tolist(), host["payback_period"].to_numpy(),
                                     host["max_market_share"].to_numpy(),
                                     mdf.loc[mdf.metric == "payback_period", "payback_period"].to_numpy())
    assert b.dtype == np.float64 and f.dtype == np.int64 and m.dtype == np.float64
    assert _same(b, rb) and not np.isnan(b).any()
    assert np.array_equal(f, rf.astype(np.int64))
    assert _same(m, rm)
    if n >= 3 * len(PAYBACKS) and curve == "wide":
        k = {v: i for i, v in enumerate(PAYBACKS) if v == v}
        assert [b[k[v]] for v in (0.25, 0.75, 1.25, 3.75)] == [0.2, 0.8, 1.2, 3.8]       # half to even
        assert [b[k[v]] for v in (0.15, 0.35, 2.675)] == [0.2, 0.4, 2.7]       # x * 10 rounds to a tie or past it
        assert b[0] == 0.0 and b[1] == 5.0 and b[2] == 0.0                              # NaN, +inf, -inf
        P = len(PAYBACKS)
        assert np.isnan(m[2 * P:3 * P]).all()                                           # ind: no curve
        assert np.isnan(m[k[0.7]]) and np.isnan(m[k[1.3]]) and np.isfinite(m[k[1.25]])  # the two gaps of res
        assert np.isnan(m[k[3.3]]) and np.isfinite(m[P + k[3.3]])                       # past res, inside com
        assert np.isfinite(m[k[0.25]]) and np.isnan(m[P + k[0.25]])                     # before com starts
        assert np.isnan(m[P + k[99.0]])                                                 # clipped to 5.0: no curve there


def test_calc_max_market_share_uses_the_same_arrays(engine):
    mdf = _curves("wide")
    df = pd.DataFrame({"agent_id": np.arange(3 * len(PAYBACKS)),
                       "sector_abbr": [s for s in ("res", "com", "ind") for _ in PAYBACKS],
                       "payback_period": PAYBACKS * 3}).set_index("agent_id")
    out = gd.calc_max_market_share(df, mdf, engine=engine)
    tab, rows, fmin, lo, hi = gd.mms_table(mdf)
    row = np.array([rows.get(s, -1) for s in df["sector_abbr"]], dtype=np.int32)
    _, _, m = gd.max_market_share_arrays(engine, df["payback_period"].to_numpy(), row, tab, fmin, lo, hi)
    assert list(out.columns) == ["sector_abbr", "payback_period", "max_market_share", "metric"]
    assert _same(out["max_market_share"].to_numpy(), m)


# ---------------------------------------------------------------------- diffusion
def _diff_cols(a):
    return dict(zip(gd.DIFF_IN, (a[k] for k in mr.DIFF_ARGS)))


assert gd.DIFF_IN == ["max_market_share", "market_share_last_year", "bass_p", "bass_q", "teq_yr1",
                      "developable_agent_weight", "system_kw", "system_capex_per_kw", "adopters_cum_last_year",
                      "market_value_last_year", "system_kw_cum_last_year"]           # mr.DIFF_ARGS order
assert tuple(gd.DIFF_OUT) == mr.DIFF_OUT

ONE_DOWN = 1.0 - 2.0 ** -53
# name -> (mms, msly, p, q, teq_yr1, weight)
SELECTION = {
    "plain": (0.4, 0.1, 0.004, 0.35, 2.0, 50.0),
    "mms_zero": (0.0, 0.0, 0.004, 0.35, 2.0, 50.0),
    "mms_zero_share_above": (0.0, 0.02, 0.004, 0.35, 2.0, 50.0),          # also msly > mfix = 1e-9
    "mms_zero_share_below": (0.0, 2.5e-10, 0.004, 0.35, 2.0, 50.0),       # ratio 0.25 of the 1e-9 floor
    "share_above_cap": (0.3, 0.45, 0.004, 0.35, 2.0, 50.0),               # msly > mfix and ms > mms
    "share_at_cap": (0.3, 0.3, 0.004, 0.35, 2.0, 50.0),                   # log(0): teq inf, f 0, naf 1
    "share_at_floor": (0.0, 1e-9, 0.004, 0.35, 2.0, 50.0),                # msly == mfix with mms == 0
    "nan_cap": (np.nan, 0.1, 0.004, 0.35, 2.0, 50.0),
    "nan_share": (0.4, np.nan, 0.004, 0.35, 2.0, 50.0),
    "nan_both": (np.nan, np.nan, 0.004, 0.35, 2.0, 50.0),
    "zero_weight": (0.4, 0.1, 0.004, 0.35, 2.0, 0.0),
    "zero_share": (0.4, 0.0, 0.004, 0.35, 2.0, 50.0),
    # ms == mms exactly with msly below it: naf rounds to 1.0 (first year: a
    # long first step; later: ratio one ulp under 1 and p + q large), so the
    # cap test ms > mms is False and the new share is mms - msly, not 0
    "saturated_first": (0.4, 0.1, 0.004, 0.35, 1e4, 50.0),
    "saturated_later": (0.4, 0.4 * ONE_DOWN, 0.3, 0.9, 1e4, 50.0),
    "negative_weight": (0.4, 0.1, 0.004, 0.35, 2.0, -3.0),
}


def _selection_args(n):
    rng = np.random.default_rng(3)
    base = np.array(list(SELECTION.values()), dtype=np.float64)
    reps = -(-n // len(base))
    b = np.tile(base, (reps, 1))[:n]
    a = dict(mms=b[:, 0], msly=b[:, 1], p=b[:, 2], q=b[:, 3], teq_yr1=b[:, 4], dev_w=b[:, 5],
             system_kw=rng.uniform(2.0, 300.0, n), capex=rng.uniform(900.0, 3500.0, n),
             adopt_ly=rng.uniform(0.0, 40.0, n), mv_ly=rng.uniform(0.0, 1e6, n), skc_ly=rng.uniform(0.0, 900.0, n))
    return {k: a[k] for k in mr.DIFF_ARGS}


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("n", SIZES)
def test_diffusion_selection_and_propagation(engine, n, first):
    a = _selection_args(n)
    got = gd.diffusion_arrays(engine, _diff_cols(a), first)
    with np.errstate(all="ignore"):
        ref = od.diffusion(*[a[k] for k in mr.DIFF_ARGS], first)
    msly, mms = a["msly"], a["mms"]
    for k in gd.DIFF_OUT:
        g, r = got[k], np.asarray(ref[k], dtype=np.float64)
        assert g.shape == (n,)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin), k
        assert _same(g[~fin], r[~fin]), k                                   # NaN / +inf / -inf alike
        assert np.array_equal(g[fin] == 0, r[fin] == 0), k                  # exact zeros alike
        assert np.allclose(g[fin], r[fin], rtol=1e-12, atol=0.0), k
    for k in ("mms_fix_zeros", "ratio"):
        assert _same(got[k], ref[k]), k
    for k in ("diffusion_market_share", "market_share"):                    # where-selected: copied bits
        for src in (msly, mms):
            sel = np.asarray(ref[k]) == src
            assert np.array_equal(got[k][sel], src[sel]), k
    zeroed = np.asarray(ref["market_share"]) > mms
    assert not got["new_market_share"][zeroed].any() and zeroed.any() == (n >= len(SELECTION))
    exact = np.asarray(ref["market_share"] == mms) | np.asarray(ref["market_share"] == msly)
    assert _same(got["new_market_share"][exact], np.asarray(ref["new_market_share"])[exact])
    if n >= len(SELECTION):
        i = {name: j for j, name in enumerate(SELECTION)}
        at = i["share_at_cap"]
        assert got["bass_params_teq"][at] == np.inf and got["f"][at] == 0.0 and got["new_adopt_fraction"][at] == 1.0
        sat = i["saturated_first" if first else "saturated_later"]
        assert got["market_share"][sat] == mms[sat] and got["new_market_share"][sat] == mms[sat] - msly[sat] > 0
        assert np.isnan(got["market_share"][i["nan_share"]])                # np.maximum, not fmax
        assert got["bass_market_share"][i["nan_share"]] != got["bass_market_share"][i["nan_share"]]
        assert got["mms_fix_zeros"][i["mms_zero"]] == 1e-9 and got["ratio"][i["mms_zero_share_above"]] == 0.0
        assert got["ratio"][i["mms_zero_share_below"]] == 0.25
        assert got["new_adopters"][i["zero_weight"]] == 0.0 and got["new_market_share"][i["zero_weight"]] > 0


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_diffusion_well_conditioned_block(engine, first):
    a = mr.diffusion_well()
    got = gd.diffusion_arrays(engine, _diff_cols(a), first)
    ref = od.diffusion(*[a[k] for k in mr.DIFF_ARGS], first)
    for k in gd.DIFF_OUT:
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=0.0), k
    for k in ("mms_fix_zeros", "ratio"):
        assert _same(got[k], ref[k]), k


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("kind", ["slow", "near"])
def test_diffusion_ill_conditioned_block_vs_mpmath(engine, kind, first):
    a = mr.diffusion_ill(kind)
    got = gd.diffusion_arrays(engine, _diff_cols(a), first)
    ref = mr.diffusion_mp(a, first)
    tol = mr.ill_tolerance(kind, first)
    oerr = mr.oracle_error(kind, first)
    bad = {}
    for k in gd.DIFF_OUT:
        assert np.isfinite(got[k]).all(), k
        err = mr.max_rel_err(got[k], ref[k])
        print(f"{kind} {'first' if first else 'later'} {k}: oracle {oerr[k]:.2e} device {err:.2e} "
              f"tolerance {tol[k]:.2e} device/tolerance {err / tol[k]:.3f}")
        if not err <= tol[k]:
            bad[k] = (err, tol[k])
    assert not bad, bad


# ----------------------------------------------------------------- export weights
def _weights_case(n):
    """customers, adopters, last year's battery kW, battery kW, added."""
    rows = [
        (100.0, 7.0, 12.0, 0.0, 1),            # batt_kw == 0: the eps denominator, 1.2e10 systems
        (100.0, 7.0, 0.0, 0.0, 2),             # 0 / eps
        (100.0, 7.0, -12.0, 4.0, 1),           # negative cumulative: clamps to 0 before rounding
        (100.0, 7.0, -12.0, 0.0, 0),
        (100.0, 7.0, 12.0, -4.0, 1),           # negative kW: max(., eps) keeps the eps
        (100.0, 7.0, 3e-10, 2e-10, 0),         # kW below eps
        (100.0, 9.0, 10.0, 4.0, 0),            # quotient 2.5 -> 2
        (100.0, 9.0, 14.0, 4.0, 0),            # quotient 3.5 -> 4
        (100.0, 2.5, 0.0, 4.0, 0),             # adopters at .5: 2
        (100.0, 3.5, 0.0, 4.0, 0),             # 4
        (100.0, 0.5, 0.0, 4.0, 0),             # 0
        (np.nan, 7.0, 8.0, 4.0, 1),            # NaN customers stay NaN
        (5.0, 7.0, 8.0, 4.0, 1),               # fewer customers than adopters: 0
        (100.0, 7.0, 8.0, 4.0, 50),            # added past the adopters: PV-only clamps to 0
        (100.0, 7.0, 8.0, 4.0, -9),            # a negative correction: battery count clamps to 0
        (100.0, 1e15 + 0.5, 8.0, 4.0, 3),
    ]
    rng = np.random.default_rng(n)
    t = np.array((rows * (-(-n // len(rows))))[:n], dtype=np.float64)
    if n > len(rows):
        k = n - len(rows)
        bkw = np.where(rng.random(k) < 0.2, 0.0, rng.integers(1, 9, k) * 0.5)
        t[len(rows):, 0] = rng.uniform(0, 300, k)
        t[len(rows):, 1] = rng.integers(0, 80, k) * 0.5
        t[len(rows):, 2] = rng.integers(-4, 30, k) * 0.25
        t[len(rows):, 3] = bkw
        t[len(rows):, 4] = rng.integers(-2, 12, k)
    return t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4].astype(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_export_weights_edges(engine, n):
    cust, adopt, cum, kw, added = _weights_case(n)
    got = torch.stack(ga.export_weights(engine, cust, adopt, cum, kw, added)).cpu().numpy()
    ref = oa.weights(cust, adopt, cum, kw, added)
    assert got.shape == (3, n)
    assert _same(got, ref)
    assert np.array_equal(np.isnan(got[2]), np.isnan(cust)) and np.isfinite(got[:2]).all()
    if n >= 16:
        assert got[1, 0] == 12e9 + 1 and got[1, 2] == 1 and got[1, 4] == 12e9 + 1
        assert (got[1, 6], got[1, 7]) == (2.0, 4.0) and (got[0, 8], got[0, 9], got[0, 10]) == (2.0, 4.0, 0.0)
        assert np.isnan(got[2, 11]) and got[2, 12] == 0.0 and got[0, 13] == 0.0 and got[1, 14] == 0.0
