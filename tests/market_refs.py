"""Plain references and shared inputs for the profile-prep kernels
(k_row_pairwise_*, k_row_slots_*) and the market-step kernels (k_initial_shares,
k_diffusion).  CPU only: tests/test_gpu_prep.py and
tests/test_gpu_market_edges.py compare the device against it,
tests/test_market_refs.py checks on the same inputs that the references are
what they claim and that the data tells a wrong kernel from a right one.

Nothing here is imported from the package under test: the calendar is written
out from a Monday start and 365 days, the summation order from numpy's
pairwise sum (numpy/_core/src/umath/loops_utils.h.src) and its 8192-element
reduction buffer, the diffusion step from its formulas in mpmath.
"""
from __future__ import annotations

import functools

import numpy as np

NH = 8760
NSLOT = 576
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# ------------------------------------------------------------------- calendar
MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)        # non-leap


@functools.lru_cache(maxsize=None)
def slot_days():
    """slot -> the days d (0-based, ascending) whose hour d*24 + hod it sums:
    slot = month*48 + daytype*24 + hod, day 0 a Monday, daytype 1 = d % 7 >= 5."""
    assert sum(MONTH_DAYS) * 24 == NH
    out, start = [], 0
    for nd in MONTH_DAYS:
        for dt in (0, 1):
            days = [d for d in range(start, start + nd) if (d % 7 >= 5) == bool(dt)]
            out.extend([days] * 24)
        start += nd
    assert len(out) == NSLOT
    return out


def slot_day_counts():
    return np.array([len(d) for d in slot_days()], dtype=np.int64)


def slot_sums(rows64):
    """[R, 576] float64: per slot the float64 sum, from 0.0, of v[d*24 + hod]
    over the slot's days in ascending order."""
    rows64 = np.asarray(rows64, dtype=np.float64)
    days = slot_days()
    hod = np.arange(NSLOT) % 24
    depth = max(len(d) for d in days)
    acc = np.zeros((rows64.shape[0], NSLOT))
    for k in range(depth):
        have = np.array([len(d) > k for d in days])
        idx = np.array([d[k] * 24 if len(d) > k else 0 for d in days]) + hod
        acc = np.where(have[None, :], acc + rows64[:, idx], acc)
    return acc


# ------------------------------------------------------------ numpy-order sum
def _pw(a, off, n):
    """numpy's pairwise sum of a[:, off:off+n] (columns at once)."""
    if n < 8:
        res = np.zeros(a.shape[0])      # never reached from 8760 = 8192 + 568
        for i in range(n):
            res = res + a[:, off + i]
        return res
    if n <= 128:
        r = [a[:, off + j].copy() for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[:, off + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + a[:, off + i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pw(a, off, n2) + _pw(a, off + n2, n - n2)


def np_order_sum(rows64, chunk=8192):
    """Row sums in the order the kernel states: chunks of `chunk` elements added
    in sequence to 0.0, each chunk a pairwise split rounded down to 8 with
    8-accumulator leaves of at most 128.  chunk=None: one pairwise sum of the
    whole row (what numpy would do without its reduction buffer)."""
    a = np.asarray(rows64, dtype=np.float64)
    n = a.shape[1]
    if chunk is None:
        return _pw(a, 0, n)
    res = np.zeros(a.shape[0])
    for s in range(0, n, chunk):
        res = res + _pw(a, s, min(chunk, n - s))
    return res


# --------------------------------------------------------------- prep inputs
SHAPE_SPECIAL = ("zeros", "hour0", "hour8191", "hour8192", "hour8759", "ones", "index")
SINGLE_HOURS = (0, 8191, 8192, 8759)


def adversarial_rows(n, seed):
    """float32 [n, 8760]: signed, twelve decades: standard_normal * 10**U(-6, 6)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, NH)) * 10.0 ** rng.uniform(-6, 6, (n, NH))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def shape_rows(R):
    """float32 [R, 8760] (read-only).  Row 0 and every row past 7 are
    adversarial_rows; rows 1..7 (where R allows) are SHAPE_SPECIAL in order."""
    rows = adversarial_rows(R, 1000 + R)
    for k, name in enumerate(SHAPE_SPECIAL, start=1):
        if k >= R:
            break
        rows[k] = 0.0
        if name.startswith("hour"):
            rows[k, int(name[4:])] = 3.25
        elif name == "ones":
            rows[k] = 1.0
        elif name == "index":
            rows[k] = np.arange(NH, dtype=np.float32)           # exact below 2**24
    rows.setflags(write=False)
    return rows


def shape_positive_rows(R):
    """Rows of shape_rows(R) with no negative value and a positive sum."""
    return [k for k, name in enumerate(SHAPE_SPECIAL, start=1) if k < R and name != "zeros"]


CF_KINDS = ("extremes", "unit", "signed", "huge")


@functools.lru_cache(maxsize=None)
def cf_rows(R):
    """int32 [R, 8760] (read-only), row r of kind CF_KINDS[r % 4]: the whole
    int32 range with INT32_MIN / INT32_MAX at the chunk and row edges; the
    production range [0, 1e6]; negatives; |x| > 2e7."""
    rng = np.random.default_rng(2000 + R)
    rows = np.empty((R, NH), dtype=np.int32)
    for r in range(R):
        kind = CF_KINDS[r % 4]
        if kind == "extremes":
            v = rng.integers(INT32_MIN, INT32_MAX, NH, endpoint=True)
            v[[0, 8192]] = INT32_MIN
            v[[8191, 8759]] = INT32_MAX
        elif kind == "unit":
            v = rng.integers(0, 1_000_000, NH, endpoint=True)
            v[rng.random(NH) < 0.45] = 0                        # nights
        elif kind == "signed":
            v = rng.integers(-1_000_000, 1_000_000, NH, endpoint=True)
        else:
            v = rng.integers(20_000_001, INT32_MAX, NH, endpoint=True) * rng.choice([-1, 1], NH)
        rows[r] = v
    rows.setflags(write=False)
    return rows


def cf_positive_rows(R):
    return [r for r in range(R) if CF_KINDS[r % 4] == "unit"]


# ------------------------------------------------------------ Kahan group sum
def kahan_weights(m):
    """m >= 2 weights on which pandas' compensated group sum and the plain
    sequential sum differ: 1e8, then 1e-8 (above half an ulp of 1e8, 2**-27,
    so every plain add rounds up to a whole ulp, 1.49e-8, instead of 1e-8)."""
    w = np.full(m, 1e-8)
    w[0] = 1e8
    return w


def seq_sum(values):
    s = 0.0
    for v in values:
        if v == v:
            s = s + float(v)
    return s


# ---------------------------------------------------- diffusion step in mpmath
DIFF_OUT = ("mms_fix_zeros", "ratio", "bass_params_teq", "teq2", "f", "new_adopt_fraction",
            "bass_market_share", "diffusion_market_share", "market_share", "new_market_share",
            "new_adopters", "new_market_value", "new_system_kw", "number_of_adopters",
            "market_value", "system_kw_cum")
DIFF_ARGS = ("mms", "msly", "p", "q", "teq_yr1", "dev_w", "system_kw", "capex", "adopt_ly", "mv_ly", "skc_ly")


def diffusion_mp(args, first, digits=50):
    """The diffusion step (calc_equiv_time, bass_diffusion, the market-share
    floor and cap, the cumulative updates) on finite float64 inputs, every
    operation in mpmath at `digits` digits.  args: DIFF_ARGS -> arrays.
    Returns DIFF_OUT -> list of mpf."""
    import mpmath as mp
    out = {k: [] for k in DIFF_OUT}
    with mp.workdps(digits):
        cols = [[mp.mpf(float(x)) for x in args[k]] for k in DIFF_ARGS]
        for mms, msly, p, q, t1, w, skw, capex, a_ly, mv_ly, skc_ly in zip(*cols):
            mfix = mp.mpf(1e-9) if mms == 0 else mms
            ratio = mp.mpf(0) if msly > mfix else msly / mfix
            teq = mp.log((1 - ratio) / (1 + ratio * (q / p))) / (-1 * (p + q))
            teq2 = teq + t1 if first else teq + 2
            f = mp.exp(-1 * (p + q) * teq2)
            naf = (1 - f) / (1 + (q / p) * f)
            bms = mms * naf
            dms = msly if msly > bms else bms
            ms = dms if dms > msly else msly
            nms = mp.mpf(0) if ms > mms else ms - msly
            na = nms * w
            nmv = na * skw * capex
            nskw = na * skw
            for k, v in zip(DIFF_OUT, (mfix, ratio, teq, teq2, f, naf, bms, dms, ms, nms, na, nmv, nskw,
                                       a_ly + na, mv_ly + nmv, skc_ly + nskw)):
                out[k].append(v)
    return out


def max_rel_err(values, ref_mp, digits=50):
    """max over entries of |v - ref| / |ref| (v float64, ref mpf); an entry whose
    reference is 0 must be 0 itself (else inf)."""
    import mpmath as mp
    worst = 0.0
    with mp.workdps(digits):
        for v, r in zip(values, ref_mp):
            v = mp.mpf(float(v))
            if r == 0:
                e = 0.0 if v == 0 else float("inf")
            else:
                e = float(abs(v - r) / abs(r))
            worst = max(worst, e)
    return worst


def _diff_common(n, rng):
    return dict(teq_yr1=rng.uniform(1.0, 3.0, n), dev_w=rng.uniform(1.0, 500.0, n),
                system_kw=rng.uniform(2.0, 300.0, n), capex=rng.uniform(900.0, 3500.0, n),
                adopt_ly=rng.uniform(0.0, 40.0, n), mv_ly=rng.uniform(0.0, 1e6, n),
                skc_ly=rng.uniform(0.0, 900.0, n))


@functools.lru_cache(maxsize=None)
def diffusion_well(n=257):
    """The golden fixture's ranges: p <= 0.01, q in 0.2-0.5, ratio 0.02-0.9."""
    rng = np.random.default_rng(31)
    mms = rng.uniform(0.05, 0.9, n)
    a = dict(mms=mms, msly=mms * rng.uniform(0.02, 0.9, n), p=rng.uniform(5e-4, 0.01, n),
             q=rng.uniform(0.2, 0.5, n), **_diff_common(n, rng))
    return {k: a[k] for k in DIFF_ARGS}


@functools.lru_cache(maxsize=None)
def diffusion_ill(kind, n=64):
    """'slow': p + q from 1e-6 to 1e-3 (log-uniform), ratio 0.05-0.9.
    'near': the fixture's p and q, msly = mms * (1 - d), d from 1e-12 to 1e-9,
    so 1 - ratio cancels to 1e-4 .. 1e-7 relative in float64.
    The two are not combined: with both at once a year's growth, about
    2 (p + q)(1 - ratio) = 2e-18 of the share, is below half an ulp of the
    share, so new_market_share is 0 or one ulp in any float64 evaluation and a
    relative error against the 50-digit value says nothing."""
    rng = np.random.default_rng({"slow": 41, "near": 43}[kind])
    mms = rng.uniform(0.05, 0.9, n)
    if kind == "slow":
        s = 10.0 ** rng.uniform(-6, -3, n)
        s[0] = 1e-6
        p = s * rng.uniform(0.02, 0.5, n)
        q = s - p
        msly = mms * rng.uniform(0.05, 0.9, n)
    else:
        p, q = rng.uniform(5e-4, 0.01, n), rng.uniform(0.2, 0.5, n)
        d = 10.0 ** rng.uniform(-12, -9, n)
        d[0] = 1e-12
        msly = mms * (1.0 - d)
    a = dict(mms=mms, msly=msly, p=p, q=q, **_diff_common(n, rng))
    return {k: a[k] for k in DIFF_ARGS}


@functools.lru_cache(maxsize=None)
def oracle_error(kind, first):
    """DIFF_OUT -> max relative error of the float64 oracle against the
    50-digit restatement on diffusion_ill(kind)."""
    from oracle import diffusion as od
    a = diffusion_ill(kind)
    got = od.diffusion(*[a[k] for k in DIFF_ARGS], first)
    ref = diffusion_mp(a, first)
    return {k: max_rel_err(got[k], ref[k]) for k in DIFF_OUT}


def ill_tolerance(kind, first):
    """DIFF_OUT -> max(1e-12, 8 x the oracle's own error): the device's log and
    pow are allowed a few ulp where glibc's are under one."""
    return {k: max(1e-12, 8.0 * e) for k, e in oracle_error(kind, first).items()}


# ------------------------------------------------------ first-year seeding case
INIT_COLS = ("adopters_cum_last_year", "system_kw_cum_last_year", "batt_kw_cum_last_year",
             "batt_kwh_cum_last_year", "market_share_last_year", "market_value_last_year")
INIT_COPIES = {"initial_number_of_adopters": "adopters_cum_last_year", "initial_pv_kw": "system_kw_cum_last_year",
               "initial_batt_kw": "batt_kw_cum_last_year", "initial_batt_kwh": "batt_kwh_cum_last_year",
               "initial_market_share": "market_share_last_year"}
CAP_COLS = ("system_mw", "batt_mw", "batt_mwh", "pv_systems_count", "batt_systems_count")
# (state, sector, tech) -> (members, what the group is there for)
INIT_GROUPS = {("AA", "res", "solar"): (1, "single"),
               ("AA", "com", "solar"): (255, "some_nan"),
               ("BB", "res", "solar"): (256, "all_zero"),
               ("BB", "com", "solar"): (257, "one_zero"),
               ("CC", "res", "solar"): (700, "kahan"),
               ("CC", "ind", "solar"): (3, "all_nan"),
               ("DD", "res", "solar"): (5, "no_caps"),
               ("AA", "res", "wind"): (2, "second_tech")}


@functools.lru_cache(maxsize=None)
def initial_shares_case():
    """Groups of 1 / 255 / 256 / 257 / 700 members (and three small ones)
    interleaved in frame order.  Returns dict(state, sector, tech: lists;
    weight, capex: float64 [n] in frame order; caps: dict of lists; dev_index:
    a permutation, device row dev_index[i] holds frame row i; kind: per row)."""
    rng = np.random.default_rng(57)
    keys, kinds = [], []
    for key, (m, kind) in INIT_GROUPS.items():
        keys += [key] * m
        kinds += [kind] * m
    order = rng.permutation(len(keys))
    keys = [keys[i] for i in order]
    kinds = np.array([kinds[i] for i in order])
    n = len(keys)
    w = rng.uniform(0.5, 4000.0, n)
    w[kinds == "all_zero"] = 0.0
    w[kinds == "all_nan"] = np.nan
    rows = np.flatnonzero(kinds == "some_nan")
    w[rows[[0, 7, 100, 254]]] = np.nan                      # first and last member among them
    w[np.flatnonzero(kinds == "one_zero")[256]] = 0.0       # reached on the member loop's second trip
    rows = np.flatnonzero(kinds == "kahan")
    w[rows] = kahan_weights(rows.size)                      # frame order: 1e8 first
    caps = {"state_abbr": [], "sector_abbr": [], **{c: [] for c in CAP_COLS}}
    for s, c in dict.fromkeys((s, c) for (s, c, _), (_, kind) in INIT_GROUPS.items() if kind != "no_caps"):
        caps["state_abbr"].append(s)
        caps["sector_abbr"].append(c)
        for col in CAP_COLS:
            caps[col].append(float(rng.uniform(1.0, 900.0)))
    caps["batt_mwh"][1] = float("nan")                      # a NaN capacity: fillna(0)
    return dict(state=[k[0] for k in keys], sector=[k[1] for k in keys], tech=[k[2] for k in keys],
                weight=w, capex=rng.uniform(900.0, 3500.0, n), caps=caps,
                dev_index=rng.permutation(n).astype(np.int64), kind=kinds)


def initial_shares_pandas(case):
    """estimate_initial_market_shares as pandas operations: group sum and count,
    the two left merges, the portions, fillna(0).  Returns (frame-order columns
    dict, per-group sum Series, per-group count Series)."""
    import pandas as pd
    df = pd.DataFrame({"state_abbr": case["state"], "sector_abbr": case["sector"], "tech": case["tech"],
                       "developable_agent_weight": case["weight"], "system_capex_per_kw": case["capex"]})
    by = ["state_abbr", "sector_abbr", "tech"]
    g = df[by + ["developable_agent_weight"]].groupby(by)
    tot = g.sum().reset_index().rename(columns={"developable_agent_weight": "developable_customers_in_state"})
    cnt = g.count().reset_index().rename(columns={"developable_agent_weight": "agent_count"})
    df = pd.merge(df, pd.merge(tot, cnt, how="left", on=by), how="left", on=by)
    df = pd.merge(df, pd.DataFrame(case["caps"]), how="left", on=["state_abbr", "sector_abbr"])
    with np.errstate(all="ignore"):
        portion = np.where(df["developable_customers_in_state"] > 0,
                           df["developable_agent_weight"] / df["developable_customers_in_state"],
                           1. / df["agent_count"])
        df["adopters_cum_last_year"] = portion * df["pv_systems_count"]
        df["system_kw_cum_last_year"] = portion * df["system_mw"] * 1000.
        df["batt_kw_cum_last_year"] = portion * df["batt_mw"] * 1000.0
        df["batt_kwh_cum_last_year"] = portion * df["batt_mwh"] * 1000.0
        df["market_share_last_year"] = np.where(df["developable_agent_weight"] == 0, 0,
                                                df["adopters_cum_last_year"] / df["developable_agent_weight"])
        df["market_value_last_year"] = df["system_capex_per_kw"] * df["system_kw_cum_last_year"]
    cols = {k: df[k].fillna(0).to_numpy(dtype=np.float64) for k in INIT_COLS}
    return cols, tot.set_index(by)["developable_customers_in_state"], cnt.set_index(by)["agent_count"]
