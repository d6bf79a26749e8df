"""Constructed edge days for the battery dispatch, an exact reference of the
daily peak-shaving target and a classifier of the oracle's day_target branches.

The synthetic profiles (dgen_amd.synth) have lognormal noise on every load hour
and a cloud factor clipped at 0.05: no ties, no zero hours, no dark days, and a
saturated day (an hour's deficit above the power limit) on under 1 % of their
lane-days.  The rows built here hold the degenerate days on purpose, each in
the positions where the state carried into it differs (bank full, bank empty,
month boundary, year wrap).

Three independent pieces, all CPU only:

  edge_rows()          the day library laid out into 365-day load / cf rows
  day_target_exact()   f(T) = sum_h min(max(d_h - T, 0), P) <= E solved by
  dispatch_exact()     walking the breakpoints of f in integer arithmetic (every
                       float64 is a dyadic rational): no bisection, no
                       iteration cap, one rounding at the end
  classify_days()      the oracle's day_target (oracle/orc.c) followed branch by
                       branch in its own float64 operation order, returning the
                       branch each plan took and the edge flags of each lane-day

dispatch_exact and classify_days share the oracle's per-hour arithmetic
(orc_batt_dispatch, operation for operation) and differ only in the planner;
tests/test_dispatch_refs.py checks that the classifier's dispatch is the
oracle's bit for bit, so its labels describe the path the oracle really took.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

NH = 8760
DAYS_IN_MONTH = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
MONTH_START_DAY = np.concatenate([[0], np.cumsum(DAYS_IN_MONTH)])

LABELS = ("fits", "unsaturated", "bisect-converged", "bisect-capped", "k<=0", "clamped")
FITS, UNSAT, CONVERGED, CAPPED, KLE0, CLAMPED = range(6)
SATURATED = (CONVERGED, CAPPED, KLE0, CLAMPED)
FLAGS = ("tied_maxima", "all_zero", "nn_zero", "bank_full", "bank_empty")

# the reference's config defaults (oracle.DEFAULT_CFG, dgen_amd.config): used
# only to place the patterns' values around the nominal agent's power limit
_V_NOM, _Q_FULL, _MIN_SOC, _MAX_SOC, _ETA_OUT = 3.6, 3.2, 0.10, 0.95, 0.9408

NOMINAL_KW = 5.0          # the PV size of a row's own agent (load_kwh = the row's sum, so ls = 1)


def batt_size(desired_kw, desired_kwh, volts, v_nom=_V_NOM, q_full=_Q_FULL):
    """orc_batt_size: cells in series to the voltage, whole strings to the capacity."""
    if not desired_kwh > 0.0:
        return 0.0, 0.0
    series = math.ceil(volts / v_nom)
    strings = math.floor(desired_kwh * 1000.0 / (q_full * v_nom * series) + 0.5)
    strings = max(strings, 1.0)
    bank = q_full * v_nom * series * strings * 0.001
    return bank, bank * (desired_kw / desired_kwh)


def reference_bank(kw, volts=240.0):
    """The bank the sizing call gives a system of kw: kw / 0.8 kWh at 2 hours."""
    kwh = kw / 0.8
    return batt_size(kwh / 2.0, kwh, volts)


def string_kwh(volts=240.0):
    return _Q_FULL * _V_NOM * math.ceil(volts / _V_NOM) * 0.001


# ---------------------------------------------------------------------------
# 1. the day library
# ---------------------------------------------------------------------------
PATTERNS = ("ordinary", "dark", "flat_dark", "all_surplus", "all_zero", "zero_load_hours", "tie2", "tie3",
            "tie12", "pair_ties", "one_spike", "spike_block", "staircase", "tied_bp_lo", "tied_bp_hi",
            "bracket_below", "bracket_at", "bracket_above")
NP = len(PATTERNS)
ORD, DARK, SUR = PATTERNS.index("ordinary"), PATTERNS.index("dark"), PATTERNS.index("all_surplus")
HIGH = (PATTERNS.index("staircase"), PATTERNS.index("spike_block"))
# what the days between the position blocks cycle through: two in three saturated
FILLER = tuple(PATTERNS.index(k) for k in ("ordinary", "staircase", "spike_block", "all_surplus", "tied_bp_lo",
                                           "one_spike", "ordinary", "bracket_above", "staircase", "all_surplus",
                                           "tied_bp_hi", "spike_block"))
_HOUR_MIX = np.array([17, 3, 20, 8, 23, 11, 0, 14, 5, 19, 9, 22, 2, 16, 6, 12, 21, 1, 18, 7, 13, 4, 15, 10])


def _f32_next(x, steps):
    x = np.float32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float32(np.inf if steps > 0 else -np.inf))
    return x


def day_pattern(name, day=0):
    """(shape, cf): 24 float32 load values in kW at ls = 1 and 24 int32 cf values
    in [0, 1e6], for the nominal agent (NOMINAL_KW of PV, the reference bank:
    power limit P, deliverable energy of a full bank A).  `day` seeds the noise
    of the ordinary pattern and rotates the others' hours."""
    _, P = reference_bank(NOMINAL_KW)
    bank, _ = reference_bank(NOMINAL_KW)
    A = (_MAX_SOC - _MIN_SOC) * bank * _ETA_OUT
    h = np.arange(24)
    load = np.zeros(24)
    cf = np.zeros(24, np.int64)
    small = 0.05 + 0.04 * h                                  # 24 distinct values in [0.05, 0.97]
    if name in ("ordinary", "zero_load_hours"):
        rng = np.random.default_rng(7000 + day)
        load = (0.45 + 0.9 * np.exp(-((h - 19) / 2.5) ** 2) + 0.35 * np.exp(-((h - 7.5) / 1.5) ** 2))
        load = load * rng.lognormal(0.0, 0.15, 24)
        sun = np.clip(np.sin(np.pi * (h - 5.5) / 13.0), 0.0, None) * ((h >= 6) & (h <= 18))
        cf = np.round(1e6 * 0.75 * sun * rng.uniform(0.3, 1.0)).astype(np.int64)
        if name == "zero_load_hours":
            load[[2, 3, 4, 12, 22]] = 0.0                    # nn == 0 at night, nn < 0 at noon
    elif name == "dark":
        load = 0.5 + small[_HOUR_MIX]
    elif name == "flat_dark":
        load[:] = 1.25
    elif name == "all_surplus":
        load[:] = 0.3
        cf[:] = 900000
    elif name == "all_zero":
        pass
    elif name in ("tie2", "tie3", "tie12"):
        k = int(name[3:])
        load = small[_HOUR_MIX].copy()
        load[np.argsort(-load)[:k]] = 2.0                   # k equal largest deficits, below P
    elif name == "pair_ties":
        load = (0.2 + 0.2 * (h // 2))[_HOUR_MIX]
    elif name == "one_spike":
        load[19] = 40.0
    elif name == "spike_block":
        load[17:21] = 12.0
    elif name == "staircase":
        load = (0.19 * (h + 1.0))[_HOUR_MIX]                 # 0.19 .. 4.56, eight of them above P
    elif name in ("tied_bp_lo", "tied_bp_hi"):
        # full bank: f(W) = P (the hour at W + P + 1) + (u - W) = A up to u's
        # float32 rounding, so the answer sits on the three tied hours at W
        W = 1.0
        load = 0.02 + 0.03 * h                               # distinct, below W
        load[18:21] = W
        load[17] = W + P + 1.0
        load[21] = float(_f32_next(W + (A - P), -2 if name == "tied_bp_lo" else 2))
    elif name.startswith("bracket_"):
        load = 0.3 + small[_HOUR_MIX]
        step = {"below": -1, "at": 0, "above": 1}[name[8:]]
        p32 = np.float32(P)
        # `at` is the float32 nearest P, the others its neighbours on the two sides of P
        lo32 = p32 if float(p32) < P else _f32_next(p32, -1)
        hi32 = p32 if float(p32) > P else _f32_next(p32, 1)
        load[19] = float({-1: lo32, 0: p32, 1: hi32}[step])
    else:
        raise KeyError(name)
    if name not in ("ordinary", "zero_load_hours", "all_surplus", "all_zero"):
        load = np.roll(load, day % 5)
    return load.astype(np.float32), cf.astype(np.int32)


def row_plan(r):
    """The pattern index of each of row r's 365 days.  The position blocks
    [all_surplus, p], [dark, dark, p], [ordinary, p] of every pattern p, in an
    order rotated by r (so the rows differ on every calendar day); pattern
    (r + b) % NP on the last day of month b and pattern (r + b + 7) % NP on the
    first day of month b + 1; pattern r on December 31 and a high-deficit
    pattern other than r on January 1; FILLER elsewhere.  Row r's blocks start
    (2 r) % 7 days late, so that neighbouring rows (neighbouring lanes of the
    GPU test's waves) are at different places of the 7-day block cycle."""
    plan = np.full(365, -1, np.int64)
    plan[364] = r % NP
    plan[0] = HIGH[0] if r % NP != HIGH[0] else HIGH[1]
    for b in range(11):
        plan[MONTH_START_DAY[b + 1] - 1] = (r + b) % NP
        plan[MONTH_START_DAY[b + 1]] = (r + b + 7) % NP
    blocks = []
    for q in range(NP):
        p = (q + r) % NP
        blocks += [[SUR, p], [DARK, DARK, p], [ORD, p]]
    d, fill, lead = 1, r, (2 * r) % 7          # `lead` filler days first: neighbouring rows are out of step
    while d < 364:
        if plan[d] >= 0:
            d += 1
        elif d > lead and blocks and (plan[d:d + len(blocks[0])] < 0).all() and d + len(blocks[0]) <= 364:
            b = blocks.pop(0)
            plan[d:d + len(b)] = b
            d += len(b)
        else:
            plan[d] = FILLER[fill % len(FILLER)]
            fill += 1
            d += 1
    assert not blocks and (plan >= 0).all()
    return plan


def edge_rows(n_rows=NP):
    """(shapes float32 [R, 8760], cfs int32 [R, 8760], plan int [R, 365]): row r
    holds row_plan(r)'s days.  Valid inputs: finite, positive row sums."""
    shapes = np.zeros((n_rows, NH), np.float32)
    cfs = np.zeros((n_rows, NH), np.int32)
    plans = np.zeros((n_rows, 365), np.int64)
    for r in range(n_rows):
        plans[r] = row_plan(r)
        for d in range(365):
            s, c = day_pattern(PATTERNS[plans[r, d]], d)
            shapes[r, 24 * d:24 * d + 24] = s
            cfs[r, 24 * d:24 * d + 24] = c
    assert np.isfinite(shapes).all() and (shapes.sum(axis=1) > 0).all() and (shapes >= 0).all()
    assert cfs.min() >= 0 and cfs.max() <= 1000000
    return shapes, cfs, plans


# ---------------------------------------------------------------------------
# 2. the agents of the GPU test and of the CPU checks (one definition)
# ---------------------------------------------------------------------------
N_SYNTH_ROWS = 8
# (load scale, PV scale) of the agents that share a row; the first is the row's own agent
VARIANTS = ((1.0, 1.0), (2.0, 2.0), (0.7, 1.0), (1.0, 1.6), (1.5, 0.8))
SMALL = dict(n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


_TABLES = {}


def edge_tables():
    """(shapes, cfs, plans): the edge rows followed by N_SYNTH_ROWS rows of the
    res_1m_nem_tou synthetic population (the control)."""
    if not _TABLES:
        from dgen_amd.synth import make_population
        base = make_population("res_1m_nem_tou", 8, **SMALL)
        s, c, plans = edge_rows()
        _TABLES["t"] = (np.concatenate([s, base.shapes[:N_SYNTH_ROWS]]),
                        np.concatenate([c, base.cfs[:N_SYNTH_ROWS]]), plans)
        for a in _TABLES["t"]:
            a.setflags(write=False)
    return _TABLES["t"]


def edge_agents(n):
    """Caller-order columns of the n constructed agents: dict of load_row,
    cf_row, load_kwh, kw (the evaluated PV size), variant, and `order`, the
    explicit device order in which consecutive lanes sit on different rows
    (and so on different patterns on every calendar day).  Agent j of the
    device order sits on row j % R, variant j // R; a smaller n is a prefix of
    a larger one in device order."""
    shapes, cfs, _ = edge_tables()
    R = shapes.shape[0]
    j = np.arange(n)
    row, var = j % R, (j // R) % len(VARIANTS)
    ssum = np.array([np.sum(shapes[r].astype(np.float64)) for r in range(R)])
    naep = (cfs.astype(np.float64) / 1e6).sum(axis=1)
    ls_v = np.array([v[0] for v in VARIANTS])[var]
    kw_v = np.array([v[1] for v in VARIANTS])[var]
    edge = row < NP
    load_kwh = np.where(edge, ssum[row] * ls_v, 9000.0 * (1.0 + 0.1 * var))
    # synthetic rows: a PV size small enough that the evening peak exceeds the bank's power limit
    kw = np.where(edge, NOMINAL_KW * kw_v, 0.3 * load_kwh / naep[row])
    caller = np.lexsort((var, row))              # caller row k is device row caller[k]: by row, then variant
    order = np.empty(n, np.int64)                # upload_agents(order=...): device row j is caller row order[j]
    order[caller] = np.arange(n)
    return {"load_row": row[caller].astype(np.int32), "cf_row": row[caller].astype(np.int32),
            "load_kwh": load_kwh[caller], "kw": kw[caller], "variant": var[caller], "order": order}


def edge_population(config, n):
    """make_population(config, n) at the small table sizes with the profile
    tables replaced by edge_tables() and load_row / cf_row / load_kwh by
    edge_agents(n).  Returns (pop, kw, order): kw in caller order."""
    from dgen_amd.synth import make_population
    pop = make_population(config, n, **SMALL)
    shapes, cfs, _ = edge_tables()
    a = edge_agents(n)
    pop.shapes, pop.cfs = shapes.copy(), cfs.copy()
    for k in ("load_row", "cf_row", "load_kwh"):
        pop.cols[k] = a[k].astype(pop.cols[k].dtype)
    assert (pop.cols["flags"] & 1).all()         # residential: 240 V banks
    return pop, a["kw"].copy(), a["order"].copy()


def agent_hours(load_row, cf_row, load_kwh, kw, shapes=None, cfs=None):
    """load and pv [n, 8760] as the library forms them: shape x (load_kwh / row
    sum), cf x (((kw x 1000) x 0.96) / 1000 / 1e6)."""
    if shapes is None:
        shapes, cfs, _ = edge_tables()
    load_row, cf_row = np.atleast_1d(load_row), np.atleast_1d(cf_row)
    ssum = np.array([np.sum(shapes[r].astype(np.float64)) for r in load_row])
    ls = np.atleast_1d(load_kwh) / ssum
    cs6 = (((np.atleast_1d(kw) * 1000.0) * 0.96) / 1000.0) / 1e6
    return shapes[load_row].astype(np.float64) * ls[:, None], cfs[cf_row].astype(np.float64) * cs6[:, None]


# ---------------------------------------------------------------------------
# 3. the exact target
# ---------------------------------------------------------------------------
def day_target_exact(deficits, power, avail):
    """The smallest T >= 0 with f(T) = sum_h min(max(d_h - T, 0), P) <= E, as the
    float64 nearest the exact rational answer.  Every input is a dyadic
    rational, so scaled by a power of two they are integers; f is walked down
    from T = max d over its breakpoints (d_h, d_h - P) in integer arithmetic,
    a = #{d_h >= T} and b = #{d_h - P >= T} kept as the breakpoints are passed
    (slope -(a - b) below T).  No bisection, no iteration cap."""
    d = [float(x) for x in deficits]
    P, E = float(power), float(avail)
    assert P > 0.0 and E >= 0.0 and min(d) >= 0.0
    if max(d) == 0.0:
        return 0.0
    k = 53 - min(math.frexp(x)[1] for x in d + [P, E] if x != 0.0)
    D = sorted((int(math.ldexp(x, k)) for x in d), reverse=True)
    Pi, Ei = int(math.ldexp(P, k)), int(math.ldexp(E, k))
    ev = sorted([(x, 0) for x in D if x > 0] + [(x - Pi, 1) for x in D if x - Pi > 0], reverse=True)
    T, f, a, b, i = D[0], 0, 0, 0, 0
    while T > 0:
        while i < len(ev) and ev[i][0] == T:
            if ev[i][1] == 0:
                a += 1
            else:
                b += 1
            i += 1
        Tn = ev[i][0] if i < len(ev) else 0
        fn = f + (a - b) * (T - Tn)
        if fn > Ei:                                          # the answer lies in (Tn, T]
            t = Fraction(T * (a - b) - (Ei - f), a - b)
            return float(t / (1 << k) if k >= 0 else t * (1 << -k))
        f, T = fn, Tn
    return 0.0


def _plan_exact(win, power, avail):
    t = np.array([day_target_exact(win[i], power[i], avail[i]) for i in range(win.shape[0])])
    return t, None, None


def _seq(x):
    """Row sums in index order (np.cumsum adds sequentially, as the C loops do)."""
    return np.cumsum(x, axis=1)[:, -1]


def _plan_oracle(win, power, avail):
    """oracle/orc.c day_target on m windows at once, the same float64
    operations in the same order.  Returns (target, label, iterations)."""
    m = win.shape[0]
    s = -np.sort(-win, axis=1)
    P = power[:, None]
    T = np.zeros(m)
    label = np.full(m, FITS, np.int8)
    iters = np.zeros(m, np.int64)
    fits = _seq(np.minimum(s, P)) <= avail
    un = ~fits & (s[:, 0] <= power)
    if un.any():
        S = np.cumsum(s[un], axis=1)
        kk = np.arange(1.0, 25.0)[None, :]
        ok = S - kk * s[un] <= avail[un, None]
        K = np.ones(int(un.sum()))
        SK = s[un, 0].copy()
        for k in range(24):
            K = np.where(ok[:, k], k + 1.0, K)
            SK = np.where(ok[:, k], S[:, k], SK)
        T[un] = (SK - avail[un]) / K
        label[un] = UNSAT
    sat = ~fits & ~un
    if sat.any():
        ss, pw, av = s[sat], power[sat], avail[sat]
        n = ss.shape[0]
        a_lo = (ss > 0.0).sum(axis=1)
        b_lo = ((ss - pw[:, None]) >= 0.0).sum(axis=1)
        lo, hi, f_hi = np.zeros(n), ss[:, 0].copy(), np.zeros(n)
        a_hi, b_hi = np.zeros(n, np.int64), np.zeros(n, np.int64)
        it = np.zeros(n, np.int64)
        for _ in range(48):
            act = ~((a_lo == a_hi) & (b_lo == b_hi))
            if not act.any():
                break
            it += act
            mid = 0.5 * (lo + hi)
            e = ss - mid[:, None]
            am = (e > 0.0).sum(axis=1)
            bm = ((e - pw[:, None]) >= 0.0).sum(axis=1)
            f = _seq(np.minimum(np.maximum(e, 0.0), pw[:, None]))
            up = act & (f <= av)
            dn = act & ~(f <= av)
            hi, f_hi = np.where(up, mid, hi), np.where(up, f, f_hi)
            a_hi, b_hi = np.where(up, am, a_hi), np.where(up, bm, b_hi)
            lo = np.where(dn, mid, lo)
            a_lo, b_lo = np.where(dn, am, a_lo), np.where(dn, bm, b_lo)
        k = a_hi - b_hi
        with np.errstate(divide="ignore", invalid="ignore"):
            t = hi - (av - f_hi) / k
        below, above = (k > 0) & (t < lo), (k > 0) & (t > hi)
        t = np.where(below, lo, np.where(above, hi, t))
        lab = np.where(k <= 0, KLE0, np.where(below | above, CLAMPED, np.where(it == 48, CAPPED, CONVERGED)))
        T[sat] = np.where(k <= 0, hi, t)
        label[sat] = lab
        iters[sat] = it
    return T, label, iters


# ---------------------------------------------------------------------------
# 4. the dispatch (orc_batt_dispatch's per-hour arithmetic, n agents at once)
# ---------------------------------------------------------------------------
def _dispatch(load, pv, bank, power, cfg, planner, record):
    load, pv = np.atleast_2d(np.asarray(load, np.float64)), np.atleast_2d(np.asarray(pv, np.float64))
    n = load.shape[0]
    bank = np.broadcast_to(np.asarray(bank, np.float64), (n,)).copy()
    power = np.broadcast_to(np.asarray(power, np.float64), (n,)).copy()
    has = bank > 0.0
    hourly = cfg.batt_update_hours == 1
    loss, mfl = cfg.batt_loss_model == 1, cfg.batt_month_floor == 1
    eta = cfg.batt_conv_eff
    sb = np.where(has, bank, 1.0)                            # no division by a zero bank
    inv_eta_in = 1.0 / cfg.batt_eta_in
    in_per_bank = np.where(has, cfg.batt_eta_in / sb, 0.0)
    out_per_bank = np.where(has, 1.0 / (cfg.batt_eta_out * sb), 0.0)
    soc = np.full(n, cfg.batt_init_soc)
    target, floor_t = np.zeros(n), np.zeros(n)
    sys_out, g2l = np.zeros((n, NH)), np.zeros((n, NH))
    deficit = np.maximum(load - pv, 0.0)
    wrap = np.concatenate([deficit, deficit[:, :24]], axis=1)
    rec = None
    if record:
        slots = NH if hourly else 365
        rec = {"label": np.full((n, slots), -1, np.int8), "iters": np.zeros((n, slots), np.int64),
               "avail": np.full((n, slots), np.nan),
               "tied_maxima": np.zeros((n, slots), bool), "all_zero": np.zeros((n, slots), bool),
               "nn_zero": np.zeros((n, 365), bool), "bank_full": np.zeros((n, 365), bool),
               "bank_empty": np.zeros((n, 365), bool)}
    month_starts = set(int(x) * 24 for x in MONTH_START_DAY[1:12])

    def plan(h, who, av):
        idx = np.flatnonzero(who)
        if idx.size == 0:
            return
        win = wrap[idx, h:h + 24]
        t, lab, it = planner(win, power[idx], av[idx])
        if lab is None:
            lab, it = 0, 0
        if mfl:
            low = t < floor_t[idx]
            t = np.where(low, floor_t[idx], t)
            floor_t[idx] = t
        target[idx] = t
        if rec is not None:
            slot = h if hourly else h // 24
            top = np.sort(win, axis=1)
            rec["label"][idx, slot], rec["iters"][idx, slot] = lab, it
            rec["avail"][idx, slot] = av[idx]
            rec["tied_maxima"][idx, slot] = (top[:, -1] == top[:, -2]) & (top[:, -1] > 0.0)
            rec["all_zero"][idx, slot] = top[:, -1] == 0.0

    for h in range(NH):
        nn = load[:, h] - pv[:, h]
        if h in month_starts:
            floor_t[:] = 0.0
        chg = nn < 0.0
        if loss:
            e_av = np.maximum((soc - cfg.batt_min_soc) * bank, 0.0)
            if hourly:
                need = has & (nn > 0.0) & ((e_av > 0.0) | mfl)
                target[:] = 0.0
                plan(h, need, e_av * eta)
            elif h % 24 == 0:
                plan(h, has, e_av * eta)
            v = cfg.batt_v_cell_empty + (cfg.batt_v_cell_full - cfg.batt_v_cell_empty) * soc
            k = cfg.batt_r_cell * cfg.batt_q_full * cfg.batt_v_nom / (sb * (v * v))
            e_room = np.maximum((cfg.batt_max_soc - soc) * bank, 0.0)
            disc = 1.0 - 4.0 * k * e_room
            x_max = np.where(disc > 0.0, 2.0 * e_room / (1.0 + np.sqrt(np.maximum(disc, 0.0))), 0.5 / k)
            c = np.minimum(np.minimum(-nn, power), x_max / eta)
            x = c * eta
            soc_c = soc + (x - k * (x * x)) / sb
            y_max = 2.0 * e_av / (1.0 + np.sqrt(1.0 + 4.0 * k * e_av))
            d = np.minimum(np.minimum(np.maximum(nn - target, 0.0), power), y_max * eta)
            y = d / eta
            soc_d = soc - (y + k * (y * y)) / sb
        else:
            if not hourly and h % 24 == 0:
                plan(h, has, np.maximum((soc - cfg.batt_min_soc) * bank * cfg.batt_eta_out, 0.0))
            room = np.maximum((cfg.batt_max_soc - soc) * bank * inv_eta_in, 0.0)
            c = np.minimum(np.minimum(-nn, power), room)
            avail = np.maximum((soc - cfg.batt_min_soc) * bank * cfg.batt_eta_out, 0.0)
            if hourly:
                target[:] = 0.0
                plan(h, has & (nn > 0.0) & ((avail > 0.0) | mfl), avail)
            d = np.minimum(np.minimum(np.maximum(nn - target, 0.0), power), avail)
            soc_c = soc + c * in_per_bank
            soc_d = soc - d * out_per_bank
        soc = np.where(has, np.where(chg, soc_c, soc_d), soc)
        sys_out[:, h] = np.where(has, np.where(chg, pv[:, h] - c, pv[:, h] + d), pv[:, h])
        g2l[:, h] = np.where(has, np.where(chg, 0.0, nn - d), np.maximum(nn, 0.0))
        if rec is not None:
            day = h // 24
            rec["nn_zero"][:, day] |= has & (nn == 0.0)
            rec["bank_full"][:, day] |= has & (soc >= cfg.batt_max_soc - 1e-9)
            rec["bank_empty"][:, day] |= has & (soc <= cfg.batt_min_soc + 1e-9)
    return sys_out, g2l, rec


def dispatch_exact(load, pv, bank, power, cfg, planned=False):
    """(system output, grid-to-load) [n, 8760] of orc_batt_dispatch's rule with
    every plan's target from day_target_exact: daily plan and hourly re-plan
    (cfg.batt_update_hours), month floor, loss model.  load, pv: [8760] or
    [n, 8760]; bank, power: scalars or [n]; cfg: any object with orc.Cfg's
    attributes.  planned: also return the mask of the slots (days, or hours of
    the re-plan) in which a plan was made."""
    s, g, rec = _dispatch(load, pv, bank, power, cfg, _plan_exact, planned)
    return (s, g, rec["label"] >= 0) if planned else (s, g)


def classify_days(load, pv, bank, power, cfg):
    """The oracle's dispatch followed plan by plan.  Returns a dict:
    label [n, 365] (daily plan) or [n, 8760] (hourly re-plan; -1 where no plan
    is made) with indices into LABELS, iters (bisection iterations), avail (the
    energy each plan was made from), the plan
    flags tied_maxima and all_zero in the same shape, the lane-day flags
    nn_zero, bank_full, bank_empty [n, 365], and sys / g2l, the dispatch those
    plans give (the oracle's, bit for bit).  Everything comes from the
    reference's arithmetic; no device output enters."""
    s, g, rec = _dispatch(load, pv, bank, power, cfg, _plan_oracle, True)
    rec["sys"], rec["g2l"] = s, g
    return rec


# ---------------------------------------------------------------------------
# 5. the banks of the replay test
# ---------------------------------------------------------------------------
REPLAY_SHIFTS = (0, 1, 2, 3)
REPLAY_LEFT_OUT_CAP = 0.10


def replay_banks(a, shift):
    """Desired (bank_kwh, bank_kw) per agent of edge_agents' columns `a`, in
    caller order: device row j gets bank kind (j + shift) % 4 of {none, 0.4 of
    a string (sized to one string), the reference's kw / 0.8, three times
    that} at 1 hour or 4 hours ((j // 4 + shift) % 2), so one wave holds every
    combination."""
    j = np.argsort(a["order"])                   # caller row k is device row j[k]
    ref = a["kw"] / 0.8
    kinds = np.stack([np.zeros_like(ref), np.full_like(ref, 0.4 * string_kwh()), ref, 3.0 * ref])
    kwh = kinds[(j + shift) % 4, np.arange(ref.size)]
    hours = np.where((j // 4 + shift) % 2 == 0, 1.0, 4.0)
    return kwh, kwh / hours
