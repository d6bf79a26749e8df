"""The constructed dispatch edge days (tests/dispatch_refs.py) on the CPU: the
rows hold every pattern in every position, the oracle's dispatch agrees with
an exact solution of every plan's target, the classifier follows the oracle bit
for bit and finds every branch and flag on the agents the GPU test
(tests/test_gpu_dispatch_edges.py) runs, December 31 sees January 1 under the
hourly re-plan, and the replay test's ambiguity rule leaves out few enough
agents from the reference alone."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import dispatch_refs as dr

FORMS = {"daily": {}, "hourly": {"batt_update_hours": 1},
         "daily-floor": {"batt_month_floor": 1}, "hourly-floor": {"batt_month_floor": 1, "batt_update_hours": 1},
         "daily-loss": {"batt_loss_model": 1, "batt_r_cell": 0.02},
         "hourly-loss": {"batt_loss_model": 1, "batt_r_cell": 0.02, "batt_update_hours": 1}}
N_OF = lambda form: 65 if form.startswith("hourly") else 130


def _agents(n):
    a = dr.edge_agents(n)
    load, pv = dr.agent_hours(a["load_row"], a["cf_row"], a["load_kwh"], a["kw"])
    bp = np.array([dr.reference_bank(k) for k in a["kw"]])
    return a, load, pv, bp[:, 0], bp[:, 1]


_CACHE = {}


def _classified(form):
    if form not in _CACHE:
        a, load, pv, bank, power = _agents(N_OF(form))
        _CACHE[form] = (a, load, pv, bank, power, dr.classify_days(load, pv, bank, power, orc.make_cfg(**FORMS[form])))
    return _CACHE[form]


def test_rows_hold_every_pattern_in_every_position():
    shapes, cfs, plans = dr.edge_rows()
    assert shapes.dtype == np.float32 and cfs.dtype == np.int32 and shapes.shape == cfs.shape == (dr.NP, 8760)
    assert np.isfinite(shapes).all() and (shapes.astype(np.float64).sum(axis=1) > 0).all()
    last = dr.MONTH_START_DAY[1:12] - 1
    for p, name in enumerate(dr.PATTERNS):
        at = plans == p
        prev1 = np.roll(plans, 1, axis=1)[:, 1:]
        prev2 = np.roll(plans, 2, axis=1)[:, 2:]
        assert (at[:, 1:] & (prev1 == dr.SUR)).any(), name
        assert (at[:, 2:] & (prev1[:, 1:] == dr.DARK) & (prev2 == dr.DARK)).any(), name
        assert (at[:, 1:] & (prev1 == dr.ORD)).any(), name
        assert at[:, last].any() and at[:, last + 1].any(), name
        r = np.flatnonzero(at[:, 364])
        assert r.size and all(plans[i, 0] in dr.HIGH and plans[i, 0] != p for i in r), name
    # neighbouring rows (neighbouring lanes) hold different patterns on a calendar day
    differ = (plans != np.roll(plans, 1, axis=0)).mean()
    print(f"neighbouring rows differ on {differ:.3f} of the days")
    assert differ >= 0.9
    # same pair, same deficit bits: ties need no exact arithmetic
    s, c = dr.day_pattern("tie12")
    assert np.unique(np.sort(s)[-12:]).size == 1 and not c.any()
    s, _ = dr.day_pattern("pair_ties")
    assert np.array_equal(np.sort(s)[0::2], np.sort(s)[1::2]) and np.unique(s).size == 12
    _, P = dr.reference_bank(dr.NOMINAL_KW)
    assert dr.reference_bank(dr.NOMINAL_KW) == orc.batt_size(dr.NOMINAL_KW / 1.6, dr.NOMINAL_KW / 0.8, 240.0, orc.make_cfg())
    top = [float(dr.day_pattern("bracket_" + k)[0].max()) for k in ("below", "at", "above")]
    assert top[0] < P < top[2] and top[0] <= top[1] <= top[2]
    assert np.nextafter(np.float32(top[0]), np.float32(np.inf)) == np.float32(top[2])
    s, _ = dr.day_pattern("staircase")
    assert np.unique(s).size == 24 and 6 <= (s > P).sum() <= 10


def test_exact_target_on_hand_cases():
    """f(T) by hand: three hours 4, 2, 1 at P = 1.5.  f(0) = 1.5 + 1.5 + 1 = 4;
    f(0.5) = 1.5 + 1.5 + 0.5 = 3.5; f(1) = 1.5 + 1 = 2.5; f = 1.5 on all of [2, 2.5]
    (the smallest T counts); f(4) = 0."""
    d = [4.0, 2.0, 1.0] + [0.0] * 21
    for E, T in ((4.0, 0.0), (5.0, 0.0), (3.5, 0.5), (3.0, 0.75), (2.5, 1.0), (2.0, 1.5), (1.5, 2.0), (0.75, 3.25),
                 (0.0, 4.0)):
        assert dr.day_target_exact(d, 1.5, E) == T, (E, T)
    assert dr.day_target_exact([0.0] * 24, 1.0, 0.0) == 0.0
    # ties: 12 hours at 1 (P = 2), E = 6 -> T = 0.5; and a value no float64 sum would give exactly
    assert dr.day_target_exact([1.0] * 12 + [0.0] * 12, 2.0, 6.0) == 0.5
    assert dr.day_target_exact([1.0, 1.0, 1.0] + [0.0] * 21, 2.0, 1.0) == 2.0 / 3.0


@pytest.mark.parametrize("form", list(FORMS))
def test_oracle_matches_the_exact_reference(form):
    """orc.batt_dispatch against dispatch_exact on every constructed agent of
    tests/test_gpu_dispatch_edges.py, grid-to-load and system output within
    test_hourly_f64_planes' bound, 1e-12 x max(1, |plane| max).  Measured: the
    worst ratio is 2.6e-14 (daily plan with the month floor), 2.3e-15 on the
    daily plan; the 48-iteration cap leaves a bracket of 2^-48 of the day's
    largest deficit, 3.6e-15 relative, and is inside the bound.

    hourly-floor found a discontinuity in the rule, since removed.  The re-plan
    made a plan only where avail > 0, and under the month floor a plan raises
    the floor.  A discharge clamped by the energy left puts the SOC on
    batt_min_soc up to rounding, so the next deficit hour saw avail = 0 or dust
    of 1e-16 kWh; with dust a plan was made, its target the window's largest
    deficit, and the month's floor jumped there; with 0 it did not (oracle
    against this reference: 0.2 of the plane's maximum, agent 5, hour 1728).
    Under the floor every deficit hour now plans, as the daily plan does at a
    day's first hour: the target at avail = 0 is the limit of the targets as
    avail goes to 0.  Measured since: 1.1e-14."""
    n = N_OF(form)
    a, load, pv, bank, power = _agents(n)
    cfg = orc.make_cfg(**FORMS[form])
    se, ge = dr.dispatch_exact(load, pv, bank, power, cfg)
    worst = 0.0
    for i in range(n):
        so, go = orc.batt_dispatch(load[i], pv[i], bank[i], power[i], cfg)
        for name, x, y in (("system output", so, se[i]), ("grid to load", go, ge[i])):
            worst = max(worst, _within_bound(x, y, a, i, (form, name)))
    print(f"{form}: oracle against the exact reference, worst ratio {worst:.3e} over {n} agents")


@pytest.mark.parametrize("shift", dr.REPLAY_SHIFTS)
def test_oracle_matches_the_exact_reference_at_the_replay_banks(shift):
    """The same comparison at the banks test_replay_at_caller_given_banks
    replays (none, one string, the reference's, three times it, at 1 and 4
    hours; daily plan, the only form replay_at has)."""
    a, load, pv, _, _ = _agents(130)
    kwh, pkw = dr.replay_banks(a, shift)
    cfg = orc.make_cfg()
    bp = np.array([(0.0, 0.0) if kwh[i] == 0.0 else orc.batt_size(pkw[i], kwh[i], 240.0, cfg) for i in range(130)])
    assert (bp[:, 0] == 0.0).sum() >= 30 and np.unique(bp[:, 0]).size > 8
    se, ge = dr.dispatch_exact(load, pv, bp[:, 0], bp[:, 1], cfg)
    worst = 0.0
    for i in range(130):
        so, go = orc.batt_dispatch(load[i], pv[i], bp[i, 0], bp[i, 1], cfg)
        for name, x, y in (("system output", so, se[i]), ("grid to load", go, ge[i])):
            worst = max(worst, _within_bound(x, y, a, i, (shift, name)))
    print(f"replay banks, shift {shift}: oracle against the exact reference, worst ratio {worst:.3e}")


def _within_bound(x, y, a, i, what):
    """x (oracle) against y (exact): both finite, |x - y| max <= 1e-12 x
    max(1, |y| max).  Returns the ratio; a NaN anywhere fails."""
    assert np.isfinite(x).all() and np.isfinite(y).all(), (what, i, "not finite")
    ratio = float(np.abs(x - y).max()) / max(1.0, float(np.abs(y).max()))
    h = int(np.abs(x - y).argmax())
    row = int(a["load_row"][i])
    pat = dr.PATTERNS[dr.edge_tables()[2][row, h // 24]] if row < dr.NP else "synthetic"
    assert ratio <= 1e-12, (what, i, ratio, "hour", h, "pattern", pat)
    return ratio


@pytest.mark.parametrize("form", [f for f in FORMS if f not in ("daily", "hourly")])
def test_classifier_dispatch_is_the_oracles_in_the_option_forms(form):
    """Month floor and loss model, both plans: the classifier's dispatch is
    orc.batt_dispatch's bit for bit (NaN would not equal itself here)."""
    a, load, pv, bank, power, rec = _classified(form)
    cfg = orc.make_cfg(**FORMS[form])
    for i in range(load.shape[0]):
        so, go = orc.batt_dispatch(load[i], pv[i], bank[i], power[i], cfg)
        assert np.isfinite(so).all() and np.isfinite(go).all(), (form, i)
        assert np.array_equal(so, rec["sys"][i]) and np.array_equal(go, rec["g2l"][i]), (form, i)
    assert (rec["label"] == dr.KLE0).sum() >= 8 and (rec["label"] == dr.CLAMPED).sum() == 0


def test_capped_and_clamped_exits_at_the_target_level():
    """The two exits the dispatch chain does not reach 8 times, reached by
    hand.  One hour at s0 (saturated), one at u = 3, three tied at W = 2,
    P = 1.5: f(W) = P + (u - W) = 2.5 exactly, slope -1 right of W and -4 left
    of it.  With avail = 2.5 + g, g a few 2^-47, the answer W - g / 4 sits just
    left of the tied breakpoint, W stays inside the bracket until the cap, and
    the linear step taken from hi with the slope right of W (k = 1) lands at
    W - g, past lo: `t < lo` clamps.  Over 4 values of s0 and 128 of g both
    exits occur at least 8 times; every target is within 24 x 2^-48 x s0 of the
    exact one (the bracket the cap leaves, times the largest slope), and the
    oracle itself (bank 4 kWh, min SOC 0, eta_out 1, so avail = 4 x init SOC
    exactly) returns the classifier's target bit for bit as the grid import of
    the hour at u."""
    P, W, u = 1.5, 2.0, 3.0
    rows, av = [], []
    for s0 in (9.7, 11.3, 13.9, 17.1):
        for j in range(1, 129):
            d = np.zeros(24)
            d[5], d[7], d[9:12] = s0, u, W
            rows.append(d)
            av.append(2.5 + j * 2.0 ** -47)
    win, av = np.array(rows), np.array(av)
    T, lab, it = dr._plan_oracle(win, np.full(av.size, P), av)
    count = {dr.LABELS[k]: int((lab == k).sum()) for k in range(6)}
    print(f"hand-built targets: {count}")
    assert count["bisect-capped"] >= 8 and count["clamped"] >= 8
    assert (it[np.isin(lab, (dr.CAPPED, dr.CLAMPED))] == 48).all()
    exact = np.array([dr.day_target_exact(win[i], P, av[i]) for i in range(av.size)])
    assert (np.abs(T - exact) <= 24.0 * 2.0 ** -48 * win.max(axis=1)).all()
    for i in np.flatnonzero(np.isin(lab, (dr.CAPPED, dr.CLAMPED)))[::4]:
        load = np.zeros(8760)
        load[:24] = win[i]
        cfg = orc.make_cfg(batt_min_soc=0.0, batt_eta_out=1.0, batt_init_soc=av[i] / 4.0)
        _, g2l = orc.batt_dispatch(load, np.zeros(8760), 4.0, P, cfg)
        assert g2l[7] == T[i], (i, g2l[7], T[i])


@pytest.mark.parametrize("form", ["daily", "hourly"])
def test_classifier_follows_the_oracle_and_covers_every_branch(form):
    """The classifier's dispatch is orc.batt_dispatch's bit for bit, so its
    labels are the branches the oracle took.  Every label and flag occurs on at
    least 8 lane-days (plans, for the re-plan), with two exceptions that follow
    from the algorithm:

    clamped never occurs.  `t > hi` cannot: f_hi <= avail was tested in the
    same arithmetic, so (avail - f_hi) / k >= 0 and t <= hi.  `t < lo` needs a
    breakpoint left inside the final bracket with a slope change that carries
    the linear step past lo, i.e. the loop ended by the cap with k > 0 (below).

    bisect-capped with k > 0 needs the answer within 2^-48 of the largest
    deficit of a breakpoint without being at the window's maximum: avail has to
    equal f at a breakpoint to 15 digits.  An empty bank does that (avail = 0
    or rounding dust): the answer is the maximum, hi never moves, the loop runs
    its 48 iterations and leaves through k <= 0, so the cap is reached on every
    k<=0 plan.  With k > 0 it takes a flat piece of f, e.g. avail equal to the
    power limit with one hour saturated and the next breakpoint the answer;
    the SOC chain produces that on a few plans of the re-plan and on no day of
    the daily plan.  The count is printed, not pinned: what is asserted is that
    every such plan's exact answer lies within the last bracket of a
    breakpoint.  test_capped_and_clamped_exits_at_the_target_level reaches both
    exits at least 8 times by hand.

    The library reaches the saturated branch on at least 20 % of its lane-days
    (synthetic populations: 0.1 - 0.7 %)."""
    a, load, pv, bank, power, rec = _classified(form)
    cfg = orc.make_cfg(**FORMS[form])
    n = load.shape[0]
    for i in range(n):
        so, go = orc.batt_dispatch(load[i], pv[i], bank[i], power[i], cfg)
        assert np.array_equal(so, rec["sys"][i]) and np.array_equal(go, rec["g2l"][i]), i
    lab = rec["label"]
    count = {dr.LABELS[k]: int((lab == k).sum()) for k in range(6)}
    flags = {k: int(rec[k].sum()) for k in dr.FLAGS}
    edge = a["load_row"] < dr.NP
    share = np.isin(lab[edge], dr.SATURATED).sum() / (lab[edge] >= 0).sum()
    print(f"{form}: {count}, {flags}, cap reached {int((rec['iters'] == 48).sum())}, saturated share {share:.3f}")
    for k in ("fits", "unsaturated", "bisect-converged", "k<=0"):
        assert count[k] >= 8, (k, count)
    assert count["clamped"] == 0
    capped = rec["iters"] == 48
    assert capped.sum() >= 8 and capped[lab == dr.KLE0].all() and np.isin(lab[capped], (dr.KLE0, dr.CAPPED)).all()
    # the cap with k > 0: the exact answer is within the last bracket (2^-48 of the window's largest deficit)
    # of a breakpoint d_h or d_h - P; how often that happens is not pinned
    deficit = np.maximum(load - pv, 0.0)
    wrap = np.concatenate([deficit, deficit[:, :24]], axis=1)
    for i, slot in zip(*np.nonzero(lab == dr.CAPPED)):
        h = slot if form == "hourly" else 24 * slot
        win = wrap[i, h:h + 24]
        t = dr.day_target_exact(win, power[i], rec["avail"][i, slot])
        bps = np.concatenate([win, win - power[i]])
        assert np.abs(bps - t).min() <= 2.0 ** -47 * win.max(), (i, slot)
    if form == "daily":
        for k in dr.FLAGS:
            assert flags[k] >= 8, (k, flags)
    else:            # a plan is made only in an hour with a deficit: no all-zero window
        assert flags["all_zero"] == 0 and all(flags[k] >= 8 for k in dr.FLAGS if k != "all_zero")
    assert share >= 0.20
    # the reference bank's power limit lies inside every agent's range of deficits
    top = np.maximum(load - pv, 0.0).max(axis=1)
    assert (power < top).all() and (np.maximum(load - pv, 0.0).min(axis=1) == 0.0).all()
    # every pattern meets the bank full and the bank empty at its first hour (daily plan)
    if form == "daily":
        plans = dr.edge_tables()[2]
        own = np.flatnonzero(edge & (a["variant"] == 0))
        full_before = np.zeros(dr.NP, bool)
        empty_before = np.zeros(dr.NP, bool)
        for i in own:
            p = plans[a["load_row"][i]]
            full_before[p[1:][rec["bank_full"][i, :-1] & (p[:-1] == dr.SUR)]] = True
            empty_before[p[1:][rec["bank_empty"][i, :-1] & (p[:-1] == dr.DARK)]] = True
        assert full_before.all() and empty_before.all()
        # the saturated patterns bisect; the tied breakpoint costs the bisection far more steps
        it = {name: [] for name in dr.PATTERNS}
        for i in own:
            p = plans[a["load_row"][i]]
            ok = lab[i] == dr.CONVERGED
            for d in np.flatnonzero(ok):
                it[dr.PATTERNS[p[d]]].append(int(rec["iters"][i, d]))
        for name in ("spike_block", "staircase", "tied_bp_lo", "tied_bp_hi", "bracket_above"):
            assert len(it[name]) >= 8, name
        assert max(it["tied_bp_lo"] + it["tied_bp_hi"]) >= 20 > max(it["spike_block"])


def test_december_31_sees_january_1():
    """Under batt_update_hours = 1 the window of December 31's hours reaches
    into January 1: with the ordinary day there instead of the high-deficit
    pattern, the reference's December 31 dispatch changes."""
    a, load, pv, bank, power = _agents(dr.NP)                # the rows' own agents
    shapes, cfs, _ = dr.edge_tables()
    s2, c2 = shapes.copy(), cfs.copy()
    s_ord, c_ord = dr.day_pattern("ordinary", 0)
    s2[:dr.NP, :24], c2[:dr.NP, :24] = s_ord, c_ord
    # the same load_kwh / row sum as before, so that December 31 itself is unchanged
    ssum = lambda t: np.array([np.sum(t[r].astype(np.float64)) for r in a["load_row"]])
    load2, pv2 = dr.agent_hours(a["load_row"], a["cf_row"], a["load_kwh"] * ssum(s2) / ssum(shapes), a["kw"], s2, c2)
    assert np.allclose(load2[:, 24:], load[:, 24:], rtol=1e-15, atol=0.0) and np.array_equal(pv2[:, 24:], pv[:, 24:])
    cfg = orc.make_cfg(batt_update_hours=1)
    moved = 0
    for i in range(dr.NP):
        x = orc.batt_dispatch(load[i], pv[i], bank[i], power[i], cfg)[1][-24:]
        y = orc.batt_dispatch(load2[i], pv2[i], bank[i], power[i], cfg)[1][-24:]
        moved += not np.allclose(x, y, rtol=1e-9, atol=1e-9)
    print(f"December 31 dispatch changed by January 1 on {moved} of {dr.NP} rows")
    assert moved >= 1


@pytest.mark.parametrize("shift", dr.REPLAY_SHIFTS)
def test_replay_rule_leaves_out_few_agents(shift):
    """tests/test_gpu_replay_at.py's ambiguity rule on the constructed agents
    at the banks of test_replay_at_caller_given_banks, from the reference
    alone: at most 10 % of the agents of a case."""
    from tests.test_batt_metrics import summary_ref
    from tests.test_gpu_replay_at import _ambiguous
    a, load, pv, _, _ = _agents(130)
    kwh, pkw = dr.replay_banks(a, shift)
    cfg = orc.make_cfg()
    amb = 0
    for i in range(130):
        bank, power = (0.0, 0.0) if kwh[i] == 0.0 else orc.batt_size(pkw[i], kwh[i], 240.0, cfg)
        amb += _ambiguous(summary_ref(load[i], pv[i], bank, power, cfg)["_hours"], power, cfg)
    print(f"shift {shift}: {amb} of 130 agents ambiguous")
    assert amb <= dr.REPLAY_LEFT_OUT_CAP * 130
