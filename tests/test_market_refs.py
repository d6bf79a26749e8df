"""CPU checks of tests/market_refs.py (no GPU): the references are what they
claim to be, and the shared inputs tell a subtly wrong kernel from a right one
(tests/test_gpu_prep.py, tests/test_gpu_market_edges.py use the same inputs)."""
import numpy as np
import pandas as pd
import pytest

from dgen_amd import diffusion as gd
from oracle import market as om
from tests import market_refs as mr


# ------------------------------------------------------------ numpy-order sum
@pytest.fixture(scope="module")
def adv40():
    return mr.adversarial_rows(40, 7).astype(np.float64)


def test_kernel_order_restatement_is_numpy_bit_for_bit(adv40):
    """Chunks of 8192, pairwise split rounded to 8, 8-accumulator leaves <= 128
    equals both numpy forms the device is held to, on signed twelve-decade data."""
    f32 = mr.adversarial_rows(40, 7)
    want_shape = np.array([row.astype(np.float64).sum() for row in f32])
    assert np.array_equal(mr.np_order_sum(adv40), want_shape)
    cf = mr.cf_rows(8)
    want_cf = np.array([(row.astype(np.float64) / 1e6).sum() for row in cf])
    assert np.array_equal(mr.np_order_sum(cf.astype(np.float64) / 1e6), want_cf)


def test_other_summation_orders_differ_on_this_data(adv40):
    """Without the 8192 chunking (one pairwise sum over 8760), with a chunk of
    8760, or sequentially, most of the 40 rows sum to other bits: the data pins
    the order.  (Recorded: 30 of 40 rows differ without the chunking.)"""
    want = mr.np_order_sum(adv40)
    unchunked = mr.np_order_sum(adv40, chunk=None)
    assert np.array_equal(unchunked, mr.np_order_sum(adv40, chunk=8760))
    differ = int((unchunked != want).sum())
    print(f"rows differing without the 8192 chunk: {differ} of 40")
    assert differ >= 20
    assert (np.cumsum(adv40, axis=1)[:, -1] != want).sum() >= 20
    # the same holds for the rows the GPU test uploads (257-row case)
    rows = mr.shape_rows(257)[8:72].astype(np.float64)
    assert (mr.np_order_sum(rows, chunk=None) != mr.np_order_sum(rows)).sum() >= 32


# ------------------------------------------------------------------- calendar
def test_calendar_totals():
    cnt = mr.slot_day_counts()
    assert cnt.shape == (576,) and cnt.sum() == 8760
    per_month = cnt.reshape(12, 2, 24)
    assert (per_month == per_month[:, :, :1]).all()                       # every hour of day alike
    assert (per_month[:, :, 0].sum(axis=1) == np.array(mr.MONTH_DAYS)).all()
    # day 0 is a Monday: January has the weekends 5-6, 12-13, 19-20, 26-27
    assert per_month[0, 1, 0] == 8 and per_month[0, 0, 0] == 23
    # 52 weeks and a day: 104 weekend days, the spare day (31 Dec) a Monday
    assert per_month[:, 1, 0].sum() == 104 and per_month[:, 0, 0].sum() == 261
    # February starts on day 31, a Thursday: weekends 33-34, ..., 54-55
    assert mr.slot_days()[48 + 24][:2] == [33, 34] and mr.slot_days()[48][0] == 31
    days = [d for s in range(0, 576, 24) for d in mr.slot_days()[s]]
    assert sorted(days) == list(range(365))


def test_slot_sums_reference_on_known_rows():
    rows = mr.shape_rows(9).astype(np.float64)
    s = mr.slot_sums(rows)
    ones = 1 + mr.SHAPE_SPECIAL.index("ones")
    assert np.array_equal(s[ones], mr.slot_day_counts().astype(np.float64))
    for hour in mr.SINGLE_HOURS:
        k = 1 + mr.SHAPE_SPECIAL.index(f"hour{hour}")
        assert np.count_nonzero(s[k]) == 1 and s[k].sum() == 3.25
        d, hod = divmod(hour, 24)
        m = int(np.searchsorted(np.cumsum(mr.MONTH_DAYS), d, side="right"))
        assert s[k, m * 48 + (24 if d % 7 >= 5 else 0) + hod] == 3.25
    # a straightforward per-slot loop gives the same bits as the vectorised form
    row = rows[0]
    for slot in (0, 47, 100, 575):
        acc = 0.0
        for d in mr.slot_days()[slot]:
            acc += row[d * 24 + slot % 24]
        assert s[0, slot] == acc
    # a weekend rule of > 5, or a month starting a day late, moves the ones row
    idx = 1 + mr.SHAPE_SPECIAL.index("index")
    assert s[idx].sum() == 8760 * 8759 / 2


# ----------------------------------------------------------------- Kahan sums
def test_kahan_weights_tell_the_compensation():
    for m in (257, 700):
        w = mr.kahan_weights(m)
        kahan, cnt = om.group_sum_kahan(w)
        assert cnt == m
        assert kahan != mr.seq_sum(w)
        assert kahan == pd.Series(w).groupby(np.zeros(m, dtype=int)).sum().iloc[0]
        import math
        assert kahan == math.fsum(w)                      # here the compensated sum is the exact one


def test_initial_shares_case_layout():
    c = mr.initial_shares_case()
    kind = c["kind"]
    n = len(kind)
    assert n == sum(m for m, _ in mr.INIT_GROUPS.values())
    assert not np.array_equal(c["dev_index"], np.arange(n)) and sorted(c["dev_index"]) == list(range(n))
    # interleaved: no group is a contiguous run of frame rows
    for k in ("some_nan", "all_zero", "one_zero", "kahan"):
        rows = np.flatnonzero(kind == k)
        assert rows[-1] - rows[0] + 1 > rows.size
    w = c["weight"]
    assert np.isnan(w[kind == "all_nan"]).all() and (w[kind == "all_zero"] == 0).all()
    assert 0 < np.isnan(w[kind == "some_nan"]).sum() < 255
    z = np.flatnonzero(w[kind == "one_zero"] == 0)
    assert z.tolist() == [256]                            # past the first 256 members
    kw = w[kind == "kahan"]
    assert kw[0] == 1e8 and om.group_sum_kahan(kw)[0] != mr.seq_sum(kw)
    assert ("DD", "res") not in set(zip(c["caps"]["state_abbr"], c["caps"]["sector_abbr"]))


def test_oracle_seeding_follows_pandas_everywhere():
    """oracle.market.initial_market_shares against the pandas operations on the
    edge case, bit for bit -- the all-NaN group included: pandas counts 0
    members, 1 / 0 = inf, and inf is not filled by fillna(0)."""
    c = mr.initial_shares_case()
    ref, tot, cnt = mr.initial_shares_pandas(c)
    got = om.initial_market_shares(c["state"], c["sector"], c["tech"], c["weight"], c["capex"], c["caps"])
    for k in mr.INIT_COLS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
        assert not np.isnan(got[k]).any(), k
    for k, src in mr.INIT_COPIES.items():
        assert np.array_equal(got[k], ref[src]), k
    assert not got["initial_market_value"].any()
    kind = c["kind"]
    assert cnt.loc[("CC", "ind", "solar")] == 0 and tot.loc[("CC", "ind", "solar")] == 0.0
    assert np.isposinf(got["adopters_cum_last_year"][kind == "all_nan"]).all()
    assert np.isposinf(got["market_value_last_year"][kind == "all_nan"]).all()
    assert (got["market_share_last_year"][kind == "all_nan"] == 0).all()          # adopt / NaN -> fillna
    zero = kind == "all_zero"
    assert np.array_equal(got["adopters_cum_last_year"][zero],
                          np.full(256, (1.0 / 256) * c["caps"]["pv_systems_count"][2]))
    assert all((got[k][kind == "no_caps"] == 0).all() for k in mr.INIT_COLS)
    for key, (m, _) in mr.INIT_GROUPS.items():
        rows = [i for i in range(len(kind)) if (c["state"][i], c["sector"][i], c["tech"][i]) == key]
        s, k = om.group_sum_kahan(c["weight"][rows])
        assert (s, k) == (tot.loc[key], cnt.loc[key]) and len(rows) == m


# ------------------------------------------------------- diffusion in mpmath
def test_mp_restatement_agrees_with_the_oracle_where_well_conditioned():
    from oracle import diffusion as od
    a = mr.diffusion_well()
    for first in (True, False):
        got = od.diffusion(*[a[k] for k in mr.DIFF_ARGS], first)
        ref = mr.diffusion_mp(a, first)
        for k in mr.DIFF_OUT:
            assert mr.max_rel_err(got[k], ref[k]) < 1e-13, (first, k)


# The float64 oracle's max relative error against the 50-digit restatement on
# diffusion_ill(), per column, as measured (numpy 2.2 / glibc); the GPU test's
# tolerance is 8 x the value computed at run time, these are the record.
RECORDED_ORACLE_ERROR = {
    # the cancellation-dominated columns (IEEE subtraction, not libm); every
    # other column measured between 5e-17 and 2e-13
    ("slow", True): {"new_market_share": 2.48e-10},
    ("slow", False): {"new_market_share": 2.09e-10},
    ("near", True): {"bass_params_teq": 1.66e-6, "f": 5.22e-5, "new_market_share": 1.89e-4},
    ("near", False): {"bass_params_teq": 1.66e-6, "f": 5.22e-5, "new_market_share": 2.15e-4},
}


@pytest.mark.parametrize("kind", ["slow", "near"])
@pytest.mark.parametrize("first", [True, False])
def test_oracle_error_on_the_ill_conditioned_block(kind, first):
    err = mr.oracle_error(kind, first)
    print(kind, "first" if first else "later", {k: f"{v:.2e}" for k, v in err.items()})
    assert all(np.isfinite(v) for v in err.values()), err       # no branch differs, no zero reference
    assert err["mms_fix_zeros"] == 0.0
    assert err["ratio"] <= 2.0 ** -53                           # one correctly rounded division
    # the block is ill-conditioned: the cancellation is orders above 1e-12 ...
    assert err["new_market_share"] > 1e-11
    # ... and stays a usable bound (8 x it is far below 1)
    assert max(err.values()) < 1e-2
    rec = RECORDED_ORACLE_ERROR.get((kind, first))
    if rec is not None:
        for k, v in rec.items():
            assert err[k] <= 4 * v and v <= 4 * max(err[k], 1e-17), (k, err[k], v)


# ------------------------------------------------------------ max market share
def test_empty_curve_is_not_refused_on_the_host():
    """mms_table on a frame with no payback-period rows: no exception, NaN
    bounds and a 1 x 1 NaN table (pinned as it is; the GPU tests never send
    such bounds to the kernel)."""
    empty = pd.DataFrame({"metric": ["percent_monthly_bill_savings"], "business_model": ["host_owned"],
                          "sector_abbr": ["res"], "payback_period": [1.0], "max_market_share": [0.5]})
    tab, rows, fmin, min_pb, max_pb = gd.mms_table(empty)
    assert tab.shape == (1, 1) and np.isnan(tab).all() and rows == {} and fmin == 0
    assert np.isnan(min_pb) and np.isnan(max_pb)
