"""The references of tests/reduction_refs.py discriminate (CPU only): on the
exact inputs tests/test_gpu_reductions.py feeds the device, a numpy model of
each kernel's arithmetic stays within bound() of the exact reference, and each
subtly wrong variant of it exceeds bound() on at least one output."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import reduction_refs as rr

SEG_MUTANTS = {"f32_accumulator": dict(acc_dtype=np.float32), "drop_last": dict(drop_last=True),
               "dup_lo_256": dict(dup256=True)}
HOURLY_MUTANTS = dict(SEG_MUTANTS, no_div_1000=dict(no_div=True), swap_pvo_batt=dict(swap_w=True))
NONEMPTY = np.array(rr.SEG_COUNTS) > 0


def _err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref)


def test_exact_products_agree_with_fractions():
    rng = np.random.default_rng(1)
    a = rr._signed_mags(rng, 40)
    b = rr._signed_mags(rng, 40).astype(np.float32)
    q, A = rr._exact_products([(a, b), (b, a[::-1])])
    ref = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)) + \
        sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(b, a[::-1]))
    assert q == ref
    assert A == sum(abs(Fraction(float(x)) * Fraction(float(y))) for x, y in zip(a, b)) + \
        sum(abs(Fraction(float(x)) * Fraction(float(y))) for x, y in zip(b, a[::-1]))
    # what float64 summation loses, the reference keeps
    s, A = rr.exact_segment_sums(np.array([[1e16, 1.0, -1e16, 2.0 ** -60]]), None, None, None, [0, 0, 4])
    assert s.tolist() == [[0.0], [1.0]] and A[1, 0] > 2e16 and A[0, 0] == 0.0
    with pytest.raises(ValueError):
        rr.exact_segment_sums(np.array([[np.nan]]), None, None, None, [0, 1])


def test_bound_steps_with_the_member_count():
    u = 2.0 ** -53
    assert rr.bound(0, 3.0) == 16 * u * 3.0 and rr.bound(1, 1.0) == 17 * u
    assert rr.bound(256, 1.0) == 17 * u and rr.bound(257, 1.0) == 18 * u and rr.bound(513, 1.0) == 19 * u
    assert rr.seg_bound(rr.SEG_OFF, np.ones((13, 5))).shape == (13, 5)
    assert int(rr.SEG_OFF[-1]) == rr.N_MEMBERS == 1985 < rr.N_COLS == 2200


def test_inputs_are_cancellation_heavy():
    for dtype in ("f32", "f64"):
        for form in rr.SEGMENT_FORMS:
            s, A = rr.segment_reference(dtype, form)
            s, A = s[NONEMPTY], A[NONEMPTY]
            assert (s != 0).mean() > 0.9
            assert np.median(A[s != 0] / np.abs(s[s != 0])) > 50.0, (dtype, form)
            v1 = rr.segment_case(dtype, form, rr.K_MAX)[0]
            mag = np.abs(v1[:, :rr.N_MEMBERS])
            assert mag.min() < 1e-2 and mag.max() > 1e5 and (v1[:, :rr.N_MEMBERS] < 0).mean() > 0.3
            assert np.isnan(v1[:, rr.N_MEMBERS:]).all()
    for kind in ("none", "scatter"):
        s, A = rr.hourly_reference(kind)
        s, A = s[NONEMPTY], A[NONEMPTY]
        assert (s != 0).mean() > 0.9
        assert np.median(A[s != 0] / np.abs(s[s != 0])) > 50.0, kind


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("form", rr.SEGMENT_FORMS)
def test_segment_sums_reference_discriminates(dtype, form):
    args = rr.segment_case(dtype, form, rr.K_MAX)
    ref, A = rr.segment_reference(dtype, form)
    tol = rr.seg_bound(rr.SEG_OFF, A)
    good = rr.model_segment_sums(*args, rr.SEG_OFF)
    assert (_err(good, ref) <= tol).all()
    assert not good[~NONEMPTY].any() and not ref[~NONEMPTY].any() and not tol[~NONEMPTY].any()
    for name, kw in SEG_MUTANTS.items():
        bad = rr.model_segment_sums(*args, rr.SEG_OFF, **kw)
        assert (_err(bad, ref) > tol).any(), name
    # k = 1 is plane 0 of the k = 7 case
    one = rr.exact_segment_sums(*rr.segment_case(dtype, form, 1), rr.SEG_OFF)
    assert np.array_equal(one[0][:, 0], ref[:, 0]) and np.array_equal(one[1][:, 0], A[:, 0])


@pytest.mark.parametrize("kind,nh", [("none", rr.NH_MAX), ("scatter", rr.NH_MAX), ("repeat", 8)])
def test_state_hourly_reference_discriminates(kind, nh):
    planes, w = rr.hourly_inputs()
    planes = [p[:nh] for p in planes]
    idx = rr.hourly_idx(kind)
    ref, A = rr.hourly_reference(kind, nh)
    tol = rr.seg_bound(rr.SEG_OFF, A)
    good = rr.model_state_hourly(*planes, w, idx, rr.SEG_OFF)
    assert (_err(good, ref) <= tol).all()
    assert not good[~NONEMPTY].any() and not ref[~NONEMPTY].any() and not tol[~NONEMPTY].any()
    for name, kw in HOURLY_MUTANTS.items():
        bad = rr.model_state_hourly(*planes, w, idx, rr.SEG_OFF, **kw)
        assert (_err(bad, ref) > tol).any(), name
    # the unused columns do not enter the reference: poisoned copies give the same model bits
    mp = rr.mask_unused(planes, idx)
    mw = rr.mask_unused(w, idx)
    assert len(rr.unused_columns(idx)) >= rr.N_COLS - rr.N_MEMBERS and np.isnan(mp[0]).any()
    assert np.array_equal(rr.model_state_hourly(*mp, mw, idx, rr.SEG_OFF), good)


def test_hourly_reference_of_fewer_hours_is_a_prefix():
    ref, A = rr.hourly_reference("scatter")
    planes, w = rr.hourly_inputs()
    s5, a5 = rr.exact_state_hourly(*(p[:5] for p in planes), w, rr.hourly_idx("scatter"), rr.SEG_OFF)
    assert np.array_equal(s5, ref[:, :5]) and np.array_equal(a5, A[:, :5])
    ident, _ = rr.exact_state_hourly(*(p[:2] for p in planes), w, rr.hourly_idx("identity"), rr.SEG_OFF)
    assert np.array_equal(ident, rr.hourly_reference("none")[0][:, :2])
    rep = rr.hourly_idx("repeat")
    assert len(np.unique(rep)) < len(rep) and rep[rr.SEG_OFF[11]] == rep[rr.SEG_OFF[8]]


def test_rows_sequential_order_differs_from_pairwise():
    import torch
    from dgen_amd.partition import host_seq_sum
    rows = rr.rows_inputs()
    assert rows.shape == (300, 257)
    seq = host_seq_sum(torch.from_numpy(rows.copy()), rr.ROW_OFF).numpy()
    pair = rr.pairwise_rows_sum(rows, rr.ROW_OFF)
    for s, m in enumerate(rr.ROW_COUNTS):
        if m == 0:
            assert not seq[s].any()
        elif m < 8:                                   # below numpy's unrolling both orders coincide
            assert np.array_equal(seq[s], pair[s])
        else:
            assert (seq[s] != pair[s]).mean() > 0.25, m
            assert np.allclose(seq[s], pair[s], rtol=0, atol=1e-6 * np.abs(rows).max())


def test_weights_table_reaches_every_path():
    from oracle import attach as oa
    t = rr.weights_table()
    assert len(t) <= 255
    cust, adopt, cum, kw, added = rr.weights_columns(len(t))
    w = oa.weights(cust, adopt, cum, kw, added)
    assert np.isnan(cust).sum() == 1 and np.isnan(w[2]).sum() == 1 and np.isfinite(w[:2]).all()
    assert (cust < adopt).any() and (w[2][cust < adopt] == 0.0).all()
    assert (w[1] == 0).any() and (w[0] == 0).any() and (w[0] > 0).any() and w[1].max() < 2.0 ** 53
    assert {0.0, -3.0, 1e-12} <= set(kw.tolist()) and ((kw == 0.0) & (w[1] > 1e6)).any()
    # rint's half-to-even on the ties, one below a tie, added = -10 clamping at 0
    pick = lambda a, k, c, ad: w[:, [i for i, r in enumerate(t) if r[1:] == (a, c, k, ad)][0]]
    assert pick(2.5, 0.25, 0.625, 0)[:2].tolist() == [0.0, 2.0]
    assert pick(1.5, 0.25, 0.0, 0)[:2].tolist() == [2.0, 0.0]
    assert pick(0.5, 8.0, 28.0, 0)[:2].tolist() == [0.0, 4.0]
    assert pick(1e6 + 0.5, 8.0, 20.0, 3)[:2].tolist() == [1e6 - 5.0, 5.0]
    assert pick(3.49999, 8.0, 8.0 * math.nextafter(4.5, 0.0), 0)[:2].tolist() == [0.0, 4.0]
    assert pick(2.5, 8.0, 28.0, -10)[:2].tolist() == [2.0, 0.0]
