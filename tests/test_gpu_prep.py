"""The profile-prep kernels (k_row_pairwise_shape / _cf, k_row_slots_shape /
_cf) through dgen_prep_shapes / dgen_prep_cfs, at the block edges of both
launches (R = 1, 129, 257: row blocks of 128, slot blocks of 256 over R * 576)
and on rows that pin the summation order and the calendar.

Row sums are numpy's, bit for bit: ``row.astype(float64).sum()`` and
``(row.astype(float64) / 1e6).sum()``.  The float32 rows are signed and span
twelve decades, on which a pairwise sum without numpy's 8192-element chunks
gives other bits (tests/test_market_refs.py).  Slot sums are the float64 sums
in ascending day order over a calendar written out in tests/market_refs.py
(Monday start, 365 days), bit for bit.  Every output buffer is one row longer
than needed and the extra row must keep its sentinel."""
import numpy as np
import pytest
import torch

from dgen_amd import _lib
from tests import market_refs as mr

pytestmark = pytest.mark.gpu

E_ARG = -1                                   # DGEN_E_ARG
SENTINEL = -7.25
ROWS = [1, 129, 257]


def _prep(engine, which, rows):
    """(row_sum [R], slots [R, 576], the two guard rows) of dgen_prep_<which>."""
    R = rows.shape[0]
    d = torch.from_numpy(np.array(rows, copy=True, order="C")).to(engine.dev)
    s = torch.full((R + 1,), SENTINEL, dtype=torch.float64, device=engine.dev)
    sl = torch.full((R + 1, mr.NSLOT), SENTINEL, dtype=torch.float64, device=engine.dev)
    fn = engine.lib.dgen_prep_shapes if which == "shapes" else engine.lib.dgen_prep_cfs
    _lib.check(fn(engine.ctx, d.data_ptr(), R, s.data_ptr(), sl.data_ptr(), engine.stream_handle()),
               f"dgen_prep_{which}")
    torch.cuda.synchronize(engine.dev)
    s, sl = s.cpu().numpy(), sl.cpu().numpy()
    return s[:R], sl[:R], s[R:], sl[R:]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("R", ROWS)
def test_shape_rows(engine, R):
    rows = mr.shape_rows(R)
    got_sum, got_slots, g1, g2 = _prep(engine, "shapes", rows)
    assert (g1 == SENTINEL).all() and (g2 == SENTINEL).all()
    r64 = rows.astype(np.float64)
    want = np.array([row.astype(np.float64).sum() for row in rows])
    bad = np.flatnonzero(got_sum != want)
    assert bad.size == 0, (bad[:5], got_sum[bad[:5]], want[bad[:5]])
    assert _same_bits(got_slots, mr.slot_sums(r64))
    for k, name in enumerate(mr.SHAPE_SPECIAL, start=1):
        if k >= R:
            break
        if name == "zeros":
            assert not got_sum[k] and not got_slots[k].any()
        elif name == "ones":
            cnt = mr.slot_day_counts()
            assert got_sum[k] == 8760.0
            assert np.array_equal(got_slots[k], cnt.astype(np.float64)) and got_slots[k].sum() == 8760.0
        elif name == "index":
            assert got_sum[k] == 8760 * 8759 / 2
        else:
            assert got_sum[k] == 3.25 and np.count_nonzero(got_slots[k]) == 1
    for k in mr.shape_positive_rows(R):
        assert abs(got_slots[k].sum() - got_sum[k]) <= 1e-9 * got_sum[k], k


@pytest.mark.parametrize("R", ROWS)
def test_cf_rows(engine, R):
    rows = mr.cf_rows(R)
    got_sum, got_slots, g1, g2 = _prep(engine, "cfs", rows)
    assert (g1 == SENTINEL).all() and (g2 == SENTINEL).all()
    want = np.array([(row.astype(np.float64) / 1e6).sum() for row in rows])
    bad = np.flatnonzero(got_sum != want)
    assert bad.size == 0, (bad[:5], got_sum[bad[:5]], want[bad[:5]])
    assert _same_bits(got_slots, mr.slot_sums(rows.astype(np.float64) / 1e6))
    for k in mr.cf_positive_rows(R):
        assert got_sum[k] > 0 and abs(got_slots[k].sum() - got_sum[k]) <= 1e-9 * got_sum[k], k


@pytest.mark.parametrize("which", ["shapes", "cfs"])
def test_bad_arguments_are_refused_with_a_message(engine, which):
    fn, other = engine.lib.dgen_prep_shapes, engine.lib.dgen_prep_cfs
    if which == "cfs":
        fn, other = other, fn
    dt = torch.float32 if which == "shapes" else torch.int32
    d = torch.zeros((1, mr.NH), dtype=dt, device=engine.dev)
    s = torch.full((2,), SENTINEL, dtype=torch.float64, device=engine.dev)
    sl = torch.full((2, mr.NSLOT), SENTINEL, dtype=torch.float64, device=engine.dev)
    st = engine.stream_handle()
    good = [engine.ctx, d.data_ptr(), 1, s.data_ptr(), sl.data_ptr(), st]
    cases = {"n_rows = 0": (2, 0), "n_rows < 0": (2, -1), "no context": (0, None), "no rows": (1, None),
             "no row sums": (3, None), "no slot sums": (4, None)}
    for what, (pos, val) in cases.items():
        args = list(good)
        args[pos] = val
        # an earlier message must not stand in for this call's
        assert other(None, None, 0, None, None, None) == E_ARG
        assert f"dgen_prep_{which}" not in _lib.last_error()
        assert fn(*args) == E_ARG, what
        assert f"dgen_prep_{which}" in _lib.last_error(), what
    torch.cuda.synchronize(engine.dev)
    assert (s == SENTINEL).all() and (sl == SENTINEL).all()
    assert fn(*good) == 0
    torch.cuda.synchronize(engine.dev)
    assert s[0] == 0 and s[1] == SENTINEL and not sl[0].any() and (sl[1] == SENTINEL).all()
