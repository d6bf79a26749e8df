"""The tiered bills' period shares from one reciprocal, on the device:
dgen_share_selftest runs the kernels' own helper (share_window, recip_rn,
div_by_recip) beside the plain quotient, and a sizing call over tiered tariffs
gives the outputs recorded before the change (tests/golden/tiered_share_outputs.npz)."""
import os

import numpy as np
import pytest
import torch

from dgen_amd.engine import outputs_to_host
from dgen_amd.synth import make_population

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "tiered_share_outputs.npz")
LO, HI = 2.0 ** -256, 2.0 ** 256
ONES = (1 << 52) - 1


def _mk(e, mant):
    b = ((np.asarray(e, np.int64) + 1023).astype(np.uint64) << np.uint64(52)) | (
        np.asarray(mant, np.uint64) & np.uint64(ONES))
    return b.view(np.float64)


def _in_window(u, U):
    """share_window's statement for one u per month (the other registers 0)."""
    lo_ones = (U.view(np.uint64) & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF)
    with np.errstate(invalid="ignore"):
        u_ok = (u.view(np.uint64) == 0) | ((u >= LO) & (u < HI))
        return (U >= LO) & (U < HI) & ~lo_ones & u_ok


def _random_pairs(n, seed=20263100):
    """check_share_div.c's mix: shares of U, any exponent of the band at or
    below U's, a few ulps below U, and anywhere in the band."""
    rng = np.random.default_rng(seed)
    eU = rng.integers(-256, 256, n)
    U = _mk(eU, rng.integers(0, 1 << 52, n, dtype=np.uint64))
    kind = rng.integers(0, 8, n)
    frac = rng.integers(0, 1 << 53, n, dtype=np.uint64).astype(np.float64) * 2.0 ** -53
    mant = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    below = _mk(-256 + (rng.integers(0, 1 << 30, n) % (eU + 257)), mant)
    anyw = _mk(rng.integers(-256, 256, n), mant)
    near = (U.view(np.uint64) - rng.integers(0, 8, n).astype(np.uint64)).view(np.float64)
    u = np.where(kind < 4, U * frac, np.where(kind < 6, np.minimum(below, U), np.where(kind == 6, near, anyw)))
    u = np.where((u != 0.0) & (u < LO), 0.0, u)
    return np.ascontiguousarray(u), np.ascontiguousarray(U)


def _adversarial():
    u, U, fast = [], [], []

    def add(a, b, f):
        u.append(a); U.append(b); fast.append(f)

    for e in (-256, -255, -1, 0, 1, 52, 255):
        for m in (0, 1, ONES - 1, ONES ^ (1 << 31), (ONES ^ (1 << 51)) - 1, 1 << 51, (1 << 51) - 2):
            b = float(_mk(e, m))
            add(0.0, b, 1); add(b, b, 1); add(float(_mk(-256, 0)), b, 1); add(float(_mk(255, ONES)), b, 1)
            if m:
                add(float(np.nextafter(b, 0.0)), b, 1)
        add(float(_mk(e, 0x123)), float(_mk(e, ONES)), 0)             # significand of all ones
        add(float(_mk(e, 0)), float(_mk(e, 0xABCDEFFFFFFFF)), 0)      # low word all ones
    for a, b in ((0.0, float(np.nextafter(LO, 0.0))), (1.0, HI), (1.0, 2.0 ** 1023), (float(np.nextafter(LO, 0.0)), 1.0),
                 (2.0 ** -1000, 1.0), (2.0 ** -1022, 1.0), (5e-324, 1.0), (2.0 ** -1050, 1.0), (HI, 1.0), (-0.0, 1.0),
                 (-1.0, 2.0), (np.inf, 1.0), (np.nan, 1.0), (1.0, 0.0), (1.0, -1.0), (1.0, np.inf), (1.0, np.nan),
                 (0.0, 2.0 ** -1060)):
        add(a, b, 0)
    return np.array(u), np.array(U), np.array(fast, np.int32)


def test_helper_equals_the_device_quotient(engine):
    ur, Ur = _random_pairs(1 << 20)
    ua, Ua, fa = _adversarial()
    u, U = np.concatenate([ur, ua]), np.concatenate([Ur, Ua])
    q, ref, fast = engine.share_selftest(u, U)
    # the helper's result is the device's own u / U, bit for bit (NaNs by their bits too)
    diff = np.flatnonzero(q.view(np.uint64) != ref.view(np.uint64))
    print(f"{u.size} pairs, {diff.size} differ, fast path on {int(fast.sum())}")
    assert diff.size == 0, (u[diff[:5]], U[diff[:5]], q[diff[:5]], ref[diff[:5]])
    # and the host's (IEEE division on both sides)
    with np.errstate(all="ignore"):
        host = u / U
    assert np.array_equal(ref.view(np.uint64)[~np.isnan(host)], host.view(np.uint64)[~np.isnan(host)])
    # the window is the stated one: the fast path exactly on the pairs inside it
    inside = _in_window(u, U)
    assert np.array_equal(fast.astype(bool), inside)
    assert np.array_equal(fast[ur.size:], fa)
    # and the test does not pass by falling back
    assert inside[:ur.size].mean() > 0.99 and fast[:ur.size][inside[:ur.size]].mean() > 0.99


def test_four_live_registers_a_month(engine):
    """Months as the bills see them: up to four non-zero billed-kWh registers
    and their running sum as the divisor.  Every share equals the device
    quotient; the month takes the reciprocal path exactly when U and all four
    registers are inside the window, so one bad register declines the month."""
    rng = np.random.default_rng(20263103)
    n = 1 << 18
    e0 = rng.integers(-200, 200, n)
    u = _mk(e0[:, None] - rng.integers(0, 40, (n, 4)), rng.integers(0, 1 << 52, (n, 4), dtype=np.uint64))
    u = np.where(rng.random((n, 4)) < 0.3, 0.0, u)                  # periods that billed nothing
    bad = rng.random(n) < 0.02                                      # one register outside the window
    col = rng.integers(0, 4, n)
    vals = np.array([2.0 ** -300, 5e-324, -0.0, -1.0, 2.0 ** 300, np.nan, np.inf])
    u[np.flatnonzero(bad), col[bad]] = vals[rng.integers(0, vals.size, int(bad.sum()))]
    with np.errstate(all="ignore"):
        U = ((u[:, 0] + u[:, 1]) + u[:, 2]) + u[:, 3]               # the bills' order
    U = np.where(U > 0.0, U, 1.0)                                   # (the bills skip such months)
    q, ref, fast = engine.share_selftest(u, U)
    assert q.shape == ref.shape == (n, 4)
    diff = np.flatnonzero((q.view(np.uint64) != ref.view(np.uint64)).any(axis=1))
    with np.errstate(all="ignore"):
        host = u / U[:, None]
    ok = ~np.isnan(host)
    inside = np.logical_and.reduce([_in_window(np.ascontiguousarray(u[:, p]), U) for p in range(4)])
    print(f"{n} months, {diff.size} differ, fast path on {int(fast.sum())}, inside {int(inside.sum())}, "
          f"with a bad register {int(bad.sum())}")
    assert diff.size == 0, (u[diff[:3]], U[diff[:3]], q[diff[:3]], ref[diff[:3]])
    assert np.array_equal(ref.view(np.uint64)[ok], host.view(np.uint64)[ok])
    assert np.array_equal(fast.astype(bool), inside)
    assert not fast[bad & ~np.isinf(U) & ~np.isnan(U)].any() and fast[~bad].mean() > 0.99


CASES = (("res_1m_nem_tou", 256, 20263101), ("national_mixed", 128, 20263102))


def _pop(cfg, n, seed):
    return make_population(cfg, n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32, n_counties=16, n_tariffs=48)


@pytest.mark.parametrize("cfg,n,seed", CASES)
def test_sizing_outputs_are_the_recorded_ones(engine, cfg, n, seed):
    """One sizing call (search, scan and with-battery finance) over tariffs of
    every P in 1..4 and T in 1..3 -- NEM kWh for res_1m_nem_tou; national_mixed
    adds net billing -- equals the outputs recorded from the library before the
    shares moved to the shared reciprocal: every scalar and yearly output,
    array_equal."""
    pop = _pop(cfg, n, seed)
    t = pop.tariffs[pop.cols["tariff0"]]
    if cfg == "res_1m_nem_tou":
        assert {(p, k) for p in range(1, 5) for k in range(1, 4)} <= set(zip(t["P"].tolist(), t["T"].tolist()))
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs, None)
    engine.set_switches(pop.switches)
    batch = engine.upload_agents(pop.cols, pop.n_scratch)
    # two agents of one wave (neighbours in device order) with different tier counts
    td = pop.tariffs[pop.cols["tariff0"][np.asarray(batch.perm)]]["T"] if batch.perm is not None else t["T"]
    assert (td[0::2] != td[1::2]).any()
    out = engine.alloc_outputs(batch.n, hourly=False)
    engine.size(batch, out)
    torch.cuda.synchronize()
    o = outputs_to_host(out)
    gold = np.load(GOLDEN)
    names = [k[len(cfg) + 1:] for k in gold.files if k.startswith(cfg + ".")]
    assert len(names) >= 10
    for k in names:
        assert np.array_equal(o[k], gold[f"{cfg}.{k}"], equal_nan=True), k
