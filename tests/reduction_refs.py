"""Exact references, error bound, shared inputs and kernel models for the
reduction and state-export kernels (k_segment_sums, k_rows_seq_sum,
k_state_hourly, k_state_hourly_rows).  CPU only; tests/test_gpu_reductions.py
compares the device against it, tests/test_reduction_refs.py proves on the
same inputs that the comparison discriminates.

References
----------
Every double is mant * 2**exp with an integer mant; the products and their
sums are taken in Python integers at a common exponent, so nothing rounds until
the one conversion of the rational result to float64 (int / int true division
is correctly rounded).  `A`, the sum of the absolute products of an output, is
rounded up.

The bound
---------
The library is built with -ffp-contract=off, so the kernels' arithmetic is
plain IEEE-754 binary64 with u = 2**-53 per operation.  A computed sum of
terms equals sum t_i * (1 + th_i) with |th_i| <= k_i u / (1 - k_i u), k_i the
number of roundings on term i's path to the output (Higham, Accuracy and
Stability of Numerical Algorithms, lemma 3.1), hence |got - exact| <=
max_i(k_i) u A up to second order.  The longest path of a member of a segment
of m members through k_state_hourly is

    1                 its product (value * weight)
    2                 the two adds inside the term, (p*a + w*b) + v*d
    ceil(m / 256)     the thread's sequential adds (members lo + t + 256 r)
    8                 tree levels (k_segment_sums: 8 LDS levels over 256
                      partials; k_state_hourly: 6 butterfly levels over a wave
                      and 3 sequential adds of the wave partials, one more than
                      8 -- taken from the spare terms below)
    1                 the division by 1000

that is ceil(m / 256) + 12 roundings.  k_segment_sums has no division and at
most one inner add, so it stays below that.  Four spare terms cover the second
order terms (k u)**2 A (k < 20: below 2**-100 A), the ninth add of
k_state_hourly's tree, the reference's own final rounding (<= u |exact| <= u A)
and the rounding of the test's subtraction:

    bound(m, A) = (ceil(m / 256) + 16) * 2**-53 * A

An empty segment has A = 0: its output must be exactly 0.  This docstring is
the only place the number lives; the tests call bound().

dgen_rows_seq_sum's order ((r0 + r1) + r2) + ... is fixed by the ABI, so its
reference is dgen_amd.partition.host_seq_sum and the comparison is bit for bit.

Inputs
------
All inputs are cancellation-heavy on purpose: mixed signs, magnitudes from
about 1e-3 to 1e6, and terms that nearly cancel (neighbouring columns in the
segment-sum planes, the three products of one column in the hourly planes), so
that A / |sum| is large while the sums stay nonzero.  A kernel that drops,
repeats or mis-weights a member, or accumulates in float32, then misses the
bound by orders of magnitude (tests/test_reduction_refs.py).
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

# One segment table for every test: 13 segments over 2200 columns, 1985 of them
# members, so seg_off[-1] < n and the last 215 columns belong to nobody.
SEG_COUNTS = (0, 0, 1, 63, 64, 65, 255, 256, 257, 0, 511, 513, 0)
N_COLS = 2200
SEG_OFF = np.concatenate([[0], np.cumsum(SEG_COUNTS)]).astype(np.int64)
N_MEMBERS = int(SEG_OFF[-1])
NH_MAX = 56
K_MAX = 7
# dgen_rows_seq_sum
ROW_COUNTS = (0, 0, 1, 2, 17, 0, 280)
ROW_OFF = np.concatenate([[0], np.cumsum(ROW_COUNTS)]).astype(np.int64)
ROW_K = 257
# the combined-plane / rows-form batch (700 agents, 700 members)
BATCH_COUNTS = (0, 1, 255, 257, 0, 187)
BATCH_OFF = np.concatenate([[0], np.cumsum(BATCH_COUNTS)]).astype(np.int64)


def bound(m, A):
    """(ceil(m / 256) + 16) * 2**-53 * A: see the module docstring."""
    return (np.ceil(np.asarray(m, dtype=np.float64) / 256.0) + 16.0) * 2.0 ** -53 * np.asarray(A, np.float64)


def seg_bound(off, A):
    """bound() of a [S, ...] array of A, S = len(off) - 1 segments."""
    m = np.diff(np.asarray(off, dtype=np.int64))
    return bound(m.reshape((-1,) + (1,) * (np.ndim(A) - 1)), A)


# ------------------------------------------------------------ exact arithmetic
def _split(x):
    """x == mant * 2**exp exactly: (int64 mant, |mant| < 2**53; int64 exp)."""
    x = np.ascontiguousarray(x, dtype=np.float64)           # float32 widens exactly
    if not np.isfinite(x).all():
        raise ValueError("the exact reference takes finite values only")
    m, e = np.frexp(x)
    return np.ldexp(m, 53).astype(np.int64), e.astype(np.int64) - 53


def _exact_products(pairs):
    """(sum a*b, sum |a*b|) over all (a, b) array pairs, as Fractions."""
    parts, e0 = [], None
    for a, b in pairs:
        ma, ea = _split(a)
        mb, eb = _split(b)
        e = ea + eb
        if e.size:
            e0 = int(e.min()) if e0 is None else min(e0, int(e.min()))
        parts.append((ma.tolist(), mb.tolist(), e))
    if e0 is None:
        return Fraction(0), Fraction(0)
    tot = atot = 0
    for la, lb, e in parts:
        for x, y, s in zip(la, lb, (e - e0).tolist()):
            p = (x * y) << s
            tot += p
            atot += abs(p)
    scale = Fraction(2) ** e0
    return tot * scale, atot * scale


def _round_up(q: Fraction) -> float:
    a = float(q)
    return a if Fraction(a) >= q else math.nextafter(a, math.inf)


def exact_segment_sums(v1, w1, v2, w2, off):
    """dgen_segment_sums in exact arithmetic.  v1 / v2: [k, n] float32 or
    float64 (v2 None: absent), w1 / w2: [n] float64 (w1 None: weight 1), off:
    [S + 1].  Returns (sums [S, k], A [S, k]): each sum rounded once from the
    exact rational, A = sum |v1 w1| + |v2 w2| rounded up."""
    v1 = np.atleast_2d(np.asarray(v1))
    v2 = None if v2 is None else np.atleast_2d(np.asarray(v2))
    k = v1.shape[0]
    off = np.asarray(off, dtype=np.int64)
    S = len(off) - 1
    sums, A = np.zeros((S, k)), np.zeros((S, k))
    for s in range(S):
        sl = slice(int(off[s]), int(off[s + 1]))
        for j in range(k):
            pairs = [(v1[j, sl], np.ones(sl.stop - sl.start) if w1 is None else np.asarray(w1)[sl])]
            if v2 is not None:
                pairs.append((v2[j, sl], np.asarray(w2)[sl]))
            q, a = _exact_products(pairs)
            sums[s, j], A[s, j] = float(q), _round_up(a)
    return sums, A


def exact_state_hourly(base, pvo, wbt, w, idx, off):
    """dgen_state_hourly in exact arithmetic: out[s, h] = (sum over the members
    c of pvo[h, c] w_pvo[c] + wbt[h, c] w_batt[c] + base[h, c] w_non[c]) / 1000.
    Planes [nh, n] (logical layout), w = (w_pvo, w_batt, w_non), idx the plane
    column of each member (None: the member number), off [S + 1].  Returns
    (sums [S, nh], A [S, nh]), A the three absolute products summed, / 1000."""
    base, pvo, wbt = (np.asarray(p) for p in (base, pvo, wbt))
    wp, wb, wn = (np.asarray(x, dtype=np.float64) for x in w)
    off = np.asarray(off, dtype=np.int64)
    S, nh = len(off) - 1, base.shape[0]
    sums, A = np.zeros((S, nh)), np.zeros((S, nh))
    for s in range(S):
        c = np.arange(int(off[s]), int(off[s + 1]), dtype=np.int64)
        if idx is not None:
            c = np.asarray(idx, dtype=np.int64)[c]
        for h in range(nh):
            q, a = _exact_products([(pvo[h, c], wp[c]), (wbt[h, c], wb[c]), (base[h, c], wn[c])])
            sums[s, h], A[s, h] = float(q / 1000), _round_up(a / 1000)
    return sums, A


# ---------------------------------------------------------------- kernel models
def _block_reduce(terms, acc_dtype, tree):
    """256 threads' strided sequential partials of terms [m, ...], then the
    kernel's tree: "lds" (8 halving levels over the 256 partials) or "waves"
    (6 butterfly levels per 64-lane wave, then ((w0 + w1) + w2) + w3)."""
    m = terms.shape[0]
    rounds = -(-m // 256)
    pad = np.zeros((rounds * 256,) + terms.shape[1:], dtype=acc_dtype)
    pad[:m] = terms
    pad = pad.reshape((rounds, 256) + terms.shape[1:])
    acc = np.zeros((256,) + terms.shape[1:], dtype=acc_dtype)
    for r in range(rounds):
        acc = acc + pad[r]
    if tree == "lds":
        w = 128
        while w:
            acc = acc[:w] + acc[w:2 * w]
            w >>= 1
        return acc[0]
    wv = acc.reshape((4, 64) + terms.shape[1:])
    w = 32
    while w:
        wv = wv[:, :w] + wv[:, w:2 * w]
        w >>= 1
    return ((wv[0, 0] + wv[1, 0]) + wv[2, 0]) + wv[3, 0]


def _mutate_members(c, drop_last, dup256):
    if drop_last and len(c):
        c = c[:-1]
    if dup256 and len(c) > 256:
        c = np.concatenate([c, c[256:257]])
    return c


def model_segment_sums(v1, w1, v2, w2, off, acc_dtype=np.float64, drop_last=False, dup256=False):
    """k_segment_sums' arithmetic in numpy, with the mutants the references
    must catch: a float32 accumulator, the last member of each segment
    dropped, member lo + 256 read twice."""
    v1 = np.atleast_2d(np.asarray(v1))
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros((len(off) - 1, v1.shape[0]))
    for s in range(len(off) - 1):
        c = _mutate_members(np.arange(int(off[s]), int(off[s + 1])), drop_last, dup256)
        t = v1[:, c].astype(np.float64) * (1.0 if w1 is None else np.asarray(w1)[c])
        if v2 is not None:
            t = t + np.atleast_2d(np.asarray(v2))[:, c].astype(np.float64) * np.asarray(w2)[c]
        out[s] = _block_reduce(t.T.astype(acc_dtype), acc_dtype, "lds")
    return out


def model_state_hourly(base, pvo, wbt, w, idx, off, acc_dtype=np.float64, drop_last=False, dup256=False,
                       no_div=False, swap_w=False):
    """k_state_hourly's arithmetic in numpy, with the same mutants and two of
    its own: the division by 1000 omitted, w_pvo and w_batt swapped."""
    wp, wb, wn = (np.asarray(x, dtype=np.float64) for x in w)
    if swap_w:
        wp, wb = wb, wp
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros((len(off) - 1, base.shape[0]))
    for s in range(len(off) - 1):
        c = _mutate_members(np.arange(int(off[s]), int(off[s + 1])), drop_last, dup256)
        if idx is not None:
            c = np.asarray(idx, dtype=np.int64)[c]
        f = lambda p: np.asarray(p)[:, c].astype(np.float64)
        t = (f(pvo) * wp[c] + f(wbt) * wb[c]) + f(base) * wn[c]          # [nh, m]
        r = _block_reduce(t.T.astype(acc_dtype), acc_dtype, "waves").astype(np.float64)
        out[s] = r if no_div else r / 1000.0
    return out


def pairwise_rows_sum(rows, off):
    """np.sum's pairwise order per column: what dgen_rows_seq_sum must NOT be."""
    rows = np.asarray(rows)
    return np.stack([[np.sum(np.ascontiguousarray(rows[off[s]:off[s + 1], j])) for j in range(rows.shape[1])]
                     for s in range(len(off) - 1)])


# ----------------------------------------------------------------------- inputs
def _signed_mags(rng, shape, lo=-3.0, hi=6.0):
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(lo, hi, size=shape)


@functools.lru_cache(maxsize=None)
def segment_inputs():
    """Planes and weights of the segment-sum tests: [K_MAX, N_COLS] float32
    values (and float64 ones that no float32 holds), [N_COLS] weights.  Odd
    columns nearly cancel their left neighbour in every product; the columns
    behind the last segment are NaN everywhere."""
    rng = np.random.default_rng(20261020)
    k, n = K_MAX, N_COLS

    def cancel(v):
        half = v[:, 1::2].shape
        eps = rng.choice([-1.0, 1.0], size=half) * 10.0 ** rng.uniform(-4.0, -2.0, size=half)
        v[:, 1::2] = -v[:, 0::2] * (1.0 + eps)
        return v.astype(np.float32)

    v1, v2 = cancel(_signed_mags(rng, (k, n))), cancel(_signed_mags(rng, (k, n)))
    w1, w2 = _signed_mags(rng, n, -2.0, 2.0), _signed_mags(rng, n, -2.0, 2.0)
    w1[1::2], w2[1::2] = w1[0::2], w2[0::2]                  # the pair shares its weight
    # float64 values with full mantissas (a relative 1e-9 .. 1e-7 away from the float32 ones)
    v1d = v1.astype(np.float64) * (1.0 + rng.uniform(1e-9, 1e-7, (k, n)))
    v2d = v2.astype(np.float64) * (1.0 + rng.uniform(1e-9, 1e-7, (k, n)))
    for a in (v1, v2, v1d, v2d, w1, w2):
        a[..., N_MEMBERS:] = np.nan
        a.setflags(write=False)
    return {"f32": (v1, v2), "f64": (v1d, v2d), "w1": w1, "w2": w2}


SEGMENT_FORMS = ("plain", "w1", "w1_v2_w2")


def segment_case(dtype: str, form: str, k: int):
    """(v1, w1, v2, w2) of one segment-sum case: the first k planes."""
    d = segment_inputs()
    v1, v2 = (a[:k] for a in d[dtype])
    if form == "plain":
        return v1, None, None, None
    if form == "w1":
        return v1, d["w1"], None, None
    return v1, d["w1"], v2, d["w2"]


@functools.lru_cache(maxsize=None)
def segment_reference(dtype: str, form: str):
    """(exact sums, A) [S, K_MAX] of a case; k planes are its first k columns."""
    sums, A = exact_segment_sums(*segment_case(dtype, form, K_MAX), SEG_OFF)
    for a in (sums, A):
        a.setflags(write=False)
    return sums, A


@functools.lru_cache(maxsize=None)
def hourly_inputs():
    """Three [NH_MAX, N_COLS] float32-valued planes (base, pvo, wbt) and the
    three [N_COLS] float64 weights.  Per column and hour the baseline product
    nearly cancels the other two; every entry is finite (mask_unused() poisons
    the columns a case leaves unused)."""
    rng = np.random.default_rng(20261021)
    nh, n = NH_MAX, N_COLS
    pvo = _signed_mags(rng, (nh, n)).astype(np.float32)
    wbt = _signed_mags(rng, (nh, n)).astype(np.float32)
    w = [_signed_mags(rng, n, -1.0, 1.0) for _ in range(3)]
    eps = rng.choice([-1.0, 1.0], size=(nh, n)) * 10.0 ** rng.uniform(-5.0, -2.0, size=(nh, n))
    part = pvo.astype(np.float64) * w[0] + wbt.astype(np.float64) * w[1]
    base = (-part / w[2] * (1.0 + eps)).astype(np.float32)
    for a in (base, pvo, wbt, *w):
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return (base, pvo, wbt), tuple(w)


@functools.lru_cache(maxsize=None)
def hourly_idx(kind: str):
    """Member -> plane column: None ("none"), a fixed permutation of all
    columns of which the members take the first N_MEMBERS ("scatter"), the
    same with every third member reading the column of the member before it
    and one column shared by two segments ("repeat"), arange ("identity")."""
    if kind == "none":
        return None
    if kind == "identity":
        ix = np.arange(N_MEMBERS, dtype=np.int64)
    else:
        ix = np.random.default_rng(20261022).permutation(N_COLS)[:N_MEMBERS].astype(np.int64)
        if kind == "repeat":
            ix[2::3] = ix[1::3][:len(ix[2::3])]
            ix[SEG_OFF[11]] = ix[SEG_OFF[8]]
        elif kind != "scatter":
            raise KeyError(kind)
    ix.setflags(write=False)
    return ix


def unused_columns(idx, n=N_COLS, members=N_MEMBERS):
    """The plane columns no member reads."""
    used = np.arange(members) if idx is None else np.asarray(idx)
    return np.setdiff1d(np.arange(n), used)


def mask_unused(arrays, idx):
    """Copies of [.., N_COLS] arrays with NaN in the columns no member reads:
    a read past the last segment, or of a column outside idx, then shows."""
    dead = unused_columns(idx)
    out = []
    for a in arrays:
        a = np.array(a, copy=True)
        a[..., dead] = np.nan
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def hourly_reference(kind: str, nh: int = NH_MAX):
    """(exact sums, A) [S, nh] of the hourly inputs' first nh hours under
    hourly_idx(kind); hour h does not depend on nh, so cases of fewer hours
    take the leading columns."""
    planes, w = hourly_inputs()
    sums, A = exact_state_hourly(*(p[:nh] for p in planes), w, hourly_idx(kind), SEG_OFF)
    for a in (sums, A):
        a.setflags(write=False)
    return sums, A


@functools.lru_cache(maxsize=None)
def rows_inputs():
    """[300, ROW_K] float64 rows for dgen_rows_seq_sum, mixed signs and
    magnitudes, consecutive rows nearly cancelling."""
    rng = np.random.default_rng(20261023)
    R = int(ROW_OFF[-1])
    rows = _signed_mags(rng, (R, ROW_K))
    rows[1::2] = -rows[0::2] * (1.0 + rng.uniform(1e-9, 1e-3, (R // 2, ROW_K)))
    rows.setflags(write=False)
    return rows


def batch_idx(n: int):
    """A scattered member -> device row map for the BATCH_COUNTS segments."""
    assert n == int(BATCH_OFF[-1])
    return np.random.default_rng(20261024).permutation(n).astype(np.int64)


def weights_table():
    """Rows (customers, adopters, batt_kw_cum_last_year, batt_kw, added) for
    k_export_weights: rint ties of n_adopt and of cum / kw, batt_kw zero,
    negative and below 1e-9, both clamps, customers < adopters and one NaN
    customer count.  No NaN in adopters or batt_kw (the reference raises)."""
    n_adopt = [0.0, 0.5, 1.5, 2.5, 3.49999, 1e6 + 0.5]
    below = lambda x: math.nextafter(x, 0.0)
    kw_cum = [(0.0, 0.0),                    # quotient 0
              (0.0, 4e-3),                   # batt_kw == 0: cum / 1e-9 = 4e6
              (-3.0, 5.0),                   # batt_kw < 0 -> eps
              (-3.0, -2.0),                  # negative quotient clamps to 0
              (1e-12, 2.5e-9),               # batt_kw < 1e-9 -> eps
              (0.25, 0.0), (0.25, 0.625), (0.25, 0.875), (0.25, 0.25 * below(2.5)),
              (8.0, 20.0), (8.0, 28.0), (8.0, 8.0 * below(4.5))]
    assert 0.625 / 0.25 == 2.5 and 0.875 / 0.25 == 3.5 and 20.0 / 8.0 == 2.5 and 28.0 / 8.0 == 3.5
    assert (0.25 * below(2.5)) / 0.25 < 2.5 and (8.0 * below(4.5)) / 8.0 < 4.5
    rows = []
    for a in n_adopt:
        for kw, cum in kw_cum:
            for added in (0, 3, -10):
                i = len(rows)
                cust = a * 0.5 - 1.0 if i % 5 == 3 else a + 100.0 + i      # customers < adopters
                rows.append((cust, a, cum, kw, added))
    rows[7] = (float("nan"),) + rows[7][1:]
    return rows


def weights_columns(n: int):
    """The table cycled to n rows: (customers, adopters, cum, kw) float64 and
    added int64."""
    t = weights_table()
    r = [t[i % len(t)] for i in range(n)]
    cols = [np.array([x[j] for x in r], dtype=np.float64) for j in range(4)]
    return (*cols, np.array([x[4] for x in r], dtype=np.int64))
