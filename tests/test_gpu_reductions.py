"""The reduction and state-export kernels (k_segment_sums, k_rows_seq_sum,
k_export_weights, k_state_hourly in its four plane forms, k_state_hourly_rows)
at segment and layout edges: empty / 1 / 255 / 256 / 257-member segments, a
last segment that ends before n (the columns behind it are NaN), short and
ragged hour tiles, scattered and repeating idx, NaN weights and values.

Sums are compared with the exact references of tests/reduction_refs.py under
its derived bound (no measured tolerance anywhere); everything the header
promises bit for bit, and every repeat, is compared with array_equal /
torch.equal.  tests/test_reduction_refs.py shows on the CPU that these
comparisons catch a float32 accumulator, a dropped or repeated member, a
missing / 1000 and swapped weights on these very inputs."""
import numpy as np
import pytest
import torch

from dgen_amd import _lib
from dgen_amd import attachment as ga
from dgen_amd.engine import hourly_plane, profile_order, tile_hourly
from dgen_amd.partition import host_seq_sum
from oracle import attach as oa
from tests import reduction_refs as rr

pytestmark = pytest.mark.gpu

E_ARG = -1                                   # DGEN_E_ARG
SENTINEL = -7.25


def _dev(engine, a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(engine.dev)   # the shared inputs are read-only


def _within_bound(got, ref, A, off, what):
    """|got - exact| <= bound(m, A) for every output; empty segments exactly +0."""
    got = np.asarray(got)
    err, tol = np.abs(got - ref), rr.seg_bound(off, A)
    bad = np.argwhere(~(err <= tol))                      # a NaN output fails too
    worst = float(np.max(err[tol > 0] / tol[tol > 0]))
    print(f"{what}: max |err| / bound = {worst:.3f}")
    assert bad.size == 0, (what, bad[:5].tolist(), err[tuple(bad[0])], tol[tuple(bad[0])])
    empty = np.diff(np.asarray(off)) == 0
    assert not got[empty].any() and not np.signbit(got[empty]).any(), what


# ---------------------------------------------------------------- segment_sums
@pytest.mark.parametrize("form", rr.SEGMENT_FORMS)
@pytest.mark.parametrize("k", [1, rr.K_MAX])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_segment_sums_within_bound_and_repeatable(engine, dtype, k, form):
    v1, w1, v2, w2 = rr.segment_case(dtype, form, k)
    assert v1.shape == (k, rr.N_COLS) and np.isnan(v1[:, rr.N_MEMBERS:]).all()
    d = lambda a: None if a is None else _dev(engine, a)
    run = lambda a, b: engine.segment_sums(a, rr.SEG_OFF, w1=w1, v2=b, w2=w2)
    got = run(d(v1), d(v2))
    assert got.shape == (len(rr.SEG_COUNTS), k) and got.dtype == torch.float64
    ref, A = rr.segment_reference(dtype, form)
    _within_bound(got.cpu().numpy(), ref[:, :k], A[:, :k], rr.SEG_OFF, f"segment_sums {dtype} k={k} {form}")
    assert torch.equal(run(d(v1), d(v2)), got)
    if dtype == "f32":             # the same values widened: the same bits
        wide = run(d(v1.astype(np.float64)), d(None if v2 is None else v2.astype(np.float64)))
        assert torch.equal(wide, got)


# ---------------------------------------------------------------- rows_seq_sum
@pytest.mark.parametrize("k", [1, 255, 256, 257])
def test_rows_seq_sum_is_the_sequential_order_bit_for_bit(engine, k):
    rows = np.array(rr.rows_inputs()[:, :k], copy=True, order="C")
    got = engine.rows_seq_sum(_dev(engine, rows), rr.ROW_OFF)
    torch.cuda.synchronize(engine.dev)
    ref = host_seq_sum(torch.from_numpy(rows), rr.ROW_OFF)
    assert got.shape == (len(rr.ROW_COUNTS), k)
    assert torch.equal(got.cpu(), ref)
    empty = np.array(rr.ROW_COUNTS) == 0
    assert not got.cpu().numpy()[empty].any()


# ---------------------------------------------------------------- state_hourly
def _hourly_args(nh, kind, w=None, planes=None):
    """Host (planes [nh, N_COLS] float32-valued, weights) of a case, NaN in
    every column its members do not read."""
    p0, w0 = rr.hourly_inputs()
    planes = [p[:nh] for p in (p0 if planes is None else planes)]
    idx = rr.hourly_idx(kind)
    return rr.mask_unused(planes, idx), rr.mask_unused(w0 if w is None else w, idx), idx


def _run_hourly(engine, layout, nh, kind, w=None, planes=None):
    planes, w, idx = _hourly_args(nh, kind, w, planes)
    if layout == "plain":
        dp = [_dev(engine, p.astype(np.float64)) for p in planes]
    else:
        dt = np.float32 if layout == "f32_tiles" else np.float64
        dp = [tile_hourly(_dev(engine, p.astype(dt))) for p in planes]
    got = ga.state_hourly(engine, dp, [_dev(engine, x) for x in w], idx, rr.SEG_OFF)
    assert got.shape == (len(rr.SEG_COUNTS), nh) and got.dtype == torch.float64
    return got.cpu().numpy()


HOURLY_CASES = [("plain", nh) for nh in (1, 5, 31, 32, 33, 56)] + \
               [(lay, nh) for lay in ("f32_tiles", "f64_tiles") for nh in (4, 28, 32, 36, 56)]


@pytest.mark.parametrize("kind", ["none", "scatter"])
@pytest.mark.parametrize("layout,nh", HOURLY_CASES)
def test_state_hourly_within_bound(engine, layout, nh, kind):
    got = _run_hourly(engine, layout, nh, kind)
    ref, A = rr.hourly_reference(kind)
    _within_bound(got, ref[:, :nh], A[:, :nh], rr.SEG_OFF, f"state_hourly {layout} nh={nh} idx={kind}")


@pytest.mark.parametrize("layout", ["plain", "f32_tiles", "f64_tiles"])
def test_state_hourly_repeating_idx(engine, layout):
    got = _run_hourly(engine, layout, 8, "repeat")
    ref, A = rr.hourly_reference("repeat", 8)
    _within_bound(got, ref, A, rr.SEG_OFF, f"state_hourly {layout} repeating idx")


@pytest.mark.parametrize("kind", ["none", "scatter"])
def test_state_hourly_forms_bit_identical(engine, kind):
    """The same float32-valued planes as f32 tiles, f64 tiles and plain f64
    [nh, n] give the same bits (two hour tiles, the second of 24 hours)."""
    a = _run_hourly(engine, "f32_tiles", rr.NH_MAX, kind)
    b = _run_hourly(engine, "f64_tiles", rr.NH_MAX, kind)
    c = _run_hourly(engine, "plain", rr.NH_MAX, kind)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(_run_hourly(engine, "f32_tiles", rr.NH_MAX, kind), a)       # and again


@pytest.mark.parametrize("layout", ["plain", "f32_tiles"])
def test_state_hourly_identity_idx_is_no_idx(engine, layout):
    assert np.array_equal(_run_hourly(engine, layout, rr.NH_MAX, "identity"),
                          _run_hourly(engine, layout, rr.NH_MAX, "none"))


@pytest.mark.parametrize("layout", ["plain", "f32_tiles", "f64_tiles"])
def test_state_hourly_nan_stays_in_its_segment(engine, layout):
    """A NaN weight poisons every hour of its own segment's row and nothing
    else; a NaN plane value only its (segment, hour)."""
    nh, kind, seg = rr.NH_MAX, "scatter", 8
    assert rr.SEG_COUNTS[seg] == 257
    col = int(rr.hourly_idx(kind)[rr.SEG_OFF[seg] + 256])         # the member of the thread's second round
    clean = _run_hourly(engine, layout, nh, kind)
    assert np.isfinite(clean).all()
    others = np.arange(len(rr.SEG_COUNTS)) != seg
    w = [np.array(x, copy=True) for x in rr.hourly_inputs()[1]]
    w[2][col] = np.nan
    got = _run_hourly(engine, layout, nh, kind, w=w)
    assert np.isnan(got[seg]).all()
    assert np.array_equal(got[others], clean[others])
    planes = [np.array(p, copy=True) for p in rr.hourly_inputs()[0]]
    hour = 40                                                       # in the second, 24-hour tile
    planes[1][hour, col] = np.nan
    got = _run_hourly(engine, layout, nh, kind, planes=planes)
    hit = np.zeros_like(clean, dtype=bool)
    hit[seg, hour] = True
    assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])


# ------------------------------------------------- combined plane and rows form
def _sized_batch(engine, n=700, seed=20261025):
    from dgen_amd.synth import make_population
    from dgen_amd.year_loop import YearLoop
    pop = make_population("national_mixed", n, seed=seed, n_res_shapes=64, n_com_shapes=32, n_cf=32,
                          n_counties=16, n_tariffs=48)
    engine.load_profiles(pop.shapes, pop.cfs, pop.wholesale)
    engine.set_tariffs(pop.tariffs)
    engine.set_switches(pop.switches)
    # the rows form's precondition (daily plan, no loss model, no demand machinery)
    assert YearLoop._pick_export(engine, n, True, None, "with_batt") == "with_batt"
    batch = engine.upload_agents(pop.cols, order=profile_order(pop.cols))
    out = engine.alloc_outputs(batch.n, hourly=True)
    engine.size(batch, out)
    torch.cuda.synchronize(engine.dev)
    return batch, out


def test_combined_plane_and_rows_form_at_segment_edges(engine):
    """Segments of 0 / 1 / 255 / 257 / 0 / 187 agents through a scattered idx:
    the combined plane and the rows form give the three-plane rows bit for
    bit, and those are within the bound of the exact sums of the planes."""
    batch, out = _sized_batch(engine)
    n = batch.n
    so, idx = rr.BATCH_OFF, rr.batch_idx(n)
    rng = np.random.default_rng(20261026)
    w_host = [rr._signed_mags(rng, n, -1.0, 1.0) for _ in range(3)]
    w = tuple(_dev(engine, x) for x in w_host)
    planes = (out["baseline"], out["net_pvonly"], out["net_with_batt"])
    three = ga.state_hourly(engine, planes, w, idx, so)
    assert three.shape == (len(rr.BATCH_COUNTS), _lib.NH) and bool(torch.isfinite(three).all())

    plane = torch.empty((_lib.NH // 4, n, 4), dtype=torch.float64, device=engine.dev)
    rest = {k: v for k, v in out.items() if k not in _lib.OUTPUT_HOURLY}
    assert engine.export_plane(batch, engine.c_outputs(rest), w, plane)
    assert torch.equal(ga.state_hourly_combined(engine, plane, idx, so), three)

    rows = ga.state_hourly_rows(engine, batch, engine.c_outputs(out), out["net_with_batt"], w, idx, so)
    assert torch.equal(rows, three)
    assert torch.equal(ga.state_hourly_rows(engine, batch, engine.c_outputs(out), out["net_with_batt"], w,
                                            _dev(engine, idx), so), three)

    # exact sums of the host copies of the planes: the first hour tile, the
    # last (24-hour) one and every 97th hour between (the Python-integer
    # reference costs 2100 products per hour)
    hours = np.unique(np.concatenate([np.arange(32), np.arange(32, _lib.NH - 24, 97),
                                      np.arange(_lib.NH - 24, _lib.NH)]))
    host = [hourly_plane(p).cpu().numpy()[hours] for p in planes]
    assert all(p.dtype == np.float32 and np.isfinite(p).all() for p in host)
    ref, A = rr.exact_state_hourly(*host, w_host, idx, so)
    _within_bound(three.cpu().numpy()[:, hours], ref, A, so, "state_hourly over the sized f32 planes")
    assert (A[np.diff(so) > 0] > 0).all()


# --------------------------------------------------------------- export_weights
@pytest.mark.parametrize("n", [1, 255, 257])
def test_export_weights_match_oracle_bit_for_bit(engine, n):
    cust, adopt, cum, kw, added = rr.weights_columns(n)
    got = torch.stack(ga.export_weights(engine, cust, adopt, cum, kw, added)).cpu().numpy()
    ref = oa.weights(cust, adopt, cum, kw, added)
    assert got.shape == ref.shape == (3, n)
    assert np.array_equal(got, ref, equal_nan=True)
    assert not np.signbit(got[~np.isnan(got)]).any()
    if n > 7:
        assert np.array_equal(np.isnan(got[2]), np.isnan(cust)) and np.isfinite(got[:2]).all()


# --------------------------------------------------------------- argument paths
def _hourly_ctypes(engine, layout, nh, n_seg=2, n=8):
    """dgen_state_hourly through ctypes on buffers large enough for any
    reading of the arguments; returns (rc, out)."""
    L = ga._bind(engine.lib)
    cap = ((nh + 3) // 4) * 4 * n
    p = [torch.ones(cap, dtype=torch.float64, device=engine.dev) for _ in range(3)]
    w = [torch.ones(n, dtype=torch.float64, device=engine.dev) for _ in range(3)]
    so = _dev(engine, np.array([0, 3, n], dtype=np.int64))
    out = torch.full((2 * cap,), SENTINEL, dtype=torch.float64, device=engine.dev)
    rc = L.dgen_state_hourly(engine.ctx, p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), layout,
                             w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), None, n, nh, so.data_ptr(),
                             n_seg, out.data_ptr(), engine.stream_handle())
    torch.cuda.synchronize(engine.dev)
    return rc, out


def _untouched(out):
    return bool((out == SENTINEL).all())


def test_state_hourly_rejects_bad_layouts_before_launching(engine):
    rc, out = _hourly_ctypes(engine, 4, 8)
    assert rc == E_ARG and "planes_f32" in _lib.last_error() and _untouched(out)
    rc, out = _hourly_ctypes(engine, -1, 8)
    assert rc == E_ARG and _untouched(out)
    for layout in (1, 2, 3):
        rc, out = _hourly_ctypes(engine, layout, 6)
        assert rc == E_ARG and "% 4" in _lib.last_error() and _untouched(out), layout
    rc, out = _hourly_ctypes(engine, 0, 0)
    assert rc == E_ARG and _untouched(out)
    rc, out = _hourly_ctypes(engine, 0, 6, n_seg=0)                  # nothing to do: OK, nothing written
    assert rc == 0 and _untouched(out)
    rc, out = _hourly_ctypes(engine, 0, 6)                           # the same call with its segments runs
    assert rc == 0 and not _untouched(out)


def test_rows_seq_sum_and_segment_sums_limits_before_launching(engine):
    L, st = engine.lib, engine.stream_handle()
    zeros = lambda m, dt=torch.float64: torch.zeros(m, dtype=dt, device=engine.dev)
    sent = lambda m: torch.full((m,), SENTINEL, dtype=torch.float64, device=engine.dev)
    big = 65536
    so, rows, out = zeros(big + 1, torch.int64), zeros(4), sent(big)
    assert L.dgen_rows_seq_sum(engine.ctx, rows.data_ptr(), 1, so.data_ptr(), big, out.data_ptr(), st) == E_ARG
    assert "dgen_rows_seq_sum" in _lib.last_error()
    assert L.dgen_rows_seq_sum(engine.ctx, rows.data_ptr(), 1, so.data_ptr(), 0, out.data_ptr(), st) == 0
    torch.cuda.synchronize(engine.dev)
    assert _untouched(out)
    v, so2, out2 = zeros(big), _dev(engine, np.array([0, 1], dtype=np.int64)), sent(big)
    args = lambda k, n_seg: (engine.ctx, v.data_ptr(), None, None, None, 0, k, 1, so2.data_ptr(), n_seg,
                             out2.data_ptr(), st)
    assert L.dgen_segment_sums(*args(big, 1)) == E_ARG
    assert "dgen_segment_sums" in _lib.last_error()
    assert L.dgen_segment_sums(*args(0, 1)) == E_ARG
    assert L.dgen_segment_sums(*args(3, 0)) == 0
    torch.cuda.synchronize(engine.dev)
    assert _untouched(out2)
    assert L.dgen_segment_sums(*args(3, 1)) == 0                     # the same call with its segment runs
    torch.cuda.synchronize(engine.dev)
    assert out2[:3].tolist() == [0.0, 0.0, 0.0] and _untouched(out2[3:])


def test_wrappers_refuse_what_the_kernels_would_misread(engine):
    """Weights that are not n float64 values on the device, and mismatched
    segment-sum operands, raise in Python: nothing is launched."""
    nh, n = 8, 16
    f64 = lambda *s: torch.ones(s, dtype=torch.float64, device=engine.dev)
    planes = [f64(nh, n) for _ in range(3)]
    so = np.array([0, 5, n], dtype=np.int64)
    good = [f64(n) for _ in range(3)]
    for bad in (f64(n).float(), f64(n).cpu(), f64(n).to(torch.int64), np.ones(n)):
        for j in range(3):
            w = list(good)
            w[j] = bad
            with pytest.raises(TypeError):
                ga.state_hourly(engine, planes, w, None, so)
            with pytest.raises(TypeError):
                ga.state_hourly_rows(engine, None, None, torch.empty((_lib.NH // 4, n, 4), dtype=torch.float32,
                                                                     device=engine.dev), w, None, so)
    with pytest.raises(ValueError):
        ga.state_hourly(engine, planes, good[:2], None, so)
    with pytest.raises(ValueError):
        ga.state_hourly(engine, planes, [f64(n), f64(n), f64(n + 1)], None, so)
    assert ga.state_hourly(engine, planes, good, None, so).shape == (2, nh)

    v = f64(3, n)
    for kw in (dict(w1=np.ones(n - 1)), dict(w1=np.ones(n + 1)), dict(w1=np.ones((1, n))),
               dict(w1=np.ones(n), v2=v, w2=np.ones(n - 1)), dict(v2=f64(3, n - 1), w2=np.ones(n)),
               dict(v2=f64(2, n), w2=np.ones(n)), dict(v2=v), dict(w1=f64(n + 1))):
        with pytest.raises(ValueError):
            engine.segment_sums(v, so, **kw)
    with pytest.raises(ValueError):
        engine.segment_sums(f64(n), so, v2=f64(n + 1), w2=np.ones(n))
    assert engine.segment_sums(v, so, w1=np.ones(n), v2=v, w2=f64(n)).tolist() == [[10.0] * 3, [22.0] * 3]
