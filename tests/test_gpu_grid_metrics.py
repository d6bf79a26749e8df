"""Grid-exchange digest on the GPU: dgen_plane_digest against the numpy
definition (tests/test_grid_metrics.digest_ref) bit for bit -- the arithmetic
is fully specified (fp64, hour order, first hour wins), so no tolerance -- and
its way up through Engine.plane_digest, dgen_amd.grid_metrics and the drop-in
switch size_frame / size_chunk(grid_metrics=True)."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch      # at module level, like the other GPU test modules: in the process before libdgen_hip.so loads

from dgen_amd import _lib
from dgen_amd import financial_functions as ff
from dgen_amd import grid_metrics as gm
from dgen_amd.engine import outputs_to_host, tile_hourly
from tests import helpers
from tests.test_grid_metrics import annual_ref, digest_ref

pytestmark = pytest.mark.gpu

NH = _lib.NH


def _same(dev, ref, what=""):
    """Every member of a device digest equals the reference's, bit for bit."""
    for k, r in ref.items():
        a = dev[k].cpu().numpy()
        assert a.dtype == r.dtype and a.shape == r.shape, (what, k, a.dtype, a.shape)
        assert np.array_equal(a, r), (what, k, np.argwhere(a != r)[:4].tolist())
        if a.dtype == np.float64:      # array_equal holds 0.0 == -0.0: the zeros are positive too
            assert np.array_equal(np.signbit(a), np.signbit(r)), (what, k)


def _synthetic(n, dtype):
    """[8760, n] plane of 5 x N(0, 1) with the crafted columns written over
    columns 0.. while a random column is left (n = 1 keeps its random one)."""
    rng = np.random.default_rng(100 + n)
    p = (rng.standard_normal((NH, n)) * 5.0).astype(dtype)
    crafts = []

    def craft(f):
        crafts.append(f)
        return f

    @craft
    def zeros(c):
        c[:] = 0.0

    @craft
    def negative(c):
        c[:] = -np.abs(c) - 1.0

    @craft
    def ties(c):
        c[100] = c[300] = 99.0            # one month, two hours: the first wins
        c[1500] = c[1600] = -99.0

    @craft
    def month_edges(c):
        c[743], c[744] = 50.0, 60.0       # January's last hour, February's first
        c[8015], c[8016] = 70.0, 80.0     # November's last, December's first
        c[8759] = 90.0                    # the year's last hour (the last quad's last element)
        c[742], c[745], c[8014], c[8017], c[8758] = -50.0, -60.0, -70.0, -80.0, -90.0

    @craft
    def one_nan(c):
        c[5000] = np.nan

    @craft
    def signed_zeros(c):
        c[0::2] = 0.0
        c[1::2] = -0.0

    for j, f in enumerate(crafts):
        if j < n - 1:
            f(p[:, j])
    return p


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_synthetic_planes_match_the_definition(engine, n, dtype):
    p = _synthetic(n, dtype)
    ref = digest_ref(p)
    if n >= 7:
        assert not ref["import_kwh"][:, 0].any() and (ref["peak_export_hour"][:, 0] == -1).all()      # zeros
        assert not ref["import_kwh"][:, 1].any() and (ref["peak_export_hour"][:, 1] >= 0).all()       # negative
        assert ref["peak_import_hour"][0, 2] == 100 and ref["peak_export_hour"][2, 2] == 1500         # ties
        assert ref["peak_import_hour"][[0, 1, 10, 11], 3].tolist() == [743, 744, 8015, 8759]          # edges
        assert ref["peak_export_hour"][[0, 1, 10, 11], 3].tolist() == [742, 745, 8014, 8758]
        assert not any(np.isnan(v[:, 4]).any() for v in ref.values())                                 # NaN hour
        assert not any(v[:, 5].any() for k, v in ref.items() if k in _lib.DIGEST_F64)                 # +-0.0
    t = tile_hourly(torch.from_numpy(p).to(engine.dev))
    assert t.shape == (NH // 4, n, 4)
    d = engine.plane_digest(t)
    torch.cuda.synchronize(engine.dev)
    assert sorted(d) == sorted(_lib.DIGEST_FIELDS)
    _same(d, ref, f"n={n} {np.dtype(dtype).name}")


def test_null_members_are_not_written(engine):
    n = 130
    p = _synthetic(n, np.float32)
    ref = digest_ref(p)
    t = tile_hourly(torch.from_numpy(p).to(engine.dev))
    bufs = {k: torch.full((12, n), -7.0, dtype=torch.float64, device=engine.dev) for k in _lib.DIGEST_F64}
    bufs.update({k: torch.full((12, n), -7, dtype=torch.int32, device=engine.dev) for k in _lib.DIGEST_I32})
    co = _lib.DigestOut(import_kwh=bufs["import_kwh"].data_ptr(), peak_export_hour=bufs["peak_export_hour"].data_ptr())
    rc = engine.lib.dgen_plane_digest(engine.ctx, t.data_ptr(), 0, n, ctypes.byref(co), engine.stream_handle())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(engine.dev)
    for k in _lib.DIGEST_FIELDS:
        a = bufs[k].cpu().numpy()
        if k in ("import_kwh", "peak_export_hour"):
            assert np.array_equal(a, ref[k]), k
        else:
            assert (a == -7).all(), k
    # the engine's form of the same call
    d = engine.plane_digest(t, want=("import_kwh", "peak_export_hour"))
    assert sorted(d) == ["import_kwh", "peak_export_hour"]
    _same(d, {k: ref[k] for k in d})


def test_arguments(engine):
    t = torch.zeros((NH // 4, 2, 4), dtype=torch.float32, device=engine.dev)
    o = torch.zeros((12, 2), dtype=torch.float64, device=engine.dev)
    co = _lib.DigestOut(import_kwh=o.data_ptr())
    L, st = engine.lib, engine.stream_handle()
    assert L.dgen_plane_digest(engine.ctx, t.data_ptr(), 0, 0, ctypes.byref(co), st) == 0        # n = 0: no launch
    assert L.dgen_plane_digest(engine.ctx, None, 0, 2, ctypes.byref(co), st) == -1               # DGEN_E_ARG
    assert _lib.last_error() != ""
    assert L.dgen_plane_digest(engine.ctx, t.data_ptr(), 0, -1, ctypes.byref(co), st) == -1
    assert L.dgen_plane_digest(engine.ctx, t.data_ptr(), 0, 2, None, st) == -1
    torch.cuda.synchronize(engine.dev)
    assert not o.any().item()
    # Engine.plane_digest takes the tiles alloc_outputs makes and nothing else
    with pytest.raises(ValueError):
        engine.plane_digest(torch.zeros((NH, 2), dtype=torch.float32, device=engine.dev))
    with pytest.raises(ValueError):
        engine.plane_digest(torch.zeros((NH // 4, 4, 2), dtype=torch.float32, device=engine.dev).permute(0, 2, 1))
    with pytest.raises(TypeError):
        engine.plane_digest(torch.zeros((NH // 4, 2, 4), dtype=torch.int32, device=engine.dev))
    with pytest.raises(ValueError):
        engine.plane_digest(t, want=("import_mwh",))
    e = engine.plane_digest(torch.zeros((NH // 4, 0, 4), dtype=torch.float64, device=engine.dev))
    assert all(v.shape == (12, 0) for v in e.values())


@pytest.fixture(scope="module")
def golden(engine):
    """The golden population (21 agents) sized once with hourly planes: the
    device outputs, the host planes and their reference digests."""
    b, cols, shapes, cfs, ws = helpers.golden_population()
    engine.load_profiles(shapes, cfs, ws)
    engine.set_tariffs(b.tariffs.array())
    engine.set_switches(b.switches.array())
    batch = engine.upload_agents(cols)
    out = engine.alloc_outputs(batch.n, hourly=True)
    engine.size(batch, out)
    torch.cuda.synchronize(engine.dev)
    host = outputs_to_host(out)
    assert (host["status"] == 0).all()
    ref = {name: digest_ref(host[name].T) for name in _lib.OUTPUT_HOURLY}
    meta, _ = helpers.golden_agents()
    states = [a["inputs"]["state_abbr"] for a in meta["agents"]]
    return {"n": batch.n, "out": out, "ref": ref, "states": states}


def test_golden_population_end_to_end(engine, golden):
    assert golden["n"] == 21
    d1 = gm.digest_outputs(engine, golden["out"])
    d2 = gm.digest_outputs(engine, golden["out"])
    torch.cuda.synchronize(engine.dev)
    assert sorted(d1) == sorted(_lib.OUTPUT_HOURLY)
    for name in _lib.OUTPUT_HOURLY:
        _same(d1[name], golden["ref"][name], name)
        for k in _lib.DIGEST_FIELDS:                    # run-to-run identical
            assert torch.equal(d1[name][k], d2[name][k]), (name, k)
    base = d1["baseline"]
    assert not base["export_kwh"].any().item() and not base["peak_export_kw"].any().item()
    assert (base["peak_export_hour"] == -1).all().item()
    assert (base["import_kwh"] > 0).all().item()
    # the annual reduction, on the device
    for name in _lib.OUTPUT_HOURLY:
        a, r = gm.annual(d1[name]), annual_ref(golden["ref"][name])
        for k in _lib.DIGEST_FIELDS:
            assert np.array_equal(a[k].cpu().numpy().astype(r[k].dtype), r[k]), (name, k)


def test_state_monthly_under_the_storage_mix(engine, golden):
    from dgen_amd import attachment as ga
    from dgen_amd.dist import group_order
    n = golden["n"]
    perm, seg_off, keys = group_order(golden["states"])
    assert len(keys) >= 2 and seg_off[-1] == n
    rng = np.random.default_rng(7)
    w = ga.export_weights(engine, rng.uniform(10, 400, n), rng.uniform(0, 20, n), rng.uniform(0, 30, n),
                          rng.uniform(0, 10, n), rng.integers(0, 3, n))
    d = gm.digest_outputs(engine, golden["out"])
    got = gm.state_monthly(engine, d, w, perm, seg_off).cpu().numpy()
    assert got.shape == (len(keys), 12, 2)
    wp, wb, wn = (x.cpu().numpy() for x in w)
    ref = golden["ref"]
    want = np.zeros_like(got)
    for q, k in enumerate(("import_kwh", "export_kwh")):
        mix = ref["net_pvonly"][k] * wp + ref["net_with_batt"][k] * wb + ref["baseline"][k] * wn     # [12, n]
        for s in range(len(keys)):
            want[s, :, q] = mix[:, perm[seg_off[s]:seg_off[s + 1]]].sum(axis=1) / 1000.0
    assert want[:, :, 0].min() > 0
    # the project's tolerance for fp64 segment sums (tests/test_gpu_aggregate.py)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9), np.abs(got - want).max()


def _cells(frame, col):
    return np.stack([np.asarray(c, dtype=np.float64) for c in frame[col]])


def test_drop_in_switch():
    rows, store, table = helpers.golden_rows()
    df = pd.DataFrame(rows)
    ff._worker_conn = store
    arr, o = ff.size_frame(df, store, table, hourly="array", grid_metrics=True)
    assert all(c in arr.columns for c in gm.COLUMNS)
    planes = {"baseline": "baseline_net_hourly", "pvonly": "adopter_net_hourly_pvonly",
              "with_batt": "adopter_net_hourly_with_batt"}
    for case, col in planes.items():
        a = annual_ref(digest_ref(_cells(arr, col).T))
        for stem, member in gm.COLUMN_STEMS:
            got = arr[f"{stem}_{case}"].to_numpy()
            assert got.dtype == (np.int64 if member.endswith("hour") else np.float64), (stem, case)
            assert np.array_equal(got, a[member]), (stem, case)
    assert (arr["grid_export_kwh_baseline"] == 0).all() and (arr["peak_export_hour_baseline"] == -1).all()
    assert (arr["grid_import_kwh_pvonly"] <= arr["grid_import_kwh_baseline"]).all()

    # hourly="none": the planes are digested and released on the device, never downloaded
    non, o_non = ff.size_frame(df, store, table, hourly="none", grid_metrics=True)
    assert all(o_non[name] is None for name in _lib.OUTPUT_HOURLY)
    assert "baseline_net_hourly" not in non.columns
    # three sub-batches of 7 rows through size_chunk: the columns survive its drop list
    tm = {}
    sub, _ = ff.size_chunk(df, None, table, "simple", hourly="none", timing=tm, max_rows=7, grid_metrics=True)
    assert tm["sub_batches"] == 3
    for c in gm.COLUMNS:
        assert np.array_equal(non[c].to_numpy(), arr[c].to_numpy()), c
        assert np.array_equal(sub[c].to_numpy(), arr[c].to_numpy()), c
        assert sub[c].dtype == arr[c].dtype, c

    # the switch off: exactly the columns (and order) the frame has with it on, less the 18
    off, o_off = ff.size_frame(df, store, table, hourly="array")
    assert not any(c in off.columns for c in gm.COLUMNS) and not any(c in o_off for c in gm.COLUMNS)
    assert list(off.columns) == [c for c in arr.columns if c not in gm.COLUMNS]
    assert list(arr.columns)[-18:] == list(gm.COLUMNS)
    for k in ("system_kw", "npv", "batt_kwh"):
        assert np.array_equal(off[k].to_numpy(), arr[k].to_numpy()), k
