"""Per-agent grid-exchange metrics from the hourly planes, on the device.

The sizing kernels leave three 8760-hour net-load planes per agent in HBM
(``baseline``, ``net_pvonly``, ``net_with_batt``).  ``Engine.plane_digest``
(dgen_plane_digest) reduces one plane to, per agent and calendar month, the kWh
imported and exported, the peak import and peak export (kW) and the hour of
year of each peak.  This module carries that up:

    digest_outputs(engine, out)     the digests of the three planes of an output dict
    annual(d)                       a digest's twelve months reduced to the year, [n]
    state_monthly(...)              per segment and month import / export MWh under
                                    the storage mix (attachment.export_weights)
    annual_columns(engine, out)     the 18 per-agent columns of the drop-in switch
                                    (financial_functions.size_frame(grid_metrics=True))

Nothing here reads a plane on the host; the reductions beyond the digest kernel
are elementwise tensor operations in a fixed order and Engine.segment_sums.
The reference has no counterpart: it drops the hourly lists before writing
agent_outputs (dgen_model.py:441-458).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib

# case name of the drop-in columns -> the plane it digests
CASES = (("baseline", "baseline"), ("pvonly", "net_pvonly"), ("with_batt", "net_with_batt"))
# drop-in column stem -> digest member, in column order
COLUMN_STEMS = (("grid_import_kwh", "import_kwh"), ("grid_export_kwh", "export_kwh"),
                ("peak_import_kw", "peak_import_kw"), ("peak_import_hour", "peak_import_hour"),
                ("peak_export_kw", "peak_export_kw"), ("peak_export_hour", "peak_export_hour"))
COLUMNS = tuple(f"{stem}_{case}" for case, _ in CASES for stem, _ in COLUMN_STEMS)


def digest_outputs(engine, out: Dict[str, object], want: Sequence[str] = tuple(_lib.DIGEST_FIELDS)):
    """The digests of the three hourly planes of an alloc_outputs(...,
    hourly=True) dict, after Engine.size: {plane name: Engine.plane_digest}."""
    res = {}
    for name in _lib.OUTPUT_HOURLY:
        p = out.get(name)
        if p is None:
            raise ValueError(f"digest_outputs: the outputs hold no {name!r} plane (alloc_outputs(hourly=True))")
        res[name] = engine.plane_digest(p, want)
    return res


def _peak(kw, hour):
    """Max over the months of a [12, n] peak with its hour: a later month wins
    only when strictly larger, so a tie keeps the first month's hour."""
    import torch
    pk, hr = kw[0].clone(), hour[0].clone()
    for m in range(1, kw.shape[0]):
        better = kw[m] > pk
        pk = torch.where(better, kw[m], pk)
        hr = torch.where(better, hour[m], hr)
    return pk, hr


def annual(d: Dict[str, object]) -> Dict[str, object]:
    """A digest's [12, n] months -> [n] annual values (device tensors): import
    and export kWh as the twelve months added in month order
    (((m0 + m1) + m2) + ...), the peaks as the maximum over the months with the
    hour of the first month that reaches it."""
    res = {}
    for k in ("import_kwh", "export_kwh"):
        if k in d:
            s = d[k][0].clone()
            for m in range(1, d[k].shape[0]):
                s = s + d[k][m]
            res[k] = s
    for kw, hour in (("peak_import_kw", "peak_import_hour"), ("peak_export_kw", "peak_export_hour")):
        if kw in d and hour in d:
            res[kw], res[hour] = _peak(d[kw], d[hour])
        elif kw in d:
            res[kw] = d[kw].amax(dim=0)
    return res


def state_monthly(engine, digests: Dict[str, Dict[str, object]], weights, idx, seg_off):
    """Per segment and month, the import and export energy in MWh under the
    storage mix  w_pvo x pvonly + w_batt x with_batt + w_non x baseline
    (weights = attachment.export_weights' (w_pvo, w_batt, w_non), one per plane
    column).  digests: digest_outputs' dict; idx: plane column of each segment
    member (None: the columns themselves), seg_off [S + 1].  Each quantity is
    Engine.segment_sums over the digest's twelve month planes (k = 12): the
    two-plane weighted call, then the baseline's, added.  Returns a [S, 12, 2]
    float64 device tensor ([..., 0] import, [..., 1] export)."""
    import torch
    w_pvo, w_batt, w_non = (engine._to_dev(w, torch.float64) for w in weights)
    so = np.asarray(seg_off, dtype=np.int64)
    if so.ndim != 1 or so.size < 1 or so[0] != 0 or np.any(np.diff(so) < 0):
        raise ValueError("state_monthly: segment offsets must start at 0 and be non-decreasing")
    n = int(digests["baseline"]["import_kwh"].shape[1])
    if any(int(w.numel()) != n for w in (w_pvo, w_batt, w_non)):
        raise ValueError("state_monthly: one weight per plane column")
    ti: Optional[object] = None
    if idx is not None:
        ix = np.asarray(idx, dtype=np.int64)
        if ix.shape != (int(so[-1]),) or (ix.size and (ix.min() < 0 or ix.max() >= n)):
            raise ValueError("state_monthly: idx must name one plane column per segment member")
        ti = engine._to_dev(ix, torch.int64)
    elif int(so[-1]) > n:
        raise ValueError("state_monthly: segments exceed the plane width")
    g = (lambda t: t) if ti is None else (lambda t: t.index_select(t.dim() - 1, ti).contiguous())
    wp, wb, wn = g(w_pvo), g(w_batt), g(w_non)
    parts = []
    for k in ("import_kwh", "export_kwh"):
        mix = engine.segment_sums(g(digests["net_pvonly"][k]), so, w1=wp, v2=g(digests["net_with_batt"][k]), w2=wb)
        parts.append((mix + engine.segment_sums(g(digests["baseline"][k]), so, w1=wn)) / 1000.0)
    return torch.stack(parts, dim=2)


def annual_columns(engine, out: Dict[str, object], inv=None) -> Dict[str, np.ndarray]:
    """The drop-in switch's 18 per-agent columns (COLUMNS) of a sized output
    dict as host arrays: per case the annual import / export kWh, peak import /
    export kW (float64) and their hours of year (int64, -1 = none).  inv: the
    device gather into caller order (outputs_to_host's), None = device order.
    Only these [n] vectors cross to the host."""
    import torch
    res = {}
    for case, plane in CASES:
        p = out.get(plane)
        if p is None:
            raise ValueError(f"annual_columns: the outputs hold no {plane!r} plane")
        a = annual(engine.plane_digest(p))
        for stem, member in COLUMN_STEMS:
            t = a[member] if inv is None else a[member].index_select(0, inv)
            if t.dtype == torch.int32:
                t = t.to(torch.int64)
            res[f"{stem}_{case}"] = t.cpu().numpy()
    return res
