"""Battery size what-if: with-battery economics at caller-given banks.

The reference sizes the battery from two constants (pv_to_batt_ratio = 0.8,
batt_capacity_to_power_ratio = 2.0): the bank is kW* / 0.8 kWh with kW* / 0.8 /
2 kW.  ``Engine.batt_curve`` (dgen_batt_curve) runs the PV+battery forward pass
of a sized batch at any other bank -- dispatch replay, N-year bill, Cashloan --
K points per agent in one launch (the definitions are in include/dgen_hip.h).
This module carries that up:

    ratio_points(system_kw, pv_to_batt, hours)   [K, n] kWh and kW point arrays from ratios
    curve_outputs(engine, batch, out, kwh, kw)   the curve of a sized output dict, caller order
    best_point(curve)                            per agent the valid point of largest NPV
    annual_columns(engine, batch, out, spec)     the per-agent columns of the drop-in switch
                                                 (financial_functions.size_frame(batt_sizing=spec))

dgen_batt_curve covers the tariffs that bill from monthly bins (metering
options 0, 1, 4; tier units 0, 2; no billed demand charge); a point under
another form carries _lib.ST_HOURLY_FORM and NaN, and is never a best point.
net=True (the spec key "net_billing": True) adds dgen_batt_curve_net on the
same buffers: the net-billing tariffs (options 2 and 3, the TS sell rate
included) are computed too.  peak=True (the spec key "peak_billing": True)
adds dgen_batt_curve_peak: tariffs with billed demand charges or kWh/kW tier
units, under every metering option.  After all three what stays flagged is
the agents the sizing call left DGEN_ST_UNIT, malformed demand tables and
list overflow.

All of the above hold the PV size at kW*.  ``Engine.size_with_batt``
(dgen_size_with_batt) instead searches the PV size x on the with-battery
objective, the bank sized from x (x / ratio kWh at hours); net=True (the spec
key "net_billing": True) adds dgen_size_with_batt_net on the same buffers: the
agents whose evaluations reach options 2 and 3 are searched too; peak=True (the
spec key "peak_billing": True) adds dgen_size_with_batt_peak last: the agents
whose evaluations reach billed demand charges or kWh/kW tier units:

    co_size_spec(spec)                           size_frame's pv_batt_sizing spec as (ratio, hours)
    co_size_options(spec)                        its net- and peak-billing settings (Engine.size_with_batt's keywords)
    co_size_summarize(res, npv_ref, status_ref)  the CO_COLUMNS of a search result
    co_size_columns(engine, batch, out, spec)    the per-agent columns of the drop-in switch
                                                 (financial_functions.size_frame(pv_batt_sizing=spec))
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib

REF_PV_TO_BATT = 0.8     # the reference's pv_to_batt_ratio
REF_HOURS = 2.0          # the reference's batt_capacity_to_power_ratio
PREFIX = "batt_opt_"
COLUMNS = tuple(PREFIX + k for k in ("kwh", "kw", "npv", "payback", "point", "npv_gain", "status"))
# status bits that leave a point without a value
INVALID = (_lib.ST_BOUNDS | _lib.ST_TARIFF | _lib.ST_YEARS | _lib.ST_SCRATCH | _lib.ST_UNIT | _lib.ST_DEMAND
           | _lib.ST_HOURLY_FORM)


CO_PREFIX = "pvb_opt_"
CO_COLUMNS = tuple(CO_PREFIX + k for k in ("kw", "kwh", "batt_kw", "npv", "payback", "nfev", "status", "npv_gain"))

# the spec key "dispatch": True of either switch: the 22 batt_diag_ quantities
# (batt_metrics.ANNUAL) of the dispatch replayed at the chosen point
# (Engine.replay_at), batt_opt_diag_* and pvb_opt_diag_*
DIAG_PREFIX = PREFIX + "diag_"
CO_DIAG_PREFIX = CO_PREFIX + "diag_"


def _diag_names(prefix):
    from .batt_metrics import ANNUAL
    return tuple(prefix + k for k in ANNUAL)


def dispatch(spec) -> bool:
    """True when the spec (of either switch) asks for the dispatch at the
    chosen point: a dict with "dispatch": True."""
    return isinstance(spec, dict) and bool(spec.get("dispatch", False))


def columns_of(spec) -> Tuple[str, ...]:
    """The columns size_frame(batt_sizing=spec) adds: COLUMNS, and the 22
    batt_opt_diag_* after them with "dispatch": True."""
    return COLUMNS + (_diag_names(DIAG_PREFIX) if dispatch(spec) else ())


def co_columns_of(spec) -> Tuple[str, ...]:
    """The columns size_frame(pv_batt_sizing=spec) adds: CO_COLUMNS, and the 22
    pvb_opt_diag_* after them with "dispatch": True."""
    return CO_COLUMNS + (_diag_names(CO_DIAG_PREFIX) if dispatch(spec) else ())


def diag_columns(engine, batch, kw, bank_kwh, bank_kw, valid, prefix) -> Dict[str, np.ndarray]:
    """The 22 diag columns of a chosen point as host arrays in caller order:
    batt_metrics.replay_columns of Engine.replay_at at kw / bank_kwh / bank_kw
    ([n] device tensors in the batch's device order).  valid: [n] bool, the
    agents that have a point; the others (and any the replay flags) are
    replayed at kw = 0 without a bank and hold NaN in the float columns and 0
    in the hour counts, as the sibling *_opt_ columns do."""
    import torch
    from . import batt_metrics as bm
    zero = torch.zeros_like(kw)
    d = engine.replay_at(batch, torch.where(valid, kw, zero), torch.where(valid, bank_kwh, zero),
                         torch.where(valid, bank_kw, torch.ones_like(kw)))
    ok = valid & (d["status"] == 0)
    inv = _inverse(engine, batch.perm)
    if inv is not None:
        d = {k: v.index_select(v.dim() - 1, inv) for k, v in d.items()}
        ok = ok.index_select(0, inv)
    cols = bm.replay_columns(d, engine.cfg, prefix)
    okh = ok.cpu().numpy()
    for k, v in cols.items():
        v[~okh] = np.nan if v.dtype.kind == "f" else 0
    return cols


def _xp(t):
    if isinstance(t, np.ndarray):
        return np
    import torch
    return torch


def ratio_points(system_kw, pv_to_batt: Sequence[float] = (REF_PV_TO_BATT,),
                 hours: Sequence[float] = (REF_HOURS,)) -> Tuple[object, object]:
    """The (kwh, kw) point arrays, each [K, n] with K = len(pv_to_batt) x
    len(hours), ratio-major: point k = a x len(hours) + b has
    kwh = system_kw / pv_to_batt[a] and kw = kwh / hours[b] -- the reference's
    own expressions, so (0.8, 2.0) is its bank bit for bit.  system_kw: [n], a
    numpy array or a tensor (the result is of the same kind).  Every ratio and
    duration must be finite and positive."""
    r = [float(v) for v in pv_to_batt]
    h = [float(v) for v in hours]
    if not r or not h or not all(np.isfinite(v) and v > 0.0 for v in r + h):
        raise ValueError(f"ratio_points: ratios and hours must be finite and positive (got {r}, {h})")
    if len(r) * len(h) > _lib.BATT_CURVE_MAX_POINTS:
        raise ValueError(f"ratio_points: {len(r)} x {len(h)} points exceed {_lib.BATT_CURVE_MAX_POINTS}")
    xp = _xp(system_kw)
    kwh, kw = [], []
    for a in r:
        e = system_kw / a
        for b in h:
            kwh.append(e)
            kw.append(e / b)
    return xp.stack(kwh), xp.stack(kw)


def _inverse(engine, perm):
    if perm is None:
        return None
    import torch
    p = np.asarray(perm, np.int64)
    iv = np.empty_like(p)
    iv[p] = np.arange(p.size, dtype=np.int64)
    return engine._to_dev(iv, torch.int64)


def curve_outputs(engine, batch, out, kwh, kw=None, want: Optional[Sequence[str]] = None,
                  net: bool = False, net_cap: Optional[int] = None, peak: bool = False,
                  peak_caps=None) -> Dict[str, object]:
    """Engine.batt_curve of a batch sized (or evaluated) into `out`, with kwh /
    kw given and the members returned in caller order (batch.perm):
    {member: [K, n] device tensor}.  net / net_cap and peak / peak_caps:
    Engine.batt_curve's (the net-billing points, and the demand-charge and
    kWh/kW-tier points, computed too)."""
    import torch
    e = engine._to_dev(kwh, torch.float64)
    p = None if kw is None else engine._to_dev(kw, torch.float64)
    if batch.perm is not None:
        pm = engine._to_dev(np.asarray(batch.perm, np.int64), torch.int64)
        e = e.index_select(e.dim() - 1, pm)
        p = None if p is None else p.index_select(p.dim() - 1, pm)
    d = engine.batt_curve(batch, out, e, p, want, **_net_kw(net, net_cap), **_peak_kw(peak, peak_caps))
    inv = _inverse(engine, batch.perm)
    if inv is None:
        return d
    return {k: v.index_select(1, inv) for k, v in d.items()}


def _net_kw(net, net_cap=None):
    """Engine.batt_curve's keywords; none without net, so that a caller's
    engine sees the call it always saw."""
    if not net:
        return {}
    return {"net": True} if net_cap is None else {"net": True, "net_cap": net_cap}


def _peak_kw(peak, peak_caps=None):
    """Engine.batt_curve's keywords; none without peak, as _net_kw."""
    if not peak:
        return {}
    return {"peak": True} if peak_caps is None else {"peak": True, "peak_caps": peak_caps}


def best_point(curve: Dict[str, object]):
    """Per agent the index of the valid point of largest NPV ([n] int64; numpy
    or torch as the curve is): a point is valid when its status has no INVALID
    bit and its npv is not NaN; the first point wins a tie; -1 where no point
    is valid."""
    npv, st = curve["npv"], curve["status"]
    xp = _xp(npv)
    ok = ((st & INVALID) == 0) & ~xp.isnan(npv)
    K = npv.shape[0]
    best = xp.full_like(npv[0], -np.inf)
    if xp is np:
        idx = np.full(npv.shape[1], -1, np.int64)
    else:
        idx = xp.full((npv.shape[1],), -1, dtype=xp.int64, device=npv.device)
    for k in range(K):
        take = ok[k] & ((idx < 0) | (npv[k] > best))
        best = xp.where(take, npv[k], best)
        idx = xp.where(take, xp.full_like(idx, k), idx)
    return idx


def _pick(xp, v, idx, fill):
    """v[idx[i], i], fill where idx is -1."""
    safe = xp.where(idx < 0, xp.zeros_like(idx), idx)
    if xp is np:
        g = v[safe, np.arange(v.shape[1])]
    else:
        g = v.gather(0, safe.view(1, -1))[0]
    return xp.where(idx < 0, xp.full_like(g, fill), g)


def summarize(curve: Dict[str, object], ref_point: int) -> Dict[str, object]:
    """The COLUMNS of a curve ([n] each; numpy or torch as the curve is), with
    ref_point the index of the reference's point in it:
      batt_opt_point     best_point(curve)
      batt_opt_kwh, _kw  the installed bank and power at it (NaN where -1)
      batt_opt_npv, batt_opt_payback   npv and payback_raw at it
      batt_opt_npv_gain  batt_opt_npv minus the npv at ref_point (NaN where
                         either is missing)
      batt_opt_status    the best point's status; where no point is valid the
                         bitwise or of every point's status"""
    xp = _xp(curve["npv"])
    idx = best_point(curve)
    res = {PREFIX + "kwh": _pick(xp, curve["bank_kwh"], idx, np.nan),
           PREFIX + "kw": _pick(xp, curve["power_kw"], idx, np.nan),
           PREFIX + "npv": _pick(xp, curve["npv"], idx, np.nan),
           PREFIX + "payback": _pick(xp, curve["payback_raw"], idx, np.nan),
           PREFIX + "point": idx}
    res[PREFIX + "npv_gain"] = res[PREFIX + "npv"] - curve["npv"][ref_point]
    st = curve["status"]
    allst = st[0]
    for k in range(1, st.shape[0]):
        allst = allst | st[k]
    res[PREFIX + "status"] = _pick(xp, st, idx, 0) | xp.where(idx < 0, allst, xp.zeros_like(allst))
    return res


def grid(spec) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """size_frame's batt_sizing spec as (pv_to_batt, hours): a dict with either
    key, a (pv_to_batt, hours) pair, or True for the default grid.  The dict's
    "net_billing", "peak_billing" and "dispatch" keys are not part of the grid
    (net_billing(spec), peak_billing(spec), dispatch(spec))."""
    if spec is True:
        return (0.4, 0.8, 1.6), (1.0, 2.0, 4.0)
    if isinstance(spec, dict):
        bad = set(spec) - {"pv_to_batt", "hours", "net_billing", "peak_billing", "dispatch"}
        if bad:
            raise ValueError(f"batt_sizing: unknown keys {sorted(bad)}")
        if not isinstance(spec.get("dispatch", False), (bool, np.bool_)):
            raise ValueError(f"batt_sizing: dispatch must be a bool (got {spec['dispatch']!r})")
        return tuple(spec.get("pv_to_batt", (REF_PV_TO_BATT,))), tuple(spec.get("hours", (REF_HOURS,)))
    r, h = spec
    return tuple(r), tuple(h)


def net_billing(spec) -> bool:
    """True when the spec asks for the net-billing tariffs too: a dict with
    "net_billing": True."""
    return isinstance(spec, dict) and bool(spec.get("net_billing", False))


def peak_billing(spec) -> bool:
    """True when the spec asks for the demand-charge and kWh/kW-tier tariffs
    too: a dict with "peak_billing": True."""
    return isinstance(spec, dict) and bool(spec.get("peak_billing", False))


def annual_columns(engine, batch, out, spec=True) -> Dict[str, np.ndarray]:
    """The drop-in switch's per-agent columns (COLUMNS) of a sized output dict
    as host arrays in caller order: the curve over ratio_points(system_kw,
    *grid(spec)) with the reference's point (0.8, 2.0) appended as the last
    point, reduced by summarize().  float64, except batt_opt_point and
    batt_opt_status (int64).  Only these [n] vectors cross to the host.  With
    "net_billing": True in the spec the net-billing points are computed too
    (dgen_batt_curve_net), with "peak_billing": True the points on tariffs
    with billed demand charges or kWh/kW tier units (dgen_batt_curve_peak).
    With "dispatch": True the 22 batt_opt_diag_* columns follow (columns_of):
    the dispatch replayed at kW* with the best point's desired kWh and kW as
    the curve was handed them (diag_columns)."""
    import torch
    r, h = grid(spec)
    skw = out["system_kw"]
    kwh, kw = ratio_points(skw, r, h)
    rk, rp = ratio_points(skw, (REF_PV_TO_BATT,), (REF_HOURS,))
    kwh, kw = torch.cat([kwh, rk]), torch.cat([kw, rp])
    if kwh.shape[0] > _lib.BATT_CURVE_MAX_POINTS:
        raise ValueError(f"batt_sizing: {kwh.shape[0]} points (the reference's included) exceed "
                         f"{_lib.BATT_CURVE_MAX_POINTS}")
    # an unsized agent's system_kw may be NaN: its points are flagged, not read
    d = engine.batt_curve(batch, out, kwh, kw, ("npv", "payback_raw", "bank_kwh", "power_kw", "status"),
                          **_net_kw(net_billing(spec)), **_peak_kw(peak_billing(spec)))
    s = summarize(d, int(kwh.shape[0]) - 1)
    inv = _inverse(engine, batch.perm)
    res = {}
    for k in COLUMNS:
        t = s[k] if inv is None else s[k].index_select(0, inv)
        if t.dtype == torch.int32:
            t = t.to(torch.int64)
        res[k] = t.cpu().numpy()
    if dispatch(spec):
        idx = s[PREFIX + "point"]
        res.update(diag_columns(engine, batch, skw, _pick(torch, kwh, idx, 0.0), _pick(torch, kw, idx, 1.0),
                                idx >= 0, DIAG_PREFIX))
    return res


PEAK_KEYS = ("peak_billing", "peak_caps", "peak_blocks")


def co_size_spec(spec, peak: bool = False) -> Tuple[float, float]:
    """size_frame's pv_batt_sizing spec as (ratio, hours): True for the
    reference's constants (0.8, 2.0), or a dict with "ratio" and / or "hours";
    both must be finite and positive.  The dict's "net_billing", "net_cap" and
    "net_blocks" keys are not part of the pair (co_size_options(spec)).  The
    keys it admits without `peak` are the ones it always admitted; peak=True
    (what co_size_options and co_size_columns pass) also admits PEAK_KEYS and
    "dispatch", which are not part of the pair either."""
    if spec is True:
        return REF_PV_TO_BATT, REF_HOURS
    if not isinstance(spec, dict):
        raise ValueError(f"pv_batt_sizing: True or a dict with \"ratio\" / \"hours\" (got {spec!r})")
    bad = (set(spec) - {"ratio", "hours", "net_billing", "net_cap", "net_blocks"}
           - set(PEAK_KEYS + ("dispatch",) if peak else ()))
    if bad:
        raise ValueError(f"pv_batt_sizing: unknown keys {sorted(bad)}")
    r, h = float(spec.get("ratio", REF_PV_TO_BATT)), float(spec.get("hours", REF_HOURS))
    if not (np.isfinite(r) and r > 0.0 and np.isfinite(h) and h > 0.0):
        raise ValueError(f"pv_batt_sizing: ratio and hours must be finite and positive (got {r}, {h})")
    return r, h


def co_size_options(spec) -> Dict[str, object]:
    """Engine.size_with_batt's net keywords of a pv_batt_sizing spec: none for
    True or a dict without "net_billing": True (the engine then sees the call
    it always saw), else {"net": True} with "net_cap" (1 .. _lib.NB_CAPM mixed
    hours a month) and "net_blocks" (>= 1 persistent blocks) where the spec
    names them.  "net_billing" must be a bool, the other two ints (None: the
    default); they are checked even when net billing is off.  Likewise
    "peak_billing": True gives {"peak": True} with "peak_caps" (a pair
    (cap_mixed, cap_kept) of ints, 1 .. _lib.NB_CAPM and 1 ..
    _lib.BATT_PEAK_CAPK_MAX, None in either place: the default) and
    "peak_blocks" (>= 1); neither key implies the other.  "dispatch" must be
    a bool and is no keyword of the search (dispatch(spec))."""
    co_size_spec(spec, peak=True)
    if spec is True:
        return {}
    if not isinstance(spec.get("dispatch", False), (bool, np.bool_)):
        raise ValueError(f"pv_batt_sizing: dispatch must be a bool (got {spec['dispatch']!r})")
    net = spec.get("net_billing", False)
    if not isinstance(net, (bool, np.bool_)):
        raise ValueError(f"pv_batt_sizing: net_billing must be a bool (got {net!r})")
    kw = {}
    for key, name, top in (("net_cap", "net_cap", _lib.NB_CAPM), ("net_blocks", "net_blocks", None)):
        v = spec.get(key)
        if v is None:
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"pv_batt_sizing: {key} must be an int (got {v!r})")
        if v < 1 or (top is not None and v > top):
            raise ValueError(f"pv_batt_sizing: {key} must be " + (f"1 .. {top}" if top else ">= 1") + f" (got {v})")
        kw[name] = int(v)
    peak = spec.get("peak_billing", False)
    if not isinstance(peak, (bool, np.bool_)):
        raise ValueError(f"pv_batt_sizing: peak_billing must be a bool (got {peak!r})")
    pk = {}
    caps = spec.get("peak_caps")
    if caps is not None:
        if not isinstance(caps, (tuple, list)) or len(caps) != 2:
            raise ValueError(f"pv_batt_sizing: peak_caps must be a pair (cap_mixed, cap_kept) (got {caps!r})")
        for v, what, top in zip(caps, ("cap_mixed", "cap_kept"), (_lib.NB_CAPM, _lib.BATT_PEAK_CAPK_MAX)):
            if v is None:
                continue
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"pv_batt_sizing: peak_caps' {what} must be an int (got {v!r})")
            if v < 1 or v > top:
                raise ValueError(f"pv_batt_sizing: peak_caps' {what} must be 1 .. {top} (got {v})")
        pk["peak_caps"] = tuple(None if v is None else int(v) for v in caps)
    v = spec.get("peak_blocks")
    if v is not None:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"pv_batt_sizing: peak_blocks must be an int (got {v!r})")
        if v < 1:
            raise ValueError(f"pv_batt_sizing: peak_blocks must be >= 1 (got {v})")
        pk["peak_blocks"] = int(v)
    res = {"net": True, **kw} if net else {}
    if peak:
        res.update({"peak": True, **pk})
    return res


def co_size_summarize(res: Dict[str, object], npv_ref, status_ref) -> Dict[str, object]:
    """The CO_COLUMNS of an Engine.size_with_batt result ([n] each; numpy or
    torch as the result is).  npv_ref, status_ref: npv_pv_batt and status of
    the sizing call, in the same order.
      pvb_opt_kw, _kwh, _batt_kw   system_kw and the installed bank and power at it
      pvb_opt_npv, pvb_opt_payback npv and payback_raw at it
      pvb_opt_nfev, pvb_opt_status the search's evaluations and status
      pvb_opt_npv_gain             pvb_opt_npv - npv_ref; NaN where the search's
                                   status has an INVALID bit or its npv is NaN,
                                   or status_ref has an INVALID bit or npv_ref
                                   is NaN
    An agent whose search is invalid holds NaN in every float column (the
    device wrote them)."""
    xp = _xp(res["npv"])
    npv = res["npv"]
    ok = (((res["status"] & INVALID) == 0) & ~xp.isnan(npv)
          & ((status_ref & INVALID) == 0) & ~xp.isnan(npv_ref))
    gain = xp.where(ok, npv - npv_ref, xp.full_like(npv, np.nan))
    return {CO_PREFIX + "kw": res["system_kw"], CO_PREFIX + "kwh": res["bank_kwh"],
            CO_PREFIX + "batt_kw": res["power_kw"], CO_PREFIX + "npv": npv,
            CO_PREFIX + "payback": res["payback_raw"], CO_PREFIX + "nfev": res["nfev"],
            CO_PREFIX + "status": res["status"], CO_PREFIX + "npv_gain": gain}


def co_size_columns(engine, batch, out, spec=True) -> Dict[str, np.ndarray]:
    """The drop-in switch's per-agent columns (CO_COLUMNS) as host arrays in
    caller order: Engine.size_with_batt of the batch over the sizing call's
    bracket at co_size_spec(spec, peak=True), reduced by co_size_summarize() against the
    npv_pv_batt and status of the sized output dict `out`.  float64, except
    pvb_opt_nfev and pvb_opt_status (int64).  Only these [n] vectors cross to
    the host.  With "net_billing": True in the spec the agents on net-billing
    tariffs are searched too (dgen_size_with_batt_net; co_size_options(spec)), with
    "peak_billing": True those on billed demand charges and kWh/kW tier units
    (dgen_size_with_batt_peak).  With "dispatch": True the 22
    pvb_opt_diag_* columns follow (co_columns_of): the dispatch replayed at
    pvb_opt_kw with the bank the search sized from it, x / ratio kWh at
    (x / ratio) / hours kW (diag_columns)."""
    import torch
    r, h = co_size_spec(spec, peak=True)
    d = engine.size_with_batt(batch, r, h, want=("system_kw", "bank_kwh", "power_kw", "npv", "payback_raw", "nfev",
                                                 "status"), **co_size_options(spec))
    s = co_size_summarize(d, out["npv_pv_batt"], out["status"])
    inv = _inverse(engine, batch.perm)
    res = {}
    for k in CO_COLUMNS:
        t = s[k] if inv is None else s[k].index_select(0, inv)
        if t.dtype == torch.int32:
            t = t.to(torch.int64)
        res[k] = t.cpu().numpy()
    if dispatch(spec):
        x = d["system_kw"]
        e = x / r
        ok = ((d["status"] & INVALID) == 0) & torch.isfinite(x)
        res.update(diag_columns(engine, batch, x, e, e / h, ok, CO_DIAG_PREFIX))
    return res
