"""Per-agent battery dispatch metrics, on the device.

The hourly scan keeps the battery's state of charge in registers and drops it;
``Engine.batt_summary`` (dgen_batt_summary) replays the dispatch of a sized
batch and reduces it, per agent and calendar month, to the PV surplus and where
it went (battery, grid), what served the load (PV, battery, grid), the same
surplus sums over a midday window, the SOC range and the hours the bank sat
full, empty or power-limited (the definitions are in include/dgen_hip.h).  This
module carries that up:

    summary_outputs(engine, batch, out)   the summary of a sized output dict, caller order
    annual(d, bank_kwh, cfg)              the twelve months reduced to the year, [n],
                                          plus three ratios
    state_monthly(...)                    per segment and month MWh of the kWh members
    annual_columns(engine, batch, out)    the per-agent columns of the drop-in switch
                                          (financial_functions.size_frame(batt_metrics=True))
    replay_outputs(engine, batch, kw, bank_kwh, bank_kw)
                                          the summary (and planes) at a caller-given PV size
                                          and bank (Engine.replay_at), caller order
    replay_columns(d, cfg, prefix)        annual_columns of a replay_outputs result

Nothing here reads an hourly value on the host: no plane is needed at all, so
the metrics are the same bits in every hourly mode.  The reference's
counterpart is batt_dispatch_helpers.dispatch_export_diags, one agent at a time
from PySAM's hourly arrays.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib

KWH_MEMBERS = tuple(k for k in _lib.BATT_SUMMARY_F64 if k.endswith("_kwh"))
SOC_MEMBERS = ("soc_min", "soc_max", "soc_end")
COUNT_MEMBERS = tuple(_lib.BATT_SUMMARY_I32)
RATIOS = ("capture_mid_frac", "equiv_full_cycles", "self_sufficiency_frac")
# annual()'s members, in the drop-in switch's column order
ANNUAL = KWH_MEMBERS + SOC_MEMBERS + COUNT_MEMBERS + RATIOS
PREFIX = "batt_diag_"
COLUMNS = tuple(PREFIX + k for k in ANNUAL)


def _xp(t):
    """numpy for host arrays, torch for tensors: annual() runs on either."""
    if isinstance(t, np.ndarray):
        return np
    import torch
    return torch


def _inverse(engine, perm):
    """The device gather into caller order of a batch laid out as perm."""
    if perm is None:
        return None
    import torch
    p = np.asarray(perm, np.int64)
    iv = np.empty_like(p)
    iv[p] = np.arange(p.size, dtype=np.int64)
    return engine._to_dev(iv, torch.int64)


def summary_outputs(engine, batch, out, want: Optional[Sequence[str]] = None,
                    midday=_lib.BATT_SUMMARY_MIDDAY) -> Dict[str, object]:
    """Engine.batt_summary of a batch sized (or evaluated) into `out`, with the
    columns gathered back to caller order (batch.perm): {member: [12, n]
    device tensor}."""
    d = engine.batt_summary(batch, out, want, midday)
    inv = _inverse(engine, batch.perm)
    if inv is None:
        return d
    return {k: v.index_select(1, inv) for k, v in d.items()}


def replay_outputs(engine, batch, kw, bank_kwh, bank_kw=None, want: Optional[Sequence[str]] = None,
                   midday=_lib.BATT_SUMMARY_MIDDAY, planes=None) -> Dict[str, object]:
    """Engine.replay_at in caller order: the dispatch replayed with kw[k] kW of
    PV and a bank of bank_kwh[k] kWh / bank_kw[k] kW (None: bank_kwh / 2) for
    caller row k -- the point a what-if call priced (batt_sizing.best_point,
    Engine.size_with_batt), not only the reference's kW / 0.8 at 2 h.  The [n]
    inputs (host arrays or device tensors) are laid out in the batch's device
    order (batch.perm) for the call and the results gathered back:
    {member: [12, n]} like summary_outputs, plus bank_kwh, power_kw (the bank
    as sized, what annual() takes) and status, each [n].  planes ("f32" /
    "f64"): baseline, pvonly and with_batt come back as the hour-quad tiles
    [NH / 4, n, 4] with their columns still in the batch's device order, the
    form Engine.plane_digest and attachment.state_hourly take."""
    import torch
    perm = batch.perm
    pt = None if perm is None else engine._to_dev(np.asarray(perm, np.int64), torch.int64)

    def dev_order(v):
        if v is None:
            return None
        t = engine._to_dev(v, torch.float64)
        return t if pt is None else t.index_select(0, pt)

    d = engine.replay_at(batch, dev_order(kw), dev_order(bank_kwh), dev_order(bank_kw), want, midday, planes)
    inv = _inverse(engine, perm)
    if inv is None:
        return d
    return {k: v if k in _lib.REPLAY_PLANES else v.index_select(v.dim() - 1, inv) for k, v in d.items()}


def annual(d: Dict[str, object], bank_kwh, cfg) -> Dict[str, object]:
    """A summary's [12, n] months -> [n] annual values (device tensors, or
    numpy arrays when d holds numpy arrays):
      the *_kwh members and the hour counts   the twelve months added in month
                                              order (((m0 + m1) + m2) + ...)
      soc_min, soc_max                        min / max over the months
      soc_end                                 December's
      capture_mid_frac       pv_to_batt_mid / surplus_mid, 0 where the midday
                             surplus is <= 1e-9 kWh
      equiv_full_cycles      batt_to_load / eta_out / (bank x (max_soc -
                             min_soc)): the energy drawn from the cells over the
                             usable capacity; 0 without a bank
      self_sufficiency_frac  1 - grid_to_load / load with load = pv_to_load +
                             batt_to_load + grid_to_load; 0 where load is 0
    bank_kwh: [n], the agents' batt_kwh in d's column order; cfg: the engine's
    EngineConfig (batt_eta_out, batt_max_soc, batt_min_soc).  Members d lacks
    are left out, a ratio with them."""
    res = {}
    for k in KWH_MEMBERS + COUNT_MEMBERS:
        if k in d:
            s = d[k][0]
            for m in range(1, d[k].shape[0]):
                s = s + d[k][m]
            res[k] = s
    if "soc_min" in d:
        xp = _xp(d["soc_min"])
        s = d["soc_min"][0]
        for m in range(1, d["soc_min"].shape[0]):
            s = xp.minimum(s, d["soc_min"][m])
        res["soc_min"] = s
    if "soc_max" in d:
        xp = _xp(d["soc_max"])
        s = d["soc_max"][0]
        for m in range(1, d["soc_max"].shape[0]):
            s = xp.maximum(s, d["soc_max"][m])
        res["soc_max"] = s
    if "soc_end" in d:
        res["soc_end"] = d["soc_end"][d["soc_end"].shape[0] - 1] + 0.0
    if "pv_to_batt_mid_kwh" in res and "surplus_mid_kwh" in res:
        num, den = res["pv_to_batt_mid_kwh"], res["surplus_mid_kwh"]
        xp = _xp(den)
        ok = den > 1e-9
        res["capture_mid_frac"] = xp.where(ok, num / xp.where(ok, den, xp.ones_like(den)), xp.zeros_like(den))
    if "batt_to_load_kwh" in res:
        b2l = res["batt_to_load_kwh"]
        xp = _xp(b2l)
        bank = bank_kwh if xp is not np else np.asarray(bank_kwh, np.float64)
        ok = bank > 0.0
        usable = xp.where(ok, bank, xp.ones_like(bank)) * (cfg.batt_max_soc - cfg.batt_min_soc)
        res["equiv_full_cycles"] = xp.where(ok, b2l / cfg.batt_eta_out / usable, xp.zeros_like(b2l))
    if all(k in res for k in ("pv_to_load_kwh", "batt_to_load_kwh", "grid_to_load_kwh")):
        g2l = res["grid_to_load_kwh"]
        xp = _xp(g2l)
        load = (res["pv_to_load_kwh"] + res["batt_to_load_kwh"]) + g2l
        ok = load > 0.0
        res["self_sufficiency_frac"] = xp.where(ok, 1.0 - g2l / xp.where(ok, load, xp.ones_like(load)),
                                                xp.zeros_like(load))
    return res


def state_monthly(engine, d: Dict[str, object], weight, idx, seg_off, members: Sequence[str] = KWH_MEMBERS):
    """Per segment and month, the weighted energy of each kWh member in MWh:
    sum over the segment's members of weight x d[member] / 1000 (weight: one
    per summary column, e.g. the adopters with storage,
    attachment.export_weights' w_batt).  idx: the summary column of each
    segment member (None: the columns themselves), seg_off [S + 1].  Each
    member is one Engine.segment_sums over its twelve month planes (k = 12).
    Returns a [S, 12, len(members)] float64 device tensor."""
    import torch
    members = tuple(members)
    bad = [k for k in members if k not in KWH_MEMBERS or k not in d]
    if bad or not members:
        raise ValueError(f"state_monthly: members must be kWh members of the summary (got {members})")
    w = engine._to_dev(weight, torch.float64)
    so = np.asarray(seg_off, dtype=np.int64)
    if so.ndim != 1 or so.size < 1 or so[0] != 0 or np.any(np.diff(so) < 0):
        raise ValueError("state_monthly: segment offsets must start at 0 and be non-decreasing")
    n = int(d[members[0]].shape[1])
    if int(w.numel()) != n:
        raise ValueError("state_monthly: one weight per summary column")
    ti = None
    if idx is not None:
        ix = np.asarray(idx, dtype=np.int64)
        if ix.shape != (int(so[-1]),) or (ix.size and (ix.min() < 0 or ix.max() >= n)):
            raise ValueError("state_monthly: idx must name one summary column per segment member")
        ti = engine._to_dev(ix, torch.int64)
    elif int(so[-1]) > n:
        raise ValueError("state_monthly: segments exceed the summary width")
    g = (lambda t: t) if ti is None else (lambda t: t.index_select(t.dim() - 1, ti).contiguous())
    wg = g(w)
    parts = [engine.segment_sums(g(d[k]), so, w1=wg) / 1000.0 for k in members]
    return torch.stack(parts, dim=2)


def annual_columns(engine, batch, out, midday=_lib.BATT_SUMMARY_MIDDAY) -> Dict[str, np.ndarray]:
    """The drop-in switch's per-agent columns (COLUMNS) of a sized output dict
    as host arrays in caller order: annual() of the batch's summary with
    bank_kwh = out["batt_kwh"], float64 except the hour counts (int64).  Only
    these [n] vectors cross to the host."""
    import torch
    inv = _inverse(engine, batch.perm)
    a = annual(engine.batt_summary(batch, out, None, midday), out["batt_kwh"], engine.cfg)
    res = {}
    for k in ANNUAL:
        t = a[k] if inv is None else a[k].index_select(0, inv)
        if t.dtype == torch.int32:
            t = t.to(torch.int64)
        res[PREFIX + k] = t.cpu().numpy()
    return res


def replay_columns(d: Dict[str, object], cfg, prefix: str = PREFIX) -> Dict[str, np.ndarray]:
    """annual_columns for a replay: the per-agent columns (prefix + each of
    ANNUAL) of replay_outputs' result `d` as host arrays in d's order --
    annual() with the bank the replay sized (d["bank_kwh"]), float64 except the
    hour counts (int64)."""
    a = annual({k: d[k] for k in _lib.BATT_SUMMARY_FIELDS}, d["bank_kwh"], cfg)
    res = {}
    for k in ANNUAL:
        t = a[k]
        if not isinstance(t, np.ndarray):
            t = t.cpu().numpy()
        res[prefix + k] = t.astype(np.int64) if t.dtype == np.int32 else t
    return res
