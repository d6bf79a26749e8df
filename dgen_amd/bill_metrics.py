"""Year-1 monthly bill breakdown per agent, on the device.

The sizing kernels reduce a year's bill to one number per case;
``Engine.bill_months`` (dgen_bill_months) replays an agent's profile rows at a
given size under a given tariff and writes, per calendar month, the energy
charge, the export credit, the fixed and demand charges, the total, the kWh
credit bank or dollar carry-over after the month, the imported, exported and
billed kWh and the peak (the definitions are in include/dgen_hip.h).  This
module carries that up:

    bill_outputs(engine, batch, out)      the three cases of a sized output dict --
                                          baseline (0 kW), pvonly (x_last), with_batt
                                          (system_kw, the battery dispatched) -- all
                                          under out["tariff_final"], caller order
    annual(d)                             the twelve months reduced to the year, [n]
    state_monthly(...)                    per segment and month, weighted member sums
    annual_columns(engine, batch, out)    the per-agent columns of the drop-in switch
                                          (financial_functions.size_frame(bill_metrics=True))
    what_if(engine, batch, kw, k)         every agent billed under tariff k of the table

All three cases are billed under tariff_final, the sticky tariff after the
search and the battery run's storage rate switch.  The engine's
first_with / bill_w_pv come from the search's tariff: the pvonly case
reproduces them only where the storage rate switch did not move the tariff
(the with_batt case reproduces bill_w_batt[1], the baseline bill_wo_batt[1]).
Utilityrate5's counterparts are its year1_monthly_* and charge_w_sys_*_ym
outputs, which the reference drops.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from .batt_metrics import _inverse, _xp

CASES = ("baseline", "pvonly", "with_batt")
# the members annual_columns needs
MEMBERS = ("energy_charge", "export_credit", "fixed_charge", "demand_flat", "demand_tou", "total")
SUM_MEMBERS = tuple(k for k in _lib.BILL_FIELDS if k not in ("carry", "peak_kw"))
# annual_columns' names per case, and the annual() member (or pair, added) behind each
_COLS = (("energy", ("energy_charge",)), ("credit", ("export_credit",)), ("fixed", ("fixed_charge",)),
         ("demand", ("demand_flat", "demand_tou")), ("total", ("total",)))
PREFIX = "bill_"
COLUMNS = tuple(f"{PREFIX}{c}_{case}" for case in CASES for c in [k for k, _ in _COLS] + ["max_month"])


def bill_outputs(engine, batch, out, want: Optional[Sequence[str]] = None) -> Dict[str, Dict[str, object]]:
    """Engine.bill_months of a batch sized (or evaluated) into `out` (the
    alloc_outputs dict), for the three cases, each under out["tariff_final"]:
    {case: {member: [12, n] device tensor, "status": [n]}} with the columns
    gathered back to caller order (batch.perm)."""
    tf = out["tariff_final"]
    import torch
    runs = (("baseline", torch.zeros_like(out["system_kw"]), False), ("pvonly", out["x_last"], False),
            ("with_batt", out["system_kw"], True))
    inv = _inverse(engine, batch.perm)
    res = {}
    for case, kw, battery in runs:
        d = engine.bill_months(batch, kw, tf, battery=battery, want=want)
        res[case] = d if inv is None else {k: v.index_select(v.dim() - 1, inv) for k, v in d.items()}
    return res


def annual(d: Dict[str, object]) -> Dict[str, object]:
    """One case's [12, n] months -> [n] annual values (device tensors, or numpy
    arrays when d holds numpy arrays):
      every dollar and kWh member   the twelve months added in month order
                                    (((m0 + m1) + m2) + ...)
      carry                         December's
      peak_kw                       the maximum over the months
      max_month                     the month (0 to 11, int64) of the largest
                                    total, the first of equal ones
    Members d lacks are left out."""
    res = {}
    for k in SUM_MEMBERS:
        if k in d:
            s = d[k][0]
            for m in range(1, d[k].shape[0]):
                s = s + d[k][m]
            res[k] = s
    if "carry" in d:
        res["carry"] = d["carry"][d["carry"].shape[0] - 1] + 0.0
    if "peak_kw" in d:
        xp = _xp(d["peak_kw"])
        s = d["peak_kw"][0]
        for m in range(1, d["peak_kw"].shape[0]):
            s = xp.maximum(s, d["peak_kw"][m])
        res["peak_kw"] = s
    if "total" in d:
        t = d["total"]
        xp = _xp(t)
        best = t[0]
        arg = np.zeros(best.shape, np.int64) if xp is np else xp.zeros_like(best, dtype=xp.int64)
        for m in range(1, t.shape[0]):
            up = t[m] > best
            best = xp.where(up, t[m], best)
            arg = xp.where(up, xp.full_like(arg, m), arg)
        res["max_month"] = arg
    return res


def state_monthly(engine, d: Dict[str, object], weight, idx, seg_off, members: Sequence[str] = ("total",)):
    """Per segment and month, the weighted sum of each member of one case:
    sum over the segment's members of weight x d[member] (weight: one per
    column of d, e.g. the adopters).  idx: the column of each segment member
    (None: the columns themselves), seg_off [S + 1].  Each member is one
    Engine.segment_sums over its twelve month planes (k = 12), as
    batt_metrics.state_monthly.  Returns a [S, 12, len(members)] float64
    device tensor."""
    import torch
    members = tuple(members)
    bad = [k for k in members if k not in _lib.BILL_FIELDS or k not in d]
    if bad or not members:
        raise ValueError(f"state_monthly: members must be bill members of d (got {members})")
    w = engine._to_dev(weight, torch.float64)
    so = np.asarray(seg_off, dtype=np.int64)
    if so.ndim != 1 or so.size < 1 or so[0] != 0 or np.any(np.diff(so) < 0):
        raise ValueError("state_monthly: segment offsets must start at 0 and be non-decreasing")
    n = int(d[members[0]].shape[1])
    if int(w.numel()) != n:
        raise ValueError("state_monthly: one weight per column")
    ti = None
    if idx is not None:
        ix = np.asarray(idx, dtype=np.int64)
        if ix.shape != (int(so[-1]),) or (ix.size and (ix.min() < 0 or ix.max() >= n)):
            raise ValueError("state_monthly: idx must name one column per segment member")
        ti = engine._to_dev(ix, torch.int64)
    elif int(so[-1]) > n:
        raise ValueError("state_monthly: segments exceed the width")
    g = (lambda t: t) if ti is None else (lambda t: t.index_select(t.dim() - 1, ti).contiguous())
    wg = g(w)
    return torch.stack([engine.segment_sums(g(d[k]), so, w1=wg) for k in members], dim=2)


def annual_columns(engine, batch, out) -> Dict[str, np.ndarray]:
    """The drop-in switch's per-agent columns (COLUMNS) of a sized output dict
    as host arrays in caller order: per case, annual() of bill_outputs --
    bill_energy_, bill_credit_, bill_fixed_, bill_demand_ (flat + TOU),
    bill_total_ (float64 dollars of year 1) and bill_max_month_ (int64).  Only
    these [n] vectors cross to the host."""
    res = {}
    for case, d in bill_outputs(engine, batch, out, want=MEMBERS).items():
        a = annual(d)
        for name, parts in _COLS:
            t = a[parts[0]]
            for k in parts[1:]:
                t = t + a[k]
            res[f"{PREFIX}{name}_{case}"] = t.cpu().numpy()
        res[f"{PREFIX}max_month_{case}"] = a["max_month"].cpu().numpy()
    return {k: res[k] for k in COLUMNS}


def what_if(engine, batch, kw, tariff_index: int, battery: bool = False, want=None) -> Dict[str, object]:
    """Every agent of `batch` billed at kw[j] (device order) under the one
    tariff `tariff_index` of the engine's table, whatever the agent's own:
    Engine.bill_months with tariff = tariff_index everywhere."""
    import torch
    k = int(tariff_index)
    return engine.bill_months(batch, kw, torch.full((batch.n,), k, dtype=torch.int32, device=engine.dev),
                              battery=battery, want=want)
