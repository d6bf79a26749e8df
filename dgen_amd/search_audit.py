"""Search trace and certificate audit of the sizing call.

The default mode (dgen_set_exact 1) keeps the fast search's Brent path for every
agent a bound on |device objective - reference objective| settles
(k_brent_certify).  ``Engine.search_trace``
(dgen_search_trace) lays that open: per agent the (x, f) evaluations of the
fast search, the error model, the bound the certificate carried to every
evaluation, and its decision.  This module is the host side of the audit:

    replay_x(f, lo, hi, xatol)        scipy's bounded Brent (the kernels' brent_bounded, op for
                                      op in Python floats) fed a list of objective values
    bracket_of(load_kwh, naep)        the bracket and xatol of ff:440-444
    bound_tables(...)                 the bound tables Engine.load_profiles / set_tariffs upload
    model_of(...)                     the certificate's error model restated from agent columns
    compare(trace, reference_traces)  observed / bound per agent and at worst
    audit_columns(engine, batch, out) the per-agent columns of the drop-in switch
                                      (financial_functions.size_frame(search_audit=True))

The reference traces are (x, f) pairs of a reference run's own search (the test
oracle's brent_trace); nothing here imports it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib

TRACE_MAX = _lib.TRACE_MAX
BT_GAMMA = 512.0                       # dgen_hip.hip BT_GAMMA
BT_EPS = 2.220446049250313e-16         # dgen_hip.hip BT_EPS
MAXY = _lib.MAXY
COLUMNS = ("search_nfev_fast", "search_certified", "search_rerun", "search_bound_usd")

_SQRT_EPS = 1.4832396974191326e-08     # sqrt(2.2e-16)
_GOLDEN = 0.3819660112501051           # 0.5 * (3 - sqrt(5))


def _sign(v: float) -> float:
    return 1.0 if v > 0.0 else (-1.0 if v < 0.0 else 0.0)


def replay_x(f: Sequence[float], lo: float, hi: float, xatol: float):
    """scipy 1.15.3 _minimize_scalar_bounded (maxfun 500) with the objective
    replaced by the list `f`: evaluation k returns f[k].  Returns (xs, nfev,
    xf): the arguments of the evaluations taken, their number and the search's
    result.  A search that asks for a value beyond the list stops there with
    nfev = len(f) + 1 and xf NaN (the device's truncated trace: 32 values, nfev
    33)."""
    f = [float(v) for v in f]
    a, b = float(lo), float(hi)
    xatol = float(xatol)
    fulc = a + _GOLDEN * (b - a)
    nfc = xf = fulc
    rat = e = 0.0
    x = xf
    fx = ffulc = fnfc = 0.0
    num = 0
    xs: List[float] = []
    while True:
        if num >= len(f):
            return xs, len(f) + 1, math.nan
        fu = f[num]
        xs.append(x)
        num += 1
        if num == 1:
            fx = ffulc = fnfc = fu
        elif fu <= fx:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if fu <= fnfc or nfc == xf:
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif fu <= ffulc or fulc == xf or fulc == nfc:
                fulc, ffulc = x, fu
        xm = 0.5 * (a + b)
        tol1 = _SQRT_EPS * abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= 500:
            break
        if not (abs(xf - xm) > (tol2 - 0.5 * (b - a))):
            break
        golden = True
        if abs(e) > tol1:
            golden = False
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            r = e
            e = rat
            if abs(p) < abs(0.5 * q * r) and p > q * (a - xf) and p < q * (b - xf):
                rat = (p + 0.0) / q
                x = xf + rat
                if (x - a) < tol2 or (b - x) < tol2:
                    si = _sign(xm - xf) + (1.0 if (xm - xf) == 0.0 else 0.0)
                    rat = tol1 * si
            else:
                golden = True
        if golden:
            e = (a - xf) if xf >= xm else (b - xf)
            rat = _GOLDEN * e
        si = _sign(rat) + (1.0 if rat == 0.0 else 0.0)
        ar = abs(rat)
        x = xf + si * (ar if ar > tol1 else tol1)
    return xs, num, xf


def bracket_of(load_kwh: float, naep: float):
    """(low, high, xatol) of an agent's search as k_size forms them (ff:440-444)."""
    max_load = float(load_kwh) / float(naep)
    low, high = max_load * 0.8, max_load * 1.25
    span = high - low
    tl = (span if span > 1.0 else 1.0) * 1e-3
    fl = math.floor(tl) if math.isfinite(tl) else tl
    return low, high, (2.0 if fl < 2.0 else float(fl))


def bound_tables(shapes, cfs, wholesale, tariffs, demand=None) -> Dict[str, object]:
    """The tables the error model reads, as Engine.load_profiles and
    Engine.set_tariffs derive them: the profile rows' sums (numpy's) and
    absolute maxima, the wholesale rows' maxima and the tariffs' price bounds
    (engine.tariff_price_bounds over the records with their peak records
    attached).  `demand`: the demand table the engine was given (None in the
    reference's mode).  A member set to None afterwards is a missing table."""
    from .engine import tariff_price_bounds
    from .tariff import attach_peak_records
    sh = np.asarray(shapes)
    cf = np.asarray(cfs)
    recs, dem, _ = attach_peak_records(tariffs, demand)
    ws = None if wholesale is None or not len(wholesale) else np.asarray(wholesale, np.float64)
    return {
        "shape_sum": sh.astype(np.float64).sum(axis=1),
        "cf_naep": (cf.astype(np.float64) / 1e6).sum(axis=1),       # ff:350-351: gen_per_kw.sum()
        "bt_shape_max": np.abs(sh).max(axis=1).astype(np.float64),
        "bt_cf_max": np.abs(cf).max(axis=1).astype(np.float64),
        "bt_ts_max": None if ws is None else np.nan_to_num(np.abs(ws), nan=0.0, posinf=0.0).max(axis=1),
        "bt_tariff": tariff_price_bounds(recs, dem),
        "records": recs,
        "has_wholesale": ws is not None,
    }


def _prices(tb, skip_dc: int, tix: int, pm: float, pmdc: float, pku: float, mo2: bool):
    """bt_prices: the price bounds of tariff tix folded into (pm, pmdc, pku, mo2)."""
    t = tb["records"][tix]
    mo2 = mo2 or int(t["mo"]) == 2
    bt = tb.get("bt_tariff")
    if bt is not None:
        return (max(pm, float(bt[tix, 0])), max(pmdc, float(bt[tix, 1]) if skip_dc == 0 else 0.0),
                max(pku, float(bt[tix, 2])), mo2)
    P, T = int(t["P"]), int(t["T"])
    e = max(float(np.abs(t["buy"][:P, :T]).max(initial=0.0)), float(np.abs(t["sell"][:P, :T]).max(initial=0.0)))
    cap = float(np.abs(t["cap"][:T]).sum())
    pm = max(pm, e)
    u = int(t["unit"])
    if u in (1, 3):
        pku = max(pku, 2.0 * e * cap * (31.0 if u == 3 else 1.0))
    if skip_dc == 0 and int(t["dc"]) > 0:
        pmdc = math.inf                   # no bound without the table
    return pm, pmdc, pku, mo2


def model_of(cols, switches, tables: Dict[str, object], skip_demand_charges: int = 1,
             nm_yearend_sell_rate: float = 0.02, rows: Optional[Sequence[int]] = None) -> np.ndarray:
    """The error model k_brent_certify builds (BtModel: c0, c1, ce, lip),
    restated on the host from the agent columns `cols`, the switch table and
    bound_tables' result: [n, 4] float64.  |f_device - f_reference| <= c0 + c1
    |x| + ce |f| at the same x, |f(x) - f(x')| <= lip |x - x'|.  An agent whose
    model lacks a bound table (bt_ts_max for a TS sell-rate agent, bt_shape_max
    / bt_cf_max under demand charges) or names a switch row outside the tariff
    table gets non-finite members (NaN where the kernel stops building); the
    kernel then certifies nothing for it.  The running products may be ordered
    differently from the device's: equal to ~1e-12 relative, not bit for bit."""
    n = len(cols["load_kwh"])
    ix = range(n) if rows is None else rows
    recs = tables["records"]
    n_t = len(recs)
    out = np.full((n, 4), np.nan)
    g = BT_GAMMA * BT_EPS
    for i in ix:
        N = int(cols["econ_life"][i])
        kwh = float(cols["load_kwh"][i])
        lr, cr = int(cols["load_row"][i]), int(cols["cf_row"][i])
        naep0 = float(tables["cf_naep"][cr])
        pm, pmdc, pku, otc, mo2 = abs(float(nm_yearend_sell_rate)), 0.0, 0.0, 0.0, False
        pm, pmdc, pku, mo2 = _prices(tables, skip_demand_charges, int(cols["tariff0"][i]), pm, pmdc, pku, mo2)
        off, cnt = int(cols["sw_solar_off"][i]), int(cols["sw_solar_cnt"][i])
        ok = True
        for r in switches[off:off + cnt]:
            tt = int(r["tariff"])
            if tt < 0 or tt >= n_t:
                ok = False
                break
            pm, pmdc, pku, mo2 = _prices(tables, skip_demand_charges, tt, pm, pmdc, pku, mo2)
            otc = max(otc, abs(float(r["one_time_charge"])))
        is_ca = (int(cols["flags"][i]) & 2) != 0
        wr = int(cols["wholesale_row"][i])
        if mo2 and not is_ca and wr >= 0 and tables.get("has_wholesale"):
            if tables.get("bt_ts_max") is None:
                ok = False
            else:
                pm = max(pm, float(tables["bt_ts_max"][wr]) * abs(float(cols["price_mult"][i])) * (1.0 + 1e-6))
        infl, real = float(cols["inflation"][i]), float(cols["real_discount"][i])
        rr = 1.0 / ((1.0 + real) * (1.0 + infl))
        rb = abs(1.0 + infl + float(cols["escalator"][i]))
        sb = abs(1.0 - float(cols["pv_deg"][i]))
        D, dr, er, smax, sy = 0.0, 1.0, 1.0, 1.0, 1.0
        for _ in range(1, min(N, MAXY) + 1):
            dr *= rr
            D += dr * er
            er *= rb
            smax = max(smax, sy)
            sy *= sb
        D *= 1.01
        S = float(tables["shape_sum"][lr])
        lmax = (float(tables["bt_shape_max"][lr]) * abs(kwh / S)) if tables.get("bt_shape_max") is not None else math.inf
        gmax = float(tables["bt_cf_max"][cr]) * 1e-6 if tables.get("bt_cf_max") is not None else math.inf
        capc = abs(float(cols["capex"][i]) * float(cols["ccm"][i]))
        dem = pmdc + pku
        c0 = g * (2.0 * D * pm * 2.0 * abs(kwh) + (4.0 * D * dem * 24.0 * lmax if dem > 0.0 else 0.0) + otc)
        c1 = g * (2.0 * D * smax * 0.96 * pm * abs(naep0)
                  + (4.0 * D * smax * 0.96 * dem * 12.0 * gmax if dem > 0.0 else 0.0) + 4.0 * capc)
        lip = ((3.0 + 0.02 * D) * capc + 2.2 * D * smax * 0.96 * pm * abs(naep0)
               + (4.0 * D * smax * 0.96 * dem * 12.0 * gmax if dem > 0.0 else 0.0))
        out[i] = (c0, c1, g, lip) if ok else (math.nan, math.nan, g, math.nan)
    return out


def _ratio(diff: float, bound: float) -> float:
    if diff == 0.0:
        return 0.0
    return diff / bound if bound > 0.0 else math.inf


def compare(trace: Dict[str, np.ndarray], reference_traces: Sequence[Optional[np.ndarray]]) -> Dict[str, object]:
    """Observed / bound of a device trace (Engine.search_trace's members x, f,
    f_bound, x_bound, nfev, certified as host arrays) against the reference's
    own searches: reference_traces[i] is agent i's [nfev_ref, 2] array of (x,
    f) pairs, or None / empty for an agent to leave out.  The rule, per agent:
    evaluation k is compared while the certificate has a row for it (f_bound[k]
    not NaN), both searches took it, and every earlier evaluation had |x_device
    - x_reference| <= x_bound; at a compared k the certificate claims
    |f_device[k] - f_reference[k]| <= f_bound[k].  Returns per-agent arrays
      compared      evaluations compared (0: none, or no search)
      ratio_f       max over them of |f_d - f_r| / f_bound (0 where equal; inf
                    for a difference against a zero bound; NaN: none compared)
      ratio_x       the same of |x_d - x_r| / x_bound
      f_violations  compared evaluations with |f_d - f_r| > f_bound
      x_violations  compared evaluations with |x_d - x_r| > x_bound
      x0_equal      x[0] equals the reference's bit for bit
      nfev_equal    the device's fast nfev equals the reference's
    and the scalars worst_f, worst_x (max of the ratios, 0.0 with nothing
    compared), agents (compared > 0) and deep (agents with >= 3 evaluations
    compared)."""
    x, f = np.asarray(trace["x"]), np.asarray(trace["f"])
    fb, xb = np.asarray(trace["f_bound"]), np.asarray(trace["x_bound"])
    nfev = np.asarray(trace["nfev"])
    n = x.shape[0]
    res = {"compared": np.zeros(n, np.int64), "ratio_f": np.full(n, np.nan), "ratio_x": np.full(n, np.nan),
           "f_violations": np.zeros(n, np.int64), "x_violations": np.zeros(n, np.int64),
           "x0_equal": np.zeros(n, bool), "nfev_equal": np.zeros(n, bool)}
    for i in range(n):
        ref = None if reference_traces[i] is None else np.asarray(reference_traces[i], np.float64).reshape(-1, 2)
        if ref is None or not len(ref) or nfev[i] <= 0:
            continue
        res["x0_equal"][i] = x[i, 0] == ref[0, 0]
        res["nfev_equal"][i] = int(nfev[i]) == len(ref)
        rf = rx = 0.0
        for k in range(min(int(nfev[i]), TRACE_MAX, len(ref))):
            if math.isnan(fb[i, k]):
                break
            df, dx = abs(f[i, k] - ref[k, 1]), abs(x[i, k] - ref[k, 0])
            res["compared"][i] += 1
            rf, rx = max(rf, _ratio(df, fb[i, k])), max(rx, _ratio(dx, xb[i, k]))
            res["f_violations"][i] += int(not df <= fb[i, k])
            if not dx <= xb[i, k]:
                res["x_violations"][i] += 1
                break
        if res["compared"][i]:
            res["ratio_f"][i], res["ratio_x"][i] = rf, rx
    got = res["compared"] > 0
    res["agents"] = int(got.sum())
    res["deep"] = int((res["compared"] >= 3).sum())
    res["worst_f"] = float(np.max(res["ratio_f"][got])) if got.any() else 0.0
    res["worst_x"] = float(np.max(res["ratio_x"][got])) if got.any() else 0.0
    return res


def audit_columns(engine, batch, out) -> Dict[str, np.ndarray]:
    """The drop-in switch's per-agent columns (COLUMNS) of a batch just sized
    into `out`, as host arrays in caller order:
      search_nfev_fast   evaluations of the fast search (int64; 33: truncated)
      search_certified   1 the bound settled the search, 0 not, -1 no search
      search_rerun       certified == 0: the agent mode 1 re-runs in the
                         reference's arithmetic (bool)
      search_bound_usd   the certificate's bound of |device - reference| on the
                         objective, at the evaluation that gave the fast
                         search's system_kw (NaN: no search, truncated, or the
                         certificate stopped before that evaluation)
    Only these [n] vectors cross to the host."""
    import torch
    from .batt_metrics import _inverse
    t = engine.search_trace(batch, out, ("x", "f_bound", "system_kw", "nfev", "certified"))
    hit = t["x"] == t["system_kw"].unsqueeze(1)          # NaN rows never match
    k = hit.to(torch.int8).argmax(dim=1, keepdim=True)   # the first evaluation at system_kw
    bound = torch.where(hit.any(dim=1), t["f_bound"].gather(1, k).squeeze(1),
                        torch.full_like(t["system_kw"], float("nan")))
    inv = _inverse(engine, batch.perm)
    g = (lambda v: v) if inv is None else (lambda v: v.index_select(0, inv))
    cert = g(t["certified"]).cpu().numpy().astype(np.int64)
    return {"search_nfev_fast": g(t["nfev"]).cpu().numpy().astype(np.int64), "search_certified": cert,
            "search_rerun": cert == 0, "search_bound_usd": g(bound).cpu().numpy()}
