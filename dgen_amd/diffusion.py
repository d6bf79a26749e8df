"""Diffusion step on the device: drop-ins for

    financial_functions.calc_max_market_share(dataframe, max_market_share_df)   ff:1264-1310
    diffusion_functions_elec.calc_diffusion_solar(df, is_first_year, bass_params, year, ...)
                                                                                 diffusion_functions_elec.py:24-156

The pandas merges that attach per-(state, sector) Bass parameters and the curve
keys stay on the host, exactly as the reference writes them; the per-agent
arithmetic (payback clip / round / curve lookup, equivalent time, Bass step,
market-share floor and cap, cumulative updates) runs in k_max_market_share /
k_diffusion through the C-ABI.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import numpy as np
import pandas as pd

from . import _lib

ANCHOR_YEARS = (2014, 2016, 2018)
# config.OBSERVED_DEPLOYMENT_BY_STATE of the reference (config.py:67): the CSV of
# observed PV / storage deployment by (state, sector, year) that the anchor
# years rescale to.  Set it, or pass observed_deployment= to calc_diffusion_solar.
OBSERVED_DEPLOYMENT_BY_STATE = None

_LAST_YEAR_COLS = ['agent_id', 'market_share', 'max_market_share', 'number_of_adopters',
                   'market_value', 'initial_number_of_adopters', 'initial_pv_kw', 'initial_batt_kw',
                   'initial_batt_kwh', 'initial_market_share', 'initial_market_value',
                   'system_kw_cum', 'new_system_kw', 'batt_kw_cum', 'new_batt_kw', 'batt_kwh_cum',
                   'new_batt_kwh']
_LAST_YEAR_RENAME = {'market_share': 'market_share_last_year',
                     'max_market_share': 'max_market_share_last_year',
                     'number_of_adopters': 'adopters_cum_last_year',
                     'market_value': 'market_value_last_year',
                     'system_kw_cum': 'system_kw_cum_last_year',
                     'batt_kw_cum': 'batt_kw_cum_last_year',
                     'batt_kwh_cum': 'batt_kwh_cum_last_year'}
DIFF_IN = ["max_market_share", "market_share_last_year", "bass_p", "bass_q", "teq_yr1",
           "developable_agent_weight", "system_kw", "system_capex_per_kw", "adopters_cum_last_year",
           "market_value_last_year", "system_kw_cum_last_year"]
DIFF_OUT = ["mms_fix_zeros", "ratio", "bass_params_teq", "teq2", "f", "new_adopt_fraction",
            "bass_market_share", "diffusion_market_share", "market_share", "new_market_share",
            "new_adopters", "new_market_value", "new_system_kw", "number_of_adopters",
            "market_value", "system_kw_cum"]


class MmsTable(ctypes.Structure):
    _fields_ = [("mms", ctypes.c_void_p), ("n_rows", ctypes.c_int32), ("n_factors", ctypes.c_int32),
                ("factor_min", ctypes.c_int32), ("pad", ctypes.c_int32), ("min_pb", ctypes.c_double),
                ("max_pb", ctypes.c_double)]


class DiffIn(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in DIFF_IN]


class DiffOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in DIFF_OUT]


def _bind(L):
    if getattr(L, "_dgen_diff_bound", False):
        return L
    L.dgen_max_market_share.restype = ctypes.c_int32
    L.dgen_max_market_share.argtypes = [ctypes.c_void_p, ctypes.POINTER(MmsTable), ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.dgen_diffusion.restype = ctypes.c_int32
    L.dgen_diffusion.argtypes = [ctypes.c_void_p, ctypes.POINTER(DiffIn), ctypes.POINTER(DiffOut),
                                 ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    L._dgen_diff_bound = True
    return L


def mms_table(max_market_share_df: pd.DataFrame):
    """Dense (sector -> row) x (factor) table of the rows the reference's merge
    can hit: metric 'payback_period', business_model 'host_owned' (ff:1299-1307).
    Returns (table [rows, F], {sector: row}, factor_min, min_pb, max_pb)."""
    pb_rows = max_market_share_df.loc[max_market_share_df.metric == 'payback_period', 'payback_period']
    max_pb, min_pb = float(pb_rows.max()), float(pb_rows.min())
    sub = max_market_share_df[(max_market_share_df['metric'] == 'payback_period') &
                              (max_market_share_df['business_model'] == 'host_owned')].copy()
    fac = (sub['payback_period'] * 100).round()
    fac = fac.replace([np.inf, -np.inf], np.nan)
    sub = sub.assign(_f=fac).dropna(subset=['_f'])
    if sub.duplicated(subset=['sector_abbr', '_f']).any():
        raise NotImplementedError("duplicate (sector, payback) curve points: the reference's merge "
                                  "would duplicate agent rows")
    sectors = list(dict.fromkeys(sub['sector_abbr'].tolist()))
    rows = {s: k for k, s in enumerate(sectors)}
    if len(sub):
        fmin, fmax = int(sub['_f'].min()), int(sub['_f'].max())
    else:
        fmin, fmax = 0, -1
    F = fmax - fmin + 1
    tab = np.full((max(len(sectors), 1), max(F, 1)), np.nan)
    for s, f, v in zip(sub['sector_abbr'], sub['_f'].astype(np.int64), sub['max_market_share']):
        tab[rows[s], int(f) - fmin] = float(v)
    return tab, rows, fmin, min_pb, max_pb


def _dev(engine, a, dtype):
    return engine._to_dev(np.asarray(a), dtype)


def max_market_share_arrays(engine, payback, row, tab, fmin: int, min_pb: float, max_pb: float
                            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Run k_max_market_share on host columns: payback [n] float64 and the
    agents' curve rows [n] int32 (-1: no curve) against mms_table()'s dense
    table -> (payback_period_bounded float64, payback_period_as_factor int64,
    max_market_share float64)."""
    import torch
    L = _bind(engine.lib)
    tab = np.asarray(tab, dtype=np.float64)
    n = len(payback)
    t_tab = _dev(engine, tab, torch.float64)
    t_pb, t_row = _dev(engine, payback, torch.float64), _dev(engine, row, torch.int32)
    b = torch.empty(n, dtype=torch.float64, device=engine.dev)
    fct = torch.empty(n, dtype=torch.int64, device=engine.dev)
    mms = torch.empty(n, dtype=torch.float64, device=engine.dev)
    tb = MmsTable(mms=t_tab.data_ptr(), n_rows=tab.shape[0], n_factors=tab.shape[1],
                  factor_min=fmin, pad=0, min_pb=min_pb, max_pb=max_pb)
    _lib.check(L.dgen_max_market_share(engine.ctx, ctypes.byref(tb), t_pb.data_ptr(), t_row.data_ptr(),
                                       n, b.data_ptr(), fct.data_ptr(), mms.data_ptr(),
                                       engine.stream_handle()), "dgen_max_market_share")
    torch.cuda.synchronize(engine.dev)
    return b.cpu().numpy(), fct.cpu().numpy(), mms.cpu().numpy()


def calc_max_market_share(dataframe: pd.DataFrame, max_market_share_df: pd.DataFrame,
                          engine=None) -> pd.DataFrame:
    """ff:1264 -- attach max_market_share by (sector_abbr, payback factor)."""
    from .financial_functions import get_engine
    eng = engine or get_engine()
    in_cols = list(dataframe.columns)
    df = dataframe.reset_index()
    df['business_model'] = 'host_owned'
    df['metric'] = 'payback_period'
    tab, rows, fmin, min_pb, max_pb = mms_table(max_market_share_df)
    row = np.array([rows.get(s, -1) for s in df['sector_abbr']], dtype=np.int32)
    pb = df['payback_period'].to_numpy(dtype=np.float64)
    b, fct, mms = max_market_share_arrays(eng, pb, row, tab, fmin, min_pb, max_pb)
    df['payback_period_bounded'] = b
    df['payback_period_as_factor'] = pd.array(fct, dtype='Int64')
    df['max_market_share'] = mms
    return df[in_cols + ['max_market_share', 'metric']]


def diffusion_arrays(engine, cols: Dict[str, np.ndarray], is_first_year: bool) -> Dict[str, np.ndarray]:
    """Run k_diffusion on host columns (DIFF_IN names) -> DIFF_OUT arrays."""
    import torch
    L = _bind(engine.lib)
    n = len(cols["system_kw"])
    keep = {k: _dev(engine, np.asarray(cols[k], dtype=np.float64), torch.float64) for k in DIFF_IN}
    outs = {k: torch.empty(n, dtype=torch.float64, device=engine.dev) for k in DIFF_OUT}
    din = DiffIn(**{k: keep[k].data_ptr() for k in DIFF_IN})
    dout = DiffOut(**{k: outs[k].data_ptr() for k in DIFF_OUT})
    _lib.check(L.dgen_diffusion(engine.ctx, ctypes.byref(din), ctypes.byref(dout), n,
                                int(bool(is_first_year)), engine.stream_handle()), "dgen_diffusion")
    torch.cuda.synchronize(engine.dev)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _observed_table(observed_deployment) -> pd.DataFrame:
    src = observed_deployment if observed_deployment is not None else OBSERVED_DEPLOYMENT_BY_STATE
    if src is None:
        raise FileNotFoundError("anchor years (2014/2016/2018) need the observed deployment table: "
                                "set dgen_amd.diffusion.OBSERVED_DEPLOYMENT_BY_STATE (the reference's "
                                "config.OBSERVED_DEPLOYMENT_BY_STATE) or pass observed_deployment=")
    obs = src if isinstance(src, pd.DataFrame) else pd.read_csv(src)
    if obs.duplicated(subset=['state_abbr', 'sector_abbr', 'year']).any():
        raise ValueError("observed deployment table has duplicate (state, sector, year) rows: the "
                         "reference's merge would duplicate agent rows")
    return obs


def anchor_to_observed(eng, df: pd.DataFrame, observed: pd.DataFrame) -> pd.DataFrame:
    """diffusion_functions_elec.py:99-133 -- in an anchor year, rescale each
    agent's PV cumulative capacity so its (state, sector, year) group totals
    the observed MW, then re-derive adopters and market share from it (battery
    columns untouched).  The group totals are device segment sums
    (dgen_segment_sums, fixed order) over the agents sorted by group; pandas'
    groupby sum skips NaN, so NaN capacities enter as 0.  Rows whose group key
    has a NaN, or whose group the table lacks, get NaN capacity like the
    reference's left merges."""
    import torch
    group_cols = ['state_abbr', 'sector_abbr', 'year']
    n = len(df)
    # ngroup() gives NaN (pandas 2.x) for a row whose key has a NaN: -1 here
    gid = df.groupby(group_cols, sort=False, dropna=True).ngroup().fillna(-1).to_numpy(np.int64)
    ok = gid >= 0
    G = int(gid.max()) + 1 if ok.any() else 0
    order = np.argsort(np.where(ok, gid, G), kind="stable")[:int(ok.sum())]
    cnt = np.bincount(gid[ok], minlength=G)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    kw = df['system_kw_cum'].to_numpy(dtype=np.float64)
    v = eng._to_dev(np.nan_to_num(kw[order], nan=0.0, posinf=np.inf, neginf=-np.inf), torch.float64)
    tot = eng.segment_sums(v, off)[:, 0].cpu().numpy() if G else np.zeros(0)
    state_sum = np.full(n, np.nan)
    count = np.full(n, np.nan)
    state_sum[ok] = tot[gid[ok]]
    count[ok] = cnt[gid[ok]]
    df = pd.merge(df, observed, how='left', on=group_cols)
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = np.where(state_sum == 0, 1.0 / count, kw / state_sum)
    cum = scale * df['observed_solar_mw'].to_numpy(dtype=np.float64) * 1000.0
    df['system_kw_cum'] = cum
    df['number_of_adopters'] = np.where(df['sector_abbr'] == 'res', cum / 5.0, cum / 100.0)
    w = df['developable_agent_weight'].to_numpy(dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        df['market_share'] = np.where(w == 0, 0.0, df['number_of_adopters'].to_numpy() / w).astype(np.float64)
    return df.drop(columns=['observed_solar_mw'])


def calc_diffusion_solar(df, is_first_year, bass_params, year, override_p_value=None,
                         override_q_value=None, override_teq_yr1_value=None, engine=None,
                         observed_deployment=None):
    """diffusion_functions_elec.py:24 -- PV Bass diffusion for the solve year.
    (The reference accepts but does not apply the override_* arguments.)
    In the anchor years 2014/2016/2018 the PV cumulatives are rescaled to the
    observed deployment table (anchor_to_observed)."""
    from .financial_functions import get_engine
    observed = _observed_table(observed_deployment) if year in ANCHOR_YEARS else None
    eng = engine or get_engine()
    df = df.reset_index()
    bass_params = bass_params[bass_params['tech'] == 'solar']
    df = pd.merge(df, bass_params[['state_abbr', 'bass_param_p', 'bass_param_q', 'teq_yr1',
                                   'sector_abbr']], how='left', on=['state_abbr', 'sector_abbr'])
    cols = {"max_market_share": df['max_market_share'], "market_share_last_year": df['market_share_last_year'],
            "bass_p": df['bass_param_p'], "bass_q": df['bass_param_q'], "teq_yr1": df['teq_yr1'],
            "developable_agent_weight": df['developable_agent_weight'], "system_kw": df['system_kw'],
            "system_capex_per_kw": df['system_capex_per_kw'],
            "adopters_cum_last_year": df['adopters_cum_last_year'],
            "market_value_last_year": df['market_value_last_year'],
            "system_kw_cum_last_year": df['system_kw_cum_last_year']}
    o = diffusion_arrays(eng, {k: v.to_numpy(dtype=np.float64) for k, v in cols.items()}, is_first_year)
    for k in ("mms_fix_zeros", "ratio", "bass_params_teq", "teq2", "f", "new_adopt_fraction",
              "bass_market_share", "diffusion_market_share", "market_share", "new_market_share",
              "new_adopters", "new_market_value", "new_system_kw"):
        df[k] = o[k]
    df['new_batt_kw'] = 0.0
    df['new_batt_kwh'] = 0.0
    df['number_of_adopters'] = o['number_of_adopters']
    df['market_value'] = o['market_value']
    df['system_kw_cum'] = o['system_kw_cum']
    df['batt_kw_cum'] = df['batt_kw_cum_last_year']
    df['batt_kwh_cum'] = df['batt_kwh_cum_last_year']
    if observed is not None:
        df = anchor_to_observed(eng, df, observed)
    market_last_year = df[_LAST_YEAR_COLS].rename(columns=_LAST_YEAR_RENAME)
    return df, market_last_year
