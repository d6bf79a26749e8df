"""ctypes binding of libdgen_hip.so (include/dgen_hip.h).

The product path has no CPU fallback: if the library is missing or a call
fails, this raises.  Struct layouts mirror the header field for field and are
checked against sizeof() probes in tests/test_abi.py.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

from . import build as _build

NH = 8760
NSLOT = 576
MAXP = 12
MAXT = 6
MAXY = 50
NB_CAPM = 192   # include/dgen_hip.h DGEN_NB_CAPM (mixed hours per month of a net-billing record)
DCR_CAP = 1024  # include/dgen_hip.h DGEN_DCR_CAP (kept hours per battery-case demand record)

ST_BOUNDS = 0x01
ST_TARIFF = 0x02
ST_EMPTY_EC = 0x04
ST_UNIT = 0x08
ST_YEARS = 0x10
ST_SCRATCH = 0x20
ST_ZERO_LOAD = 0x40
ST_DEMAND = 0x80
ST_HOURLY_FORM = 0x100   # dgen_batt_curve only: the point's tariff needs the per-year hourly pass
ST_FATAL = ST_BOUNDS | ST_TARIFF | ST_YEARS | ST_SCRATCH | ST_UNIT | ST_DEMAND

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f64 = ctypes.c_double


class Cfg(ctypes.Structure):
    _fields_ = [
        ("skip_demand_charges", _i32), ("force_net_billing", _i32),
        ("nm_yearend_sell_rate", _f64), ("loan_rate_pct", _f64), ("insurance_rate_pct", _f64),
        ("itc_fed_max", _f64), ("depr_sl_years", _i32), ("pad0", _i32),
        ("batt_v_nom", _f64), ("batt_q_full", _f64), ("batt_min_soc", _f64),
        ("batt_max_soc", _f64), ("batt_init_soc", _f64), ("batt_eta_in", _f64),
        ("batt_eta_out", _f64), ("batt_update_hours", _i32), ("batt_loss_model", _i32),
        ("batt_r_cell", _f64), ("batt_conv_eff", _f64), ("batt_v_cell_empty", _f64),
        ("batt_v_cell_full", _f64), ("batt_month_floor", _i32), ("pad1", _i32),
    ]


class Tables(ctypes.Structure):
    _fields_ = [
        ("shapes", _vp), ("shape_sum", _vp), ("shape_slots", _vp),
        ("cfs", _vp), ("cf_naep", _vp), ("cf_slots", _vp),
        ("wholesale", _vp), ("tariffs", _vp), ("switches", _vp),
        ("n_shapes", _i64), ("n_cfs", _i64), ("n_wholesale", _i64), ("n_switches", _i64),
        ("n_tariffs", _i32), ("max_periods", _i32),
        ("demand", _vp), ("n_demand", _i32), ("peak_units", _i32),
        ("max_dc_periods", _i32), ("no_net", _i32), ("pad_t", _i32),
        ("bt_tariff", _vp), ("bt_shape_max", _vp), ("bt_cf_max", _vp), ("bt_ts_max", _vp),
    ]


AGENT_COLUMNS = [
    # (name, numpy dtype)
    ("load_row", "int32"), ("cf_row", "int32"), ("wholesale_row", "int32"), ("tariff0", "int32"),
    ("sw_solar_off", "int32"), ("sw_solar_cnt", "int32"), ("sw_storage_off", "int32"),
    ("sw_storage_cnt", "int32"), ("scratch_slot", "int32"), ("flags", "uint8"),
    ("econ_life", "int32"), ("loan_term", "int32"), ("load_kwh", "float64"),
    ("price_mult", "float64"), ("inflation", "float64"), ("pv_deg", "float64"),
    ("escalator", "float64"), ("down_payment", "float64"), ("tax_rate", "float64"),
    ("real_discount", "float64"), ("itc_frac", "float64"), ("capex", "float64"),
    ("capex_combined", "float64"), ("batt_capex_kwh", "float64"), ("ccm", "float64"),
    ("vor", "float64"),
]


class Agents(ctypes.Structure):
    _fields_ = [(name, _vp) for name, _ in AGENT_COLUMNS] + [("max_years", _i32)]


OUTPUT_SCALARS = [
    ("system_kw", "float64"), ("x_last", "float64"), ("annual_kwh", "float64"),
    ("naep", "float64"), ("capacity_factor", "float64"), ("price_per_kwh", "float64"),
    ("npv", "float64"), ("payback_raw", "float64"), ("payback_period", "float64"),
    ("first_with", "float64"), ("first_without", "float64"), ("batt_kw", "float64"),
    ("batt_kwh", "float64"), ("npv_pv_batt", "float64"), ("nfev", "int32"),
    ("tariff_final", "int32"), ("switched", "int32"), ("status", "int32"),
]
OUTPUT_YEARLY = ["cash_flow", "cfev_pv", "bill_w_pv", "bill_wo_pv", "cfev_batt", "bill_w_batt",
                 "bill_wo_batt"]
OUTPUT_HOURLY = ["baseline", "net_pvonly", "net_with_batt"]


class Outputs(ctypes.Structure):
    _fields_ = ([(name, _vp) for name, _ in OUTPUT_SCALARS]
                + [(name, _vp) for name in OUTPUT_YEARLY]
                + [(name, _vp) for name in OUTPUT_HOURLY]
                + [("hourly_f64", ctypes.c_int32), ("pad_", ctypes.c_int32)])


DIGEST_F64 = ["import_kwh", "export_kwh", "peak_import_kw", "peak_export_kw"]
DIGEST_I32 = ["peak_import_hour", "peak_export_hour"]
DIGEST_FIELDS = DIGEST_F64 + DIGEST_I32


class DigestOut(ctypes.Structure):
    """dgen_digest_out: [12][n] month-major device planes, any may be NULL."""
    _fields_ = [(name, _vp) for name in DIGEST_FIELDS]


CURVE_F64 = ["npv", "payback_raw", "first_with", "first_without", "total_cost"]
CURVE_I32 = ["tariff", "switched", "status"]
CURVE_FIELDS = CURVE_F64 + CURVE_I32
CURVE_MAX_POINTS = 64   # include/dgen_hip.h dgen_objective_curve: 1 <= K <= 64


class CurveOut(ctypes.Structure):
    """dgen_curve_out: [K][n] point-major device planes, any may be NULL."""
    _fields_ = [(name, _vp) for name in CURVE_FIELDS]


BATT_SUMMARY_F64 = ["pv_kwh", "surplus_kwh", "pv_to_batt_kwh", "pv_to_grid_kwh", "pv_to_load_kwh",
                    "batt_to_load_kwh", "grid_to_load_kwh", "surplus_mid_kwh", "pv_to_batt_mid_kwh",
                    "pv_to_grid_mid_kwh", "soc_min", "soc_max", "soc_end"]
BATT_SUMMARY_I32 = ["hours_charge", "hours_discharge", "hours_soc_bound", "hours_power_bound", "hours_empty",
                    "hours_discharge_power_bound"]
BATT_SUMMARY_FIELDS = BATT_SUMMARY_F64 + BATT_SUMMARY_I32
BATT_SUMMARY_MIDDAY = (11, 15)   # include/dgen_hip.h dgen_batt_summary: the window of a NULL opt


class BattSummaryOpt(ctypes.Structure):
    """dgen_batt_summary_opt: the midday window, hours of day, inclusive."""
    _fields_ = [("mid_lo", _i32), ("mid_hi", _i32)]


class BattSummaryOut(ctypes.Structure):
    """dgen_batt_summary_out: [12][n] month-major device planes, any may be NULL."""
    _fields_ = [(name, _vp) for name in BATT_SUMMARY_FIELDS]


BILL_FIELDS = ["energy_charge", "export_credit", "fixed_charge", "demand_flat", "demand_tou", "total", "carry",
               "import_kwh", "export_kwh", "billed_kwh", "peak_kw"]


REPLAY_PLANES = ["baseline", "pvonly", "with_batt"]   # include/dgen_hip.h dgen_replay_planes


class ReplayPlanes(ctypes.Structure):
    """dgen_replay_planes: hour-quad tiled [NH / 4][n][4] device planes (any may be NULL), float32 or
    float64 (f64 = 1)."""
    _fields_ = [(name, _vp) for name in REPLAY_PLANES] + [("f64", _i32), ("pad", _i32)]


class BillOpt(ctypes.Structure):
    """dgen_bill_opt: battery = 1 bills the scan's peak-shaving dispatch at the given kW."""
    _fields_ = [("battery", _i32), ("pad", _i32)]


class BillOut(ctypes.Structure):
    """dgen_bill_out: [12][n] month-major float64 device planes (any may be NULL) and status [n] int32."""
    _fields_ = [(name, _vp) for name in BILL_FIELDS] + [("status", _vp)]


BATT_CURVE_F64 = ["npv", "payback_raw", "total_cost", "bank_kwh", "power_kw", "bill_w_year1", "bill_wo_year1",
                  "lifetime_savings"]
BATT_CURVE_I32 = ["tariff", "switched", "status"]
BATT_CURVE_FIELDS = BATT_CURVE_F64 + BATT_CURVE_I32
BATT_CURVE_MAX_POINTS = 16   # include/dgen_hip.h DGEN_BATT_CURVE_MAX_POINTS


class BattCurveOut(ctypes.Structure):
    """dgen_batt_curve_out: [K][n] point-major device planes, any may be NULL."""
    _fields_ = [(name, _vp) for name in BATT_CURVE_FIELDS]


NB_CAPM = 192   # include/dgen_hip.h DGEN_NB_CAPM


class BattNetOpt(ctypes.Structure):
    """dgen_batt_net_opt: cap = the mixed hours a month's list holds per point (<= 0: NB_CAPM)."""
    _fields_ = [("cap", _i32), ("pad", _i32)]


BATT_PEAK_CAPM_MAX = NB_CAPM   # dgen_batt_peak_opt.cap_mixed: default and maximum (dgen_batt_curve_net's cap)
BATT_PEAK_CAPK = 744           # include/dgen_hip.h DGEN_BATT_PEAK_CAPK (default kept hours per month and point)
BATT_PEAK_CAPK_MAX = 744       # include/dgen_hip.h DGEN_BATT_PEAK_CAPK_MAX


class BattPeakOpt(ctypes.Structure):
    """dgen_batt_peak_opt: cap_mixed = dgen_batt_curve_net's cap, cap_kept = the kept hours a month's
    demand record holds per point (<= 0: the defaults)."""
    _fields_ = [("cap_mixed", _i32), ("cap_kept", _i32)]


SWB_F64 = ["system_kw", "npv", "payback_raw", "total_cost", "bank_kwh", "power_kw", "bill_w_year1",
           "bill_wo_year1", "lifetime_savings"]
SWB_I32 = ["nfev", "tariff", "switched", "status"]
SWB_FIELDS = SWB_F64 + SWB_I32
SWB_TRACE_MAX = 32   # include/dgen_hip.h DGEN_SWB_TRACE_MAX


class SwbOpt(ctypes.Structure):
    """dgen_swb_opt: desired_kwh = x / pv_to_batt_ratio, desired_kw = desired_kwh / hours (<= 0: 0.8, 2.0);
    trace_n evaluations recorded per agent."""
    _fields_ = [("pv_to_batt_ratio", _f64), ("hours", _f64), ("trace_n", _i32), ("pad", _i32)]


class SwbOut(ctypes.Structure):
    """dgen_swb_out: [n] device columns (any but status may be NULL) and the [n][trace_n] traces."""
    _fields_ = [(name, _vp) for name in SWB_FIELDS] + [("trace_x", _vp), ("trace_f", _vp)]


class SwbNetOpt(ctypes.Structure):
    """dgen_swb_net_opt: cap = the mixed hours a month's list holds per agent (<= 0: NB_CAPM), max_blocks =
    the persistent blocks of the launch (<= 0: the blocks resident on the device)."""
    _fields_ = [("cap", _i32), ("max_blocks", _i32)]


class SwbPeakOpt(ctypes.Structure):
    """dgen_swb_peak_opt: cap_mixed / cap_kept = the mixed and the kept hours a month's lists hold per agent
    (<= 0: NB_CAPM, BATT_PEAK_CAPK), max_blocks = the persistent blocks of the launch (<= 0: the blocks resident
    on the device)."""
    _fields_ = [("cap_mixed", _i32), ("cap_kept", _i32), ("max_blocks", _i32), ("pad", _i32)]


TRACE_MAX = 32   # include/dgen_hip.h DGEN_TRACE_MAX
TRACE_ROWS = ["x", "f", "f_bound", "x_bound"]            # [n][TRACE_MAX] float64
TRACE_F64 = TRACE_ROWS + ["model", "system_kw"]          # model [n][4], system_kw [n]
TRACE_I32 = ["nfev", "certified", "undecided_at"]        # [n] int32
TRACE_FIELDS = TRACE_F64 + TRACE_I32


class SearchTraceOut(ctypes.Structure):
    """dgen_search_trace_out: agent-major device buffers, any may be NULL."""
    _fields_ = [(name, _vp) for name in TRACE_FIELDS]


class DgenError(RuntimeError):
    pass


_LIB: Optional[ctypes.CDLL] = None

ABI_VERSION = 14   # include/dgen_hip.h DGEN_ABI_VERSION
DEFAULT_CHUNKS = 1   # include/dgen_hip.h DGEN_DEFAULT_CHUNKS
DEFAULT_HOURLY_MONTHS = 1   # include/dgen_hip.h DGEN_DEFAULT_HOURLY_MONTHS
DEFAULT_HOURLY_SPLIT = 2   # include/dgen_hip.h DGEN_DEFAULT_HOURLY_SPLIT

EXPORTED = [
    "dgen_abi_version", "dgen_last_error", "dgen_open", "dgen_close", "dgen_prep_shapes",
    "dgen_prep_cfs", "dgen_workspace_bytes", "dgen_size_agents", "dgen_brent_selftest",
    "dgen_kernel_times", "dgen_last_paths", "dgen_set_dc_prebuild", "dgen_segment_sums", "dgen_max_market_share", "dgen_diffusion",
    "dgen_set_pipeline", "dgen_set_hourly_segment", "dgen_set_battery", "dgen_set_nb_scan", "dgen_set_ts_rows", "dgen_set_nem_rows", "dgen_set_dc_records", "dgen_set_exact", "dgen_exact_count", "dgen_hourly_planes", "dgen_export_plane", "dgen_state_hourly_rows", "dgen_batt_attach", "dgen_export_weights", "dgen_state_hourly",
    "dgen_finance_series", "dgen_year_inputs", "dgen_initial_market_shares", "dgen_rows_seq_sum",
    "dgen_plane_digest", "dgen_eval_agents", "dgen_objective_curve", "dgen_batt_summary",
    "dgen_bill_months", "dgen_batt_curve", "dgen_batt_curve_net", "dgen_batt_curve_peak",
    "dgen_size_with_batt", "dgen_size_with_batt_net", "dgen_size_with_batt_peak", "dgen_replay_at",
    "dgen_search_trace", "dgen_share_selftest",
]


def lib_path() -> str:
    # DGEN_LIB: load an alternative build (ablation / A-B timing of kernel variants)
    return os.environ.get("DGEN_LIB") or _build.OUT


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load libdgen_hip.so; build it first if it is missing and hipcc exists."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise DgenError(f"{path} is missing: run python -m dgen_amd.build")
        _build.build()
    L = ctypes.CDLL(path)
    L.dgen_abi_version.restype = _i32
    L.dgen_last_error.restype = _i32
    L.dgen_last_error.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.dgen_open.restype = _i32
    L.dgen_open.argtypes = [_i32, ctypes.POINTER(Cfg), ctypes.POINTER(_vp)]
    L.dgen_close.restype = _i32
    L.dgen_close.argtypes = [_vp]
    L.dgen_prep_shapes.restype = _i32
    L.dgen_prep_shapes.argtypes = [_vp, _vp, _i64, _vp, _vp, _vp]
    L.dgen_prep_cfs.restype = _i32
    L.dgen_prep_cfs.argtypes = [_vp, _vp, _i64, _vp, _vp, _vp]
    L.dgen_workspace_bytes.restype = ctypes.c_size_t
    L.dgen_workspace_bytes.argtypes = [_i64, _i64]
    L.dgen_size_agents.restype = _i32
    L.dgen_size_agents.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents),
                                   ctypes.POINTER(Outputs), _i64, _vp, ctypes.c_size_t, _i64, _vp]
    L.dgen_brent_selftest.restype = _i32
    L.dgen_brent_selftest.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp,
                                      _vp, _vp]
    L.dgen_share_selftest.restype = _i32
    L.dgen_share_selftest.argtypes = [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]
    L.dgen_set_dc_prebuild.restype = _i32
    L.dgen_set_dc_prebuild.argtypes = [_vp, _i32]
    L.dgen_last_paths.restype = _i32
    L.dgen_last_paths.argtypes = [_vp, ctypes.POINTER(_i32), _i32]
    L.dgen_kernel_times.restype = _i32
    L.dgen_kernel_times.argtypes = [_vp, ctypes.POINTER(_f64), ctypes.POINTER(_f64),
                                    ctypes.POINTER(_f64)]
    L.dgen_set_pipeline.restype = _i32
    L.dgen_set_pipeline.argtypes = [_vp, _i32]
    L.dgen_finance_series.restype = _i32
    L.dgen_finance_series.argtypes = [_vp, ctypes.POINTER(Outputs), _vp, _i64, _vp, _vp]
    L.dgen_set_hourly_segment.restype = _i32
    L.dgen_set_hourly_segment.argtypes = [_vp, _i32]
    L.dgen_set_battery.restype = _i32
    L.dgen_set_battery.argtypes = [_vp, _i32]
    L.dgen_set_nb_scan.restype = _i32
    L.dgen_set_nb_scan.argtypes = [_vp, _i32]
    L.dgen_set_ts_rows.restype = _i32
    L.dgen_set_ts_rows.argtypes = [_vp, _i64, _i64]
    L.dgen_set_nem_rows.restype = _i32
    L.dgen_set_nem_rows.argtypes = [_vp, _i64]
    L.dgen_set_dc_records.restype = _i32
    L.dgen_set_dc_records.argtypes = [_vp, _i32]
    L.dgen_set_exact.restype = _i32
    L.dgen_set_exact.argtypes = [_vp, _i32]
    L.dgen_exact_count.restype = _i32
    L.dgen_exact_count.argtypes = [_vp, ctypes.POINTER(ctypes.c_int64)]
    L.dgen_hourly_planes.restype = _i32
    L.dgen_hourly_planes.argtypes = L.dgen_size_agents.argtypes
    L.dgen_export_plane.restype = _i32
    L.dgen_export_plane.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                    _vp, _vp, _vp, _vp, _i64, _vp, ctypes.c_size_t, _i64, _vp]
    L.dgen_state_hourly_rows.restype = _i32
    L.dgen_state_hourly_rows.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                         _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]
    L.dgen_segment_sums.restype = _i32
    L.dgen_segment_sums.argtypes = [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _i64, _vp, _vp]
    L.dgen_rows_seq_sum.restype = _i32
    L.dgen_rows_seq_sum.argtypes = [_vp, _vp, _i64, _vp, _i64, _vp, _vp]
    L.dgen_plane_digest.restype = _i32
    L.dgen_plane_digest.argtypes = [_vp, _vp, _i32, _i64, ctypes.POINTER(DigestOut), _vp]
    L.dgen_eval_agents.restype = _i32
    L.dgen_eval_agents.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents),
                                   ctypes.POINTER(Outputs), _vp, _i64, _vp, ctypes.c_size_t, _i64, _vp]
    L.dgen_objective_curve.restype = _i32
    L.dgen_objective_curve.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), _vp, _i32, _i64,
                                       ctypes.POINTER(CurveOut), _vp, ctypes.c_size_t, _i64, _vp]
    L.dgen_batt_summary.restype = _i32
    L.dgen_batt_summary.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                    _i64, ctypes.POINTER(BattSummaryOpt), ctypes.POINTER(BattSummaryOut), _vp]
    L.dgen_bill_months.restype = _i32
    L.dgen_bill_months.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), _vp, _vp, _i64,
                                   ctypes.POINTER(BillOpt), ctypes.POINTER(BillOut), _vp]
    L.dgen_batt_curve.restype = _i32
    L.dgen_batt_curve.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                  _i64, _i32, _vp, _vp, ctypes.POINTER(BattCurveOut), _vp]
    L.dgen_batt_curve_net.restype = _i32
    L.dgen_batt_curve_net.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                      _i64, _i32, _vp, _vp, ctypes.POINTER(BattNetOpt),
                                      ctypes.POINTER(BattCurveOut), _vp]
    L.dgen_batt_curve_peak.restype = _i32
    L.dgen_batt_curve_peak.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                       _i64, _i32, _vp, _vp, ctypes.POINTER(BattPeakOpt),
                                       ctypes.POINTER(BattCurveOut), _vp]
    L.dgen_size_with_batt.restype = _i32
    L.dgen_size_with_batt.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), _i64, _vp, _vp,
                                      ctypes.POINTER(SwbOpt), ctypes.POINTER(SwbOut), _vp]
    L.dgen_size_with_batt_net.restype = _i32
    L.dgen_size_with_batt_net.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), _i64, _vp, _vp,
                                          ctypes.POINTER(SwbOpt), ctypes.POINTER(SwbNetOpt), ctypes.POINTER(SwbOut),
                                          _vp]
    L.dgen_size_with_batt_peak.restype = _i32
    L.dgen_size_with_batt_peak.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), _i64, _vp, _vp,
                                           ctypes.POINTER(SwbOpt), ctypes.POINTER(SwbPeakOpt), ctypes.POINTER(SwbOut),
                                           _vp]
    L.dgen_replay_at.restype = _i32
    L.dgen_replay_at.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), _vp, _vp, _vp, _i64,
                                 ctypes.POINTER(BattSummaryOpt), ctypes.POINTER(BattSummaryOut),
                                 ctypes.POINTER(ReplayPlanes), _vp, _vp, _vp, _vp]
    L.dgen_search_trace.restype = _i32
    L.dgen_search_trace.argtypes = [_vp, ctypes.POINTER(Tables), ctypes.POINTER(Agents), ctypes.POINTER(Outputs),
                                    _i64, ctypes.POINTER(SearchTraceOut), _vp]
    if L.dgen_abi_version() != ABI_VERSION:
        raise DgenError("libdgen_hip.so ABI version mismatch")
    _LIB = L
    return L


def last_error() -> str:
    buf = ctypes.create_string_buffer(512)
    load().dgen_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise DgenError(f"{what} failed ({rc}): {last_error()}")
    return rc
