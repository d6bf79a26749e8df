/*
 * dgen_hip.h -- C-ABI of libdgen_hip.so, the MI355X (gfx950) sizing & economics
 * engine that replaces dGen's per-agent hot path.
 *
 * Reference interface replaced (tsgsteele/dgen @ 2025-09-19, /root/reference):
 *   financial_functions.calc_system_size_and_performance   dgen_os/python/financial_functions.py:291-568
 *   financial_functions.calc_system_performance (objective) dgen_os/python/financial_functions.py:96-288
 *   financial_functions.size_chunk (worker loop)            dgen_os/python/financial_functions.py:1136-1218
 *   agent_mutation.elec.get_and_apply_agent_load_profiles   dgen_os/python/agent_mutation/elec.py:508-532
 *   agent_mutation.elec.get_and_apply_normalized_hourly_resource_solar  elec.py:535-558
 *   agent_mutation.elec.apply_rate_switch                    dgen_os/python/agent_mutation/elec.py:838-863
 *   PySAM Utilityrate5 / Cashloan / Battery .execute()       financial_functions.py:164,270,287
 *   scipy.optimize.minimize_scalar(method='bounded')         financial_functions.py:445-447
 *
 * Conventions
 *   - Plain C types only; every pointer in dgen_tables / dgen_agents /
 *     dgen_outputs is a DEVICE pointer owned by the caller (the Python host keeps
 *     them in torch-ROCm tensors) and borrowed for the duration of a call.
 *   - Every entry point returns 0 on success or a negative DGEN_E_* code; the
 *     message is available from dgen_last_error().  No exception crosses the ABI.
 *   - Per-agent problems are reported in dgen_outputs.status (DGEN_ST_* bits);
 *     the host raises like the reference's abort-the-year behaviour
 *     (dgen_model.py:382).
 *   - Calls are stream-ordered on the given hipStream_t (NULL = default stream)
 *     and asynchronous unless stated otherwise.
 *   - Yearly array outputs are agent-major: value (agent, y) at
 *     [agent * (DGEN_MAXY + 1) + y]; hourly outputs are time-major in
 *     hour-quad tiles: (hour, agent) at [((hour / 4) * n + agent) * 4 + hour % 4]
 *     (a [2190][n][4] array: each agent's 4 consecutive hours are 16 B, so a
 *     wave writes 1 KB contiguous per plane every 4 hours).
 */
#ifndef DGEN_HIP_H
#define DGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGEN_ABI_VERSION 14
#define DGEN_DEFAULT_CHUNKS 1  /* dgen_size_agents pipeline depth (dgen_set_pipeline) */
#define DGEN_DEFAULT_HOURLY_MONTHS 1  /* months per k_hourly_batt launch (dgen_set_hourly_segment) */
#define DGEN_DEFAULT_HOURLY_SPLIT 2   /* parts of a chunk's hourly scan, each on its own stream */
#define DGEN_NH    8760   /* hours per year                                    */
#define DGEN_NSLOT 576    /* 12 months x {weekday, weekend} x 24 hours         */
#define DGEN_MAXP  12     /* TOU periods                                        */
#define DGEN_MAXT  6      /* tiers                                              */
#define DGEN_MAXY  50     /* analysis years                                     */
#define DGEN_DCP   8      /* demand-charge TOU periods (extension mode)         */
#define DGEN_DCR_CAP 1024 /* kept hours per battery-case demand record          */
#define DGEN_DCT   4      /* demand-charge tiers (extension mode)               */

/* error codes */
#define DGEN_OK            0
#define DGEN_E_ARG        -1
#define DGEN_E_HIP        -2
#define DGEN_E_UNSUPPORTED -3

/* per-agent status bits */
#define DGEN_ST_BOUNDS       0x01  /* non-finite Brent bracket (scipy raises)       */
#define DGEN_ST_TARIFF       0x02  /* tariff index out of range / malformed          */
#define DGEN_ST_EMPTY_EC     0x04  /* tariff has no energy-charge matrix              */
#define DGEN_ST_UNIT         0x08  /* unsupported usage unit code (1, 3)              */
#define DGEN_ST_YEARS        0x10  /* analysis period outside 1..DGEN_MAXY            */
#define DGEN_ST_SCRATCH      0x20  /* mo=2 battery run without a scratch slot         */
#define DGEN_ST_ZERO_LOAD    0x40  /* load_kwh == 0: reference divides by zero (ff:549)*/
#define DGEN_ST_DEMAND       0x80  /* demand-charge mat outside SSC's / the record's   */
                                   /* limits (month, period, tier numbering)          */
#define DGEN_ST_HOURLY_FORM  0x100 /* dgen_batt_curve and dgen_size_with_batt only:    */
                                   /* the point's tariff bills hourly imports, demand  */
                                   /* charges or kWh/kW tiers, which they do not cover. */
                                   /* After the _net / _peak fill-ins of the curve, or  */
                                   /* dgen_size_with_batt_net / _peak: see their text   */

/* Engine configuration: the PySAM config defaults the reference never sets
 * (CustomGenerationBattery{Residential,Commercial}, ff:59-80) plus the
 * reference's module switches (ff:35,38).                                     */
typedef struct {
    int32_t skip_demand_charges;   /* 1 = the reference (ff:35 SKIP_DEMAND_CHARGES  */
                                   /* = True): tariffs' demand records are ignored; */
                                   /* 0 = extension mode: they are billed           */
    int32_t force_net_billing;     /* ff:38; applied by the host tariff compiler    */
    double  nm_yearend_sell_rate;  /* $/kWh, Utilityrate5 ur_nm_yearend_sell_rate  */
    double  loan_rate_pct;         /* Cashloan loan_rate (%)                        */
    double  insurance_rate_pct;    /* Cashloan insurance_rate (%)                   */
    double  itc_fed_max;           /* Cashloan itc_fed_percent_maxvalue ($)         */
    int32_t depr_sl_years;         /* straight-line depreciation years (type 2)     */
    int32_t pad0;
    double  batt_v_nom;            /* Li-ion cell nominal voltage (V)               */
    double  batt_q_full;           /* cell capacity (Ah)                            */
    double  batt_min_soc;          /* fraction                                      */
    double  batt_max_soc;          /* fraction                                      */
    double  batt_init_soc;         /* fraction (ff:151: 30 %)                       */
    double  batt_eta_in;           /* AC -> stored                                  */
    double  batt_eta_out;          /* stored -> AC                                  */
    int32_t batt_update_hours;     /* peak-shaving re-plan interval: 24 = one 24-h  */
                                   /* plan per calendar day (SSC's BTM peak-shaving */
                                   /* update), 1 = a 24-h look-ahead plan every     */
                                   /* hour (bdh:86-87 read literally); DESIGN.md 3  */
    int32_t batt_loss_model;       /* 0: constant efficiencies batt_eta_in / _out   */
                                   /* (default); 1: Li-ion loss model (ABI 9):      */
                                   /* converters batt_conv_eff each way + cell I^2 R */
                                   /* with an open-circuit voltage linear in SOC     */
                                   /* (parameters are guesses)  */
    double  batt_r_cell;           /* cell internal resistance (ohm)                */
    double  batt_conv_eff;         /* AC-DC and DC-AC converter efficiency          */
    double  batt_v_cell_empty;     /* cell open-circuit voltage at SOC 0 (V)        */
    double  batt_v_cell_full;      /* cell open-circuit voltage at SOC 1 (V)        */
    int32_t batt_month_floor;      /* 1: a plan's target never falls below the     */
                                   /* month's earlier targets (SSC's monthly peak-  */
                                   /* shaving target, as we read it; ABI 9); 0: off */
    int32_t pad1;
} dgen_cfg;

/* Compiled tariff = the Utilityrate5.ElectricityRates energy fields that
 * process_tariff (ff:575-648) writes, after normalize_tariff (ff:962-1007).
 * Built on the host, bit-exact to the reference compile (tests/golden).      */
typedef struct {
    int32_t P, T;                  /* periods, tiers                               */
    int32_t mo;                    /* ur_metering_option (0 or 2)                  */
    int32_t unit;                  /* usage unit code: 0 kWh/mo, 1 kWh/kW, 2 kWh    */
                                   /* daily, 3 kWh/kW daily (ff:778-779, one code   */
                                   /* per tariff, ff:939-956); 1 and 3 scale the tier*/
                                   /* caps by the month's peak import (kW), which the*/
                                   /* kernels take from the record `dc` points to    */
                                   /* (its flat peak; a zero-charge one-period record*/
                                   /* when the tariff has no demand charges)         */
    double  fixed;                 /* ur_monthly_fixed_charge ($/month)            */
    double  cap[DGEN_MAXT];        /* tier upper bounds (single cap per tier)      */
    double  buy[DGEN_MAXP][DGEN_MAXT];
    double  sell[DGEN_MAXP][DGEN_MAXT];
    uint8_t wkday[12][24];         /* 0-based period per (month, hour)             */
    uint8_t wkend[12][24];
    int32_t flags;                 /* DGEN_ST_EMPTY_EC / _UNIT / _DEMAND if so      */
    int32_t dc;                    /* 1 + index into dgen_tables.demand; 0 = none  */
                                   /* (charges billed in extension mode only; the   */
                                   /* peaks of units 1 / 3 are read in both modes)  */
} dgen_tariff;

/* Demand charges of one tariff (extension mode): the ur_dc_flat_mat /
 * ur_dc_tou_mat / ur_dc_sched_* fields process_tariff writes when
 * SKIP_DEMAND_CHARGES is off (ff:604-615), packed on the host.  Per month the
 * flat peak is the max hourly grid import (kW = kWh per hour; 0 without
 * import) and each TOU peak the max over that period's hours; each peak is
 * billed through its tier table (tier upper bounds in kW, the last tier
 * unbounded above), escalated with the energy charges.  SSC semantics
 * restated from SAM's published methodology: parity unpinned.                */
typedef struct {
    int32_t tou_nt[DGEN_DCP];      /* tiers per TOU period (0 = no charge)          */
    int32_t flat_nt[12];           /* tiers per month (0 = no charge)               */
    int32_t flags;                 /* DGEN_ST_DEMAND when the mats were out of range*/
    int32_t pad;
    double  tou_cap[DGEN_DCP][DGEN_DCT];
    double  tou_price[DGEN_DCP][DGEN_DCT];   /* $/kW                              */
    double  flat_cap[12][DGEN_DCT];
    double  flat_price[12][DGEN_DCT];
    uint8_t wkday[12][24];         /* 0-based demand period per (month, hour)       */
    uint8_t wkend[12][24];
} dgen_demand;

/* One row of diffusion_shared.rate_switch_lkup_2020 (elec.py:828-836), already
 * filtered to one agent's (tech, eia_id, res_com) on the host.                */
typedef struct {
    double  min_kw, max_kw, one_time_charge;
    int32_t tariff;                /* index into dgen_tables.tariffs                */
    int32_t pad;
} dgen_switch;

/* Resident tables (device pointers). */
typedef struct {
    const float*   shapes;         /* [n_shapes][8760] kwh_load_profile rows        */
    const double*  shape_sum;      /* [n_shapes]   np.sum of the row (numpy order)  */
    const double*  shape_slots;    /* [n_shapes][576] slot sums of the row          */
    const int32_t* cfs;            /* [n_cfs][8760] solar cf x 1e6                  */
    const double*  cf_naep;        /* [n_cfs]      np.sum(cf / 1e6)                 */
    const double*  cf_slots;       /* [n_cfs][576] slot sums of cf / 1e6            */
    const double*  wholesale;      /* [n_wholesale][8760] $/kWh (may be NULL)       */
    const dgen_tariff* tariffs;
    const dgen_switch* switches;
    int64_t n_shapes, n_cfs, n_wholesale, n_switches;
    int32_t n_tariffs;
    int32_t max_periods;           /* max P over tariffs (sizes LDS; 0 = DGEN_MAXP) */
    const dgen_demand* demand;     /* [n_demand] (may be NULL when n_demand == 0)   */
    int32_t n_demand;
    int32_t peak_units;            /* 1: some tariff bills its tiers in kWh/kW (unit */
                                   /* codes 1, 3): the year-lane kernels keep month  */
                                   /* peaks per lane (see dgen_tariff.unit)          */
    int32_t max_dc_periods;        /* 1 + the largest period in the demand records' */
                                   /* schedules (sizes LDS; 0 = DGEN_DCP)           */
    int32_t no_net;                /* 1: no agent of the call can bill net hourly   */
                                   /* (metering options 2, 3: initial tariff and    */
                                   /* every rate-switch candidate): the demand-     */
                                   /* charge kernels run their instantiations       */
                                   /* without the net-billing paths (fewer          */
                                   /* registers); 0: some may (ABI 12)              */
    int32_t pad_t;
    /* Bounds of the certified Brent paths (ABI 14, dgen_set_exact; each may be   */
    /* NULL: the agents that would need it take the exact re-run instead):        */
    const double*  bt_tariff;      /* [n_tariffs][3]: max |buy|, |sell| ($/kWh);   */
                                   /* demand prices, max over months of the flat   */
                                   /* tier price + the TOU periods' ($/kW); the     */
                                   /* kWh/kW tier caps' peak sensitivity ($/kW)     */
    const double*  bt_shape_max;   /* [n_shapes] max |shape| of the row             */
    const double*  bt_cf_max;      /* [n_cfs]    max |cf| of the row (x 1e6)        */
    const double*  bt_ts_max;      /* [n_wholesale] max |wholesale| of the row      */
} dgen_tables;

/* Agent batch, structure of arrays (device pointers, length n).  Column
 * meaning follows the agent row read by the reference. */
typedef struct {
    const int32_t* load_row;       /* row of shapes  <- (bldg_id, sector, state)     */
    const int32_t* cf_row;         /* row of cfs     <- (gid, tilt, azimuth)         */
    const int32_t* wholesale_row;  /* row of wholesale or -1 (no finite 8760 series) */
    const int32_t* tariff0;        /* initial tariff (tariff_dict)                   */
    const int32_t* sw_solar_off;   /* rate-switch candidates, tech = 'solar'          */
    const int32_t* sw_solar_cnt;
    const int32_t* sw_storage_off; /* rate-switch candidates, tech = 'storage'        */
    const int32_t* sw_storage_cnt;
    const int32_t* scratch_slot;   /* hourly scratch slot for mo=2 or demand-charge   */
                                   /* battery runs, or -1                             */
    const uint8_t* flags;          /* bit0 sector_abbr == 'res', bit1 state == 'CA'  */
    const int32_t* econ_life;      /* economic_lifetime_yrs                           */
    const int32_t* loan_term;      /* loan_term_yrs                                   */
    const double* load_kwh;        /* load_kwh_per_customer_in_bin                    */
    const double* price_mult;      /* elec_price_multiplier                           */
    const double* inflation;       /* inflation_rate (fraction)                       */
    const double* pv_deg;          /* pv_degradation_factor                           */
    const double* escalator;       /* elec_price_escalator                            */
    const double* down_payment;    /* down_payment_fraction                           */
    const double* tax_rate;        /* tax_rate                                        */
    const double* real_discount;   /* real_discount_rate                              */
    const double* itc_frac;        /* itc_fraction_of_capex                           */
    const double* capex;           /* system_capex_per_kw                             */
    const double* capex_combined;  /* system_capex_per_kw_combined                    */
    const double* batt_capex_kwh;  /* batt_capex_per_kwh_combined                     */
    const double* ccm;             /* cap_cost_multiplier                             */
    const double* vor;             /* value_of_resiliency_usd                         */
    int32_t max_years;             /* max econ_life over the batch: <= 32 runs two    */
                                   /* agents per wave in the year-lane kernels; 0 or  */
                                   /* > 32 runs one (agents above 32 lanes then fail  */
                                   /* with DGEN_ST_YEARS instead of being truncated)  */
} dgen_agents;

/* Outputs (device pointers).  Hourly planes may be NULL (on-device reduction
 * mode: nothing hourly is materialised).                                     */
typedef struct {
    double* system_kw;             /* res.x                                           */
    double* x_last;                /* last evaluated x (source of PV-only outputs)    */
    double* annual_kwh;            /* annual_energy_production_kwh                    */
    double* naep;                  /* annual / max(system_kw, 1e-9)                   */
    double* capacity_factor;
    double* price_per_kwh;
    double* npv;
    double* payback_raw;           /* Cashloan payback                                */
    double* payback_period;        /* np.round(payback if finite else 30.1, 1)        */
    double* first_with;            /* utility_bill_w_sys_year1                        */
    double* first_without;         /* utility_bill_wo_sys_year1                       */
    double* batt_kw;               /* batt_power_discharge_max_kwdc                   */
    double* batt_kwh;              /* batt_bank_installed_capacity                    */
    double* npv_pv_batt;           /* NPV of the PV+battery run (not in the ref row)  */
    int32_t* nfev;                 /* PV-only objective evaluations                   */
    int32_t* tariff_final;         /* sticky tariff state after both runs             */
    int32_t* switched;             /* any rate switch happened (nem limit -> 1e6)     */
    int32_t* status;               /* DGEN_ST_* bits                                  */
    double* cash_flow;             /* [n][MAXY+1] cf_payback_with_expenses            */
    double* cfev_pv;               /* [n][MAXY+1] cf_energy_value_pv_only             */
    double* bill_w_pv;             /* [n][MAXY+1] utility_bill_w_sys_pv_only          */
    double* bill_wo_pv;            /* [n][MAXY+1] utility_bill_wo_sys_pv_only         */
    double* cfev_batt;             /* [n][MAXY+1] cf_energy_value_pv_batt             */
    double* bill_w_batt;           /* [n][MAXY+1] utility_bill_w_sys_pv_batt          */
    double* bill_wo_batt;          /* [n][MAXY+1] utility_bill_wo_sys_pv_batt         */
    void*   baseline;              /* [2190][n][4] baseline_net_hourly (may be NULL)  */
    void*   net_pvonly;            /* [2190][n][4] adopter_net_hourly_pvonly          */
    void*   net_with_batt;         /* [2190][n][4] adopter_net_hourly_with_batt       */
    int32_t hourly_f64;            /* plane element type: 0 float (default), 1 double */
                                   /* (the reference's fp64 lists, bit-for-bit the    */
                                   /* values the kernels compute; 2 x the bytes)      */
    int32_t pad_;
} dgen_outputs;

typedef struct dgen_ctx dgen_ctx;

/* Version / build info. */
int32_t dgen_abi_version(void);

/* Copy the last error message of this thread into buf (NUL-terminated). */
int32_t dgen_last_error(char* buf, size_t n);

/* Open an engine on HIP device `device` with configuration `cfg`. */
int32_t dgen_open(int32_t device, const dgen_cfg* cfg, dgen_ctx** out);
int32_t dgen_close(dgen_ctx* ctx);

/* Profile-table preparation (replaces the per-agent SQL fetch + scaling of
 * elec.py:508-558, done once per table load instead of once per agent):
 * row sums in numpy's exact pairwise order and 576 slot sums per row.        */
int32_t dgen_prep_shapes(dgen_ctx* ctx, const float* shapes, int64_t n_rows, double* row_sum,
                         double* row_slots, void* stream);
int32_t dgen_prep_cfs(dgen_ctx* ctx, const int32_t* cfs, int64_t n_rows, double* row_naep,
                      double* row_slots, void* stream);

/* Workspace bytes for a batch of n agents with n_scratch scratch slots (agents
 * whose tariffs can bill net or carry demand charges):
 *   8 x (4 x 144 n + n + 8760 n_scratch)   bins, carries, battery output plane
 *   + DGEN_NB_BYTES x n_scratch             net-billing split records (k_size,
 *                                           k_batt_finance): per (month, period)
 *                                           4 f64 sums, 12 counts, 12 x 192
 *                                           mixed-hour entries of 24 B       */
#define DGEN_NB_BYTES 59968
#define DGEN_NB_CAPM 192     /* mixed hours per month a net-billing split record holds */
size_t dgen_workspace_bytes(int64_t n, int64_t n_scratch);

/* Size a batch: Brent over PV kW with 25-year bills + cash flow per
 * evaluation, then one PV+battery forward run at kW*, all on device.         */
int32_t dgen_size_agents(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                         const dgen_outputs* out, int64_t n, void* workspace, size_t ws_bytes,
                         int64_t n_scratch, void* stream);

/* Test entry: the device Brent on f(x) = c2 (x - x0)^2 + c1 x per lane,
 * recording up to maxn evaluated x per lane (xs: [lane][maxn]).              */
int32_t dgen_brent_selftest(dgen_ctx* ctx, const double* lo, const double* hi,
                            const double* xatol, const double* c2, const double* x0,
                            const double* c1, int64_t n, double* xs, int32_t maxn,
                            double* xopt, int32_t* nfev, void* stream);

/* Test entry: the tiered bills' period shares u[p] / U of a month as the
 * year-lane kernels form them (one corrected reciprocal of U inside the
 * helper's operand window, the divisions outside).  Per month i: u[4 i .. 4 i + 3]
 * the four billed-kWh registers, U[i] their divisor; q the helper's shares,
 * ref the plain device quotients ([n][4] each), fast[i] 1 where the month
 * was inside the window.                                                     */
int32_t dgen_share_selftest(dgen_ctx* ctx, const double* u, const double* U, int64_t n,
                            double* q, double* ref, int32_t* fast, void* stream);

/* Deterministic weighted segmented sums over contiguous agent ranges, for the
 * per-(state, sector) totals and per-state 8760-h net sums that feed diffusion
 * (replaces size_chunk's running net_sum, ff:1173-1188, and the per-state
 * hourly export, attachment_rate_functions.py:151-206):
 *   out[s * k + j] = sum_{i in [seg_off[s], seg_off[s+1])}
 *                      w1[i] * v1[j * n + i] + w2[i] * v2[j * n + i]
 * v1/v2 are k planes of n agents (plane-major, float32 or float64 by
 * `values_f32`); v2/w2 may be NULL, w1 NULL means weight 1.  Fixed summation
 * order (256-thread strided partials + LDS tree) => run-to-run identical.     */
int32_t dgen_segment_sums(dgen_ctx* ctx, const void* v1, const double* w1, const void* v2,
                          const double* w2, int32_t values_f32, int32_t k, int64_t n,
                          const int64_t* seg_off, int64_t n_seg, double* out, void* stream);

/* Sequential sum of row segments (ABI 9): out[s * k + j] = the rows
 * r in [seg_off[s], seg_off[s+1]) of in[r * k + j] added in row order
 * (((r0 + r1) + r2) + ...).  The model-year loop forms each state's totals and
 * 8760-h rows as the sum of fixed-size member chunks' partials in chunk order
 * (dgen_amd/partition.py), so a state split across ranks sums to the same bits
 * as on one rank.  n_seg <= 65535.                                           */
int32_t dgen_rows_seq_sum(dgen_ctx* ctx, const double* in, int64_t k, const int64_t* seg_off,
                          int64_t n_seg, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Diffusion step: the per-agent arithmetic of
 *   financial_functions.calc_max_market_share      ff:1264-1310 (payback -> max market share)
 *   diffusion_functions_elec.calc_diffusion_solar   diffusion_functions_elec.py:24-156
 *     (calc_equiv_time :343-372, calc_diffusion_market_share :251-292,
 *      bass_diffusion :323-338).
 * The pandas merges (bass p/q/teq_yr1 by state x sector, table keys) stay on
 * the host; every per-agent number is computed here.
 * ---------------------------------------------------------------------- */

/* max_market_curves_to_model (metric 'payback_period', business model
 * 'host_owned') as a dense table: value(row, factor) at
 * mms[row * n_factors + (factor - factor_min)], factor = round(100 * payback)
 * on the 0.1-year grid; NaN = no curve point (left-merge miss).              */
typedef struct {
    const double* mms;
    int32_t n_rows, n_factors, factor_min, pad;
    double min_pb, max_pb;          /* clip range (min / max over the curve)    */
} dgen_mms_table;

/* payback_period_bounded, payback_period_as_factor, max_market_share.
 * mms_row: curve row of the agent's sector (-1: no curve -> NaN).            */
int32_t dgen_max_market_share(dgen_ctx* ctx, const dgen_mms_table* table, const double* payback,
                              const int32_t* mms_row, int64_t n, double* payback_bounded,
                              int64_t* factor, double* max_market_share, void* stream);

typedef struct {
    const double* max_market_share;
    const double* market_share_last_year;
    const double* bass_p;
    const double* bass_q;
    const double* teq_yr1;
    const double* developable_agent_weight;
    const double* system_kw;
    const double* system_capex_per_kw;
    const double* adopters_cum_last_year;
    const double* market_value_last_year;
    const double* system_kw_cum_last_year;
} dgen_diffusion_in;

typedef struct {
    double *mms_fix_zeros, *ratio, *bass_params_teq, *teq2, *f, *new_adopt_fraction;
    double *bass_market_share, *diffusion_market_share, *market_share, *new_market_share;
    double *new_adopters, *new_market_value, *new_system_kw, *number_of_adopters;
    double *market_value, *system_kw_cum;
} dgen_diffusion_out;

/* One Bass diffusion step for every agent (is_first_year selects teq_yr1). */
int32_t dgen_diffusion(dgen_ctx* ctx, const dgen_diffusion_in* in, const dgen_diffusion_out* out,
                       int64_t n, int32_t is_first_year, void* stream);

/* ------------------------------------------------------------------------
 * Battery attachment and the per-state hourly export:
 *   attachment_rate_functions._allocate_battery_adopters_integer  :58-138
 *   attachment_rate_functions.export_state_hourly_with_storage_mix :141-206
 * ---------------------------------------------------------------------- */
typedef struct {
    const double* new_adopters;           /* diffusion's new_adopters (float)     */
    const int64_t* aid_rank;              /* rank of str(agent_id), unique        */
    const double* batt_kw;
    const double* batt_kwh;
    const double* batt_kw_cum_last_year;
    const double* batt_kwh_cum_last_year;
} dgen_attach_in;

typedef struct {
    int64_t* added;                       /* batt_adopters_added_this_year        */
    double *new_batt_kw, *new_batt_kwh, *batt_kw_cum, *batt_kwh_cum;
} dgen_attach_out;

/* Largest-remainder allocation per group: agents of group g are
 * [seg_off[g], seg_off[g+1]) in the reference's row order (its n.sum() is
 * numpy-pairwise in that order); rate[g] = the group's storage_attachment_rate.
 * Tie-break among equal fractional parts: ascending str(agent_id) (aid_rank).
 * Replaces the per-group pandas sort (:105-129).  Integer results bit-exact. */
int32_t dgen_batt_attach(dgen_ctx* ctx, const dgen_attach_in* in, const dgen_attach_out* out,
                         const int64_t* seg_off, const double* rate, int64_t n_seg, void* stream);

/* Per-agent multipliers of the state export (:181-190): w_pvo = pvo_cum,
 * w_batt = batt_cum (integers as doubles), w_non = max(n_cust - n_adopt, 0). */
int32_t dgen_export_weights(dgen_ctx* ctx, const double* customers_in_bin,
                            const double* number_of_adopters, const double* batt_kw_cum_last_year,
                            const double* batt_kw, const int64_t* added, int64_t n, double* w_pvo,
                            double* w_batt, double* w_non, void* stream);

/* Per-state hourly net sums in MW (:179-198) from the three hourly planes
 * (planes_f32 = 1: float32 in dgen_size_agents' hour-quad tiles
 * [n_hours / 4][n][4], its hourly outputs in place, n_hours % 4 == 0;
 * 2: the same tiles in float64 (dgen_outputs.hourly_f64); 0: float64
 * [n_hours][n]; 3: dgen_export_plane's combined float64 plane in tiles, in
 * `baseline`, pvonly / with_batt / weights unused) and the per-column weights:
 * out[s * n_hours + h].  Members of state s are the plane columns
 * idx[seg_off[s] .. seg_off[s+1]) (idx NULL: columns seg_off[s] ..
 * seg_off[s+1]).  Fixed summation order (deterministic); the reference's
 * sequential iterrows sum is matched to fp64 rounding, not bit for bit.    */
int32_t dgen_state_hourly(dgen_ctx* ctx, const void* baseline, const void* pvonly,
                          const void* with_batt, int32_t planes_f32, const double* w_pvo,
                          const double* w_batt, const double* w_non, const int64_t* idx, int64_t n,
                          int32_t n_hours, const int64_t* seg_off, int64_t n_seg, double* out,
                          void* stream);

/* ------------------------------------------------------------------------
 * Per-year agent attributes: the elec.apply_* merges that
 * dgen_model.py:252-292 runs on the agent frame every model year, as device
 * gathers over per-year tables compiled on the host (dgen_amd/market.py,
 * the reference's own expressions per table row):
 *   apply_load_growth                         elec.py:398-411
 *   apply_elec_price_multiplier_and_escalator elec.py:29-82
 *   apply_pv_tech_performance / apply_pv_prices / apply_pv_plus_batt_prices
 *   apply_financial_params (financing + ITC)  elec.py:135-394
 *   apply_value_of_resiliency                 elec.py:284-314
 *   apply_wholesale_elec_prices               elec.py:608-616
 *   calculate_developable_customers_and_load  elec.py:414-423
 * A left merge that finds no row gives NaN (reals) or -1 (ints); -1 keys do
 * the same.  by_sector rows carry DGEN_YS_COLS columns in this order:       */
enum {
    DGEN_YS_CAPEX = 0,          /* system_capex_per_kw                        */
    DGEN_YS_CAPEX_COMBINED,     /* system_capex_per_kw_combined               */
    DGEN_YS_BATT_CAPEX_KWH,     /* batt_capex_per_kwh_combined                */
    DGEN_YS_PV_DEG,             /* pv_degradation_factor                      */
    DGEN_YS_ITC,                /* itc_fraction_of_capex (tech 'solar')       */
    DGEN_YS_ECON_LIFE,          /* economic_lifetime_yrs                      */
    DGEN_YS_LOAN_TERM,          /* loan_term_yrs                              */
    DGEN_YS_DOWN_PAYMENT,       /* down_payment_fraction                      */
    DGEN_YS_REAL_DISCOUNT,      /* real_discount_rate                         */
    DGEN_YS_TAX_RATE,           /* tax_rate                                   */
    DGEN_YS_COLS
};
/* by_sector_county rows: load_multiplier, elec_price_multiplier,
 * elec_price_escalator (DGEN_YC_COLS); by_state_sector: value_of_resiliency_usd. */
enum { DGEN_YC_LOAD_MULT = 0, DGEN_YC_PRICE_MULT, DGEN_YC_ESCALATOR, DGEN_YC_COLS };

typedef struct {
    const int32_t* k_sector;          /* row of by_sector (-1: none)            */
    const int32_t* k_sector_county;   /* row of by_sector_county                 */
    const int32_t* k_state_sector;    /* row of by_state_sector                  */
    const int32_t* k_county;          /* row of wholesale_row                    */
    const uint8_t* is_res;            /* sector_abbr == 'res' (load growth rule) */
    const double* load_kwh_initial;   /* load_kwh_per_customer_in_bin_initial    */
    const double* customers_initial;  /* customers_in_bin_initial                */
    const double* load_in_bin_initial;/* load_kwh_in_bin_initial                 */
} dgen_year_keys;

typedef struct {
    const double* by_sector;          /* [n_sector][DGEN_YS_COLS]                */
    const double* by_sector_county;   /* [n_sector_county][DGEN_YC_COLS]         */
    const double* by_state_sector;    /* [n_state_sector]                        */
    const int32_t* wholesale_row;     /* [n_county]: this year's wholesale row   */
    int64_t n_sector, n_sector_county, n_state_sector, n_county;
    double inflation_rate;            /* apply_financial_params' scalar          */
} dgen_year_tables;

typedef struct {                      /* the dgen_agents columns it rewrites +   */
    double *load_kwh, *price_mult, *escalator, *inflation, *pv_deg, *capex, *capex_combined;
    double *batt_capex_kwh, *itc_frac, *down_payment, *real_discount, *tax_rate, *vor;
    int32_t *econ_life, *loan_term, *wholesale_row;
    double *customers_in_bin, *load_kwh_in_bin;   /* the loop's developable weight / load */
} dgen_year_out;

int32_t dgen_year_inputs(dgen_ctx* ctx, const dgen_year_keys* keys, const dgen_year_tables* tables,
                         const dgen_year_out* out, int64_t n, void* stream);

/* First-model-year market seeding, elec.estimate_initial_market_shares
 * (elec.py:701-765): per (state, sector, tech) group the developable
 * customers (pandas' Kahan-compensated group sum, rows in frame order) and the
 * agent count, then each agent's portion of the state's starting capacities
 * (caps[g * 5 + {system_mw, batt_mw, batt_mwh, pv_systems_count,
 * batt_systems_count}], NaN when the state has no row) and the
 * *_last_year / initial_* columns, NaN -> 0 (fillna).  Group g's members are
 * rows idx[seg_off[g] .. seg_off[g+1]) in frame order.                      */
typedef struct {
    const double* developable_agent_weight;
    const double* system_capex_per_kw;
} dgen_init_in;

typedef struct {
    double *adopters_cum_last_year, *system_kw_cum_last_year, *batt_kw_cum_last_year;
    double *batt_kwh_cum_last_year, *market_share_last_year, *market_value_last_year;
    double *initial_number_of_adopters, *initial_pv_kw, *initial_batt_kw, *initial_batt_kwh;
    double *initial_market_share, *initial_market_value;
    double *developable_customers_in_state;   /* per group, [n_seg]          */
    int64_t *agent_count;                     /* per group, [n_seg]          */
} dgen_init_out;

int32_t dgen_initial_market_shares(dgen_ctx* ctx, const dgen_init_in* in, const dgen_init_out* out,
                                   const int64_t* idx, const int64_t* seg_off, const double* caps,
                                   int64_t n_seg, void* stream);

/* ------------------------------------------------------------------------
 * Finance-series export, finance_series_export.py:9-81:
 * _norm25 of the six yearly arrays the export writes per agent, in the
 * reference's column order -- cf_energy_value / utility_bill_w_sys /
 * utility_bill_wo_sys of the pv_only case, then of the pv_batt case (O's
 * cfev_pv, bill_w_pv, bill_wo_pv, cfev_batt, bill_w_batt, bill_wo_batt).
 * Entry k of agent i = O.<series>[i * (DGEN_MAXY + 1) + k] for k < list_len[i]
 * (the agent's list length, economic life + 1), 0 otherwise; first 25 entries
 * (the 26-long lists are truncated); non-finite -> 0.  out: [6][n][25] f64.
 * ---------------------------------------------------------------------- */
int32_t dgen_finance_series(dgen_ctx* ctx, const dgen_outputs* O, const int32_t* list_len, int64_t n,
                            double* out, void* stream);

/* Average per-call kernel time (ms) of the dgen_size_agents calls since the
 * previous query: k_size, k_hourly_batt, k_batt_finance, each summed over the
 * call's chunks (HIP events recorded on the stream each kernel runs on).
 * Returns the number of calls averaged (>= 0) or an error code.              */
int32_t dgen_kernel_times(dgen_ctx* ctx, double* ms_size, double* ms_hourly, double* ms_finance);

/* The record forms the last dgen_size_agents call on ctx took, as the call
 * decided them from its tables, settings and LDS limits (ABI 11): out[0] the
 * battery case's net-billing split built in the scan (dgen_set_nb_scan),
 * out[1] battery-case demand records (dgen_set_dc_records), out[2] the TS
 * sell-rate agents' own split scan, out[3] the demand machinery on (demand
 * charges billed or kWh/kW tier peaks), out[4] the period count the kernels'
 * LDS is laid out for (the tables' max_periods after the call's adjustments),
 * out[5] the demand periods per record, out[6] the demand envelopes of the
 * first-evaluation tariffs prebuilt by their own kernel (k_dc_env).  Writes
 * min(n_out, DGEN_PATHS_N) values; returns DGEN_PATHS_N.  For byte
 * accounting (bench.py); replaces nothing in the reference.                 */
#define DGEN_PATHS_N 7
int32_t dgen_last_paths(dgen_ctx* ctx, int32_t* out, int32_t n_out);

/* Demand envelopes (the PV-only search's per-(month, demand period) import
 * lines, demand-charge and kWh/kW-tier batches) of every agent's
 * first-evaluation tariff prebuilt by their own kernel ahead of the search
 * (1, default; k_dc_env: day lanes, coalesced 16-B profile loads) or built by
 * the search kernel at the first evaluation that bills the tariff (0; the
 * DGEN_DC_PREBUILD=0 environment setting at dgen_open does the same).  The
 * kept lines are the same set either way and an evaluation takes their max,
 * so results are bit-identical (ABI 11).  Replaces nothing in the reference. */
int32_t dgen_set_dc_prebuild(dgen_ctx* ctx, int32_t on);

/* Rows [0, hi) of the next dgen_size_agents batches hold only agents without a
 * scratch slot (scratch_slot < 0: bins-only billing, no net-billing or demand
 * path; engine.profile_order puts them first).  A batch that has scratch slots
 * then sizes those rows with the bins-only instantiations of k_size /
 * k_batt_finance (fewer registers, slimmer LDS) and skips them in the split
 * prebuild; results are bit-identical (the same bills on the same path).  0
 * (default): the whole batch takes the batch's form.  A row in [0, hi) that
 * does hold a scratch slot would be flagged DGEN_ST_SCRATCH, so the caller
 * must only cover true bins-only rows (ABI 13).  Replaces nothing in the
 * reference. */
int32_t dgen_set_nem_rows(dgen_ctx* ctx, int64_t hi);

/* Pipeline depth of dgen_size_agents: the batch is cut into `chunks` pieces;
 * k_size of piece j+1 runs on the caller's stream while k_hourly_batt and
 * k_batt_finance of piece j run on a context-owned second stream (forked from
 * and joined back into the caller's stream, so stream order is unchanged for
 * the caller).  1 = no overlap.  Range [1, 16]; default DGEN_DEFAULT_CHUNKS.
 * Replaces nothing in the reference (its per-agent loop is serial, ff:1149). */
int32_t dgen_set_pipeline(dgen_ctx* ctx, int32_t chunks);

/* The hourly planes of a batch already sized by dgen_size_agents (same ctx
 * settings, same tables / agents / workspace), without re-sizing it: the
 * 8760-h scan alone, re-deriving the battery run from O's sizing outputs
 * (system_kw, x_last, tariff_final, switched, status); every other output it
 * writes gets the value the sizing call wrote.  For shards whose planes do not
 * fit beside the batch (dgen_amd.year_loop's chunked per-state export): size
 * the whole shard without planes, then call this per chunk of agents with the
 * chunk's slices of O and a plane buffer.  Replaces nothing in the reference
 * (its lists come out of the one sizing call, ff:505-539).                  */
int32_t dgen_hourly_planes(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                           const dgen_outputs* outputs, int64_t n, void* workspace, size_t workspace_bytes,
                           int64_t n_scratch, void* stream);

/* The per-state export's combined plane of a batch already sized by
 * dgen_size_agents (same ctx settings, tables, agents, workspace; as
 * dgen_hourly_planes, the scan alone): per agent-hour the f64 value
 * dgen_state_hourly adds from the three float32 planes,
 *   ((double)pvo * w_pvo + (double)wbt * w_batt) + (double)base * w_non,
 * in hour-quad tiles ((h, i) at ((h / 4) * n + i) * 4 + h % 4), from the
 * weights of dgen_export_weights.  dgen_state_hourly with planes_f32 = 3 sums
 * it (baseline = the plane; pvonly / with_batt / weights unused): the same
 * per-state rows, bit for bit, from 8 B per agent-hour written and read
 * instead of 12.  Daily plan without the loss model only (DGEN_E_ARG
 * otherwise: use dgen_hourly_planes).  n < 2^27.  Replaces nothing in the
 * reference (attachment_rate_functions.py:151-206 sums the frame's lists).   */
int32_t dgen_export_plane(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                          const dgen_outputs* outputs, const double* w_pvo, const double* w_batt,
                          const double* w_non, double* plane, int64_t n, void* workspace,
                          size_t workspace_bytes, int64_t n_scratch, void* stream);

/* The per-state export from the with-battery plane alone (ABI 11): a batch
 * sized by dgen_size_agents with only outputs.net_with_batt set (float32
 * hour-quad tiles; daily plan, no loss model, no demand charges / kWh/kW
 * tiers) -- the load and PV-only net load of each agent-hour are recomputed
 * from the profile rows (agents' load_row / cf_row / load_kwh, outputs'
 * x_last / status) as the scan forms them, so out (per segment, 8760 rows,
 * MW) equals dgen_state_hourly over the three float32 planes bit for bit,
 * from 4 B of plane per agent-hour.  idx / seg_off as dgen_state_hourly.
 * Replaces nothing in the reference (attachment_rate_functions.py:151-206
 * sums the frame's hourly lists).  The per-agent scalars live in a buffer
 * the ctx owns and grows on demand (after a device-wide sync): calls on one
 * ctx must be serialised, as for every other entry point.                 */
int32_t dgen_state_hourly_rows(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                               const dgen_outputs* outputs, const float* with_batt, const double* w_pvo,
                               const double* w_batt, const double* w_non, const int64_t* idx, int64_t n,
                               const int64_t* seg_off, int64_t n_seg, double* out, void* stream);

/* Months of the year per k_hourly_batt launch (the sequential 8760-h scan of
 * dgen_size_agents): the year is swept in ceil(12 / months) launches, SOC and
 * the annual PV sum carried between them in the workspace, so that all
 * resident waves read the same weeks of the shared profile rows and those
 * slices stay cache-resident.  Results do not depend on it.  Range [1, 12];
 * default DGEN_DEFAULT_HOURLY_MONTHS.  Replaces nothing in the reference.   */
int32_t dgen_set_hourly_segment(dgen_ctx* ctx, int32_t months);

/* PV+battery forward run on (1, default: the reference, which always runs it
 * at ff:479) or off (0: the PV-only variant of SURVEY 8(d)).  Off: no battery
 * sizing, storage rate switch or dispatch (batt_kw = batt_kwh = 0, the
 * with-battery plane is the PV-only net load at kW*), k_batt_finance is not
 * launched: npv_pv_batt is NaN and the three battery-case yearly arrays are
 * left untouched.                                                          */
int32_t dgen_set_battery(dgen_ctx* ctx, int32_t on);

/* Where the battery case's net-billing split is built for agents that bill
 * net without a TS sell rate: cap > 0 (default DGEN_NB_CAPM) in
 * k_hourly_batt's scan, as the system output is produced, holding at most cap
 * mixed hours per month -- k_batt_finance then bills from the record and the
 * system-output plane is not written for agents without demand charges; an
 * agent whose split overflows gets its plane from a repair pass and is billed
 * as with 0 -- or 0: in k_batt_finance from the plane.  Results are equal up
 * to the rounding of the re-associated sums (bit-identical for an overflowing
 * agent).  The scan form pays its classification in every wave that holds
 * such an agent, so a batch where few agents qualify is faster with 0 (the
 * Python engine decides per batch: Engine.upload_agents).  Applies to
 * batches whose tariffs have at most 10 periods (the scan form's doubled
 * bins then fit 64 KB of LDS per block); others build in k_batt_finance.
 * Range [0, DGEN_NB_CAPM].  Replaces nothing in the reference.            */
int32_t dgen_set_nb_scan(dgen_ctx* ctx, int32_t cap);

/* The batch rows [lo, hi) that hold every agent able to bill the hourly TS
 * sell rate (a scratch slot and a wholesale row, non-CA): the TS agents' own
 * split scan (k_hourly_batt<TS>, batches with hourly planes and a wholesale
 * table, no demand charges) is launched over those rows only; lo == hi: none.
 * Default [0, INT64_MAX): the whole batch.  Results do not depend on it as
 * long as the range covers those agents (the Python engine sets it from the
 * device order, Engine.upload_agents).  Replaces nothing in the reference.  */
int32_t dgen_set_ts_rows(dgen_ctx* ctx, int64_t lo, int64_t hi);

/* Battery-case demand records holding at most cap kept hours per agent
 * (default and maximum DGEN_DCR_CAP), or none (0).  With demand charges
 * billed (or kWh/kW tier peaks) and the daily plan, k_hourly_batt's scan keeps
 * per (month, demand period) the max load and a lower bound of every analysis
 * year's peak import, and the hours that can raise some year's peak above it
 * (a context-owned buffer per scratch slot); k_batt_finance's battery-case
 * demand pass then stages those hours only, instead of all 8760 hours of the
 * system-output plane.  Results are bit-identical (peaks are maxima of the
 * same values).  An agent whose kept hours overflow the record falls back to
 * the plane.  Replaces nothing in the reference.                            */
int32_t dgen_set_dc_records(dgen_ctx* ctx, int32_t cap);

/* Certified Brent paths (ABI 14).  The search bills from re-associated sums
 * (slot sums, net-billing split), a few ulps from the reference's hour order,
 * and scipy's bounded Brent can turn such a difference into another search
 * path (ff:440-447).  mode 1 (default): every search traces its objective
 * values; a replay with a bound on |device - reference| carried through every
 * Brent state variable lists the agents with a decision that bound does not
 * settle, and those agents' searches re-run in the reference's arithmetic
 * (hours in time order: Utilityrate5 bins, bill, Cashloan, op for op), so every
 * agent takes the reference's path.  mode 2: every searched agent re-runs
 * (test mode).  mode 0: off (k_size's search alone).  Replaces nothing in the
 * reference (its one path is the hour-order one).                            */
int32_t dgen_set_exact(dgen_ctx* ctx, int32_t mode);

/* Agents the last dgen_size_agents call re-ran in the reference's arithmetic
 * (synchronises the ctx's stream work of that call).                         */
int32_t dgen_exact_count(dgen_ctx* ctx, int64_t* out);

/* Search trace and certificate audit of the sizing call (additive to ABI 14).
 * Lays open the fast search of the last dgen_size_agents call on this ctx
 * (modes 1 and 2 trace it; the trace lives in the ctx until the next sizing or
 * evaluation call).  tables, agents, outputs and n are that call's, as
 * dgen_hourly_planes takes them; run it on that call's stream, or after it.
 * Per agent i, with K = DGEN_TRACE_MAX:
 *   x, f        the evaluations of the fast search in order: scipy's bounded
 *               Brent run again over the traced objective values from the
 *               bracket and xatol of ff:440-444, so x[i][k] are the search's
 *               own bits; NaN beyond nfev.
 *   nfev,       of that replayed search -- not of `outputs`, which hold the
 *   system_kw   reference-arithmetic re-run's values for the agents mode 1 / 2
 *               re-ran.  A search that asks for evaluation K is truncated: nfev
 *               = K + 1, system_kw NaN, certified 0, the first K rows filled.
 *   model       c0, c1, ce, lip of the certificate's error model: at the same
 *               x, |f_device - f_reference| <= c0 + c1 |x| + ce |f|, and
 *               |f(x) - f(x')| <= lip |x - x'| between rate-switch thresholds.
 *   f_bound,    evaluation k's bound of |f_device - f_reference| (the model at
 *   x_bound     x[k] plus lip x x_bound[k]) and of |x_device - x_reference|, as
 *               the certificate carried them to that evaluation.  Rows from
 *               undecided_at on are NaN.
 *   certified   1: every decision of the search is the reference's under the
 *               bound (mode 1 keeps the fast search's path); 0: not settled
 *               (mode 1 re-runs the agent) -- also for a model that is not
 *               finite, a missing bound table, or a switch row outside the
 *               tariff table; -1: no search.  The mode-1 decision whatever
 *               mode the ctx is in.
 *   undecided_at  evaluations taken when the certificate stopped at a decision
 *               the bound does not settle (nfev: only the closing test of the
 *               reported x's failed; 0: no usable model); -1 if certified.
 * No search -- outputs.status carries DGEN_ST_BOUNDS, _TARIFF, _UNIT or
 * _YEARS, or outputs.nfev is 0: certified -1, nfev 0, undecided_at -1, NaN
 * elsewhere.  One lane per agent, no atomics: agent i's rows do not depend on
 * n, its neighbours or the chunk pipeline.  DGEN_E_ARG when the last sizing /
 * evaluation call on the ctx recorded no trace (mode 0, dgen_eval_agents, no
 * call yet), when n is not that call's, or when out is NULL.  Replaces nothing
 * in the reference (scipy's search keeps no trace).                          */
#define DGEN_TRACE_MAX 32                 /* evaluations traced per search */
typedef struct {                          /* any member may be NULL: not written */
    double  *x, *f;                       /* [n][DGEN_TRACE_MAX] agent-major; NaN beyond nfev */
    double  *f_bound, *x_bound;           /* [n][DGEN_TRACE_MAX] */
    double  *model;                       /* [n][4]: c0, c1, ce, lip */
    double  *system_kw;                   /* [n] */
    int32_t *nfev;                        /* [n] */
    int32_t *certified;                   /* [n]: 1, 0, -1 */
    int32_t *undecided_at;                /* [n] */
} dgen_search_trace_out;

int32_t dgen_search_trace(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                          const dgen_outputs* out, int64_t n, const dgen_search_trace_out* trace,
                          void* stream);

/* Per-agent monthly grid-exchange digest of one hourly plane (additive to
 * ABI 14).  `plane` is one of dgen_size_agents' hourly planes in its hour-quad
 * tiles ((h, i) at ((h / 4) * n + i) * 4 + h % 4; float, or double when
 * plane_f64 is set; DGEN_NH hours).  For agent i and calendar month m (hours
 * [h0, h1) of the non-leap year, the scan's month table), in hour order:
 *   imp = exp = pk_i = pk_e = 0.0;  hr_i = hr_e = -1
 *   v = (double)plane[h, i]
 *   if v > 0:      imp += v;   if  v > pk_i: pk_i =  v, hr_i = h
 *   else if v < 0: exp += -v;  if -v > pk_e: pk_e = -v, hr_e = h
 * fp64 sums, strictly sequential in hour order; the first hour wins a tie; a
 * NaN hour fails both comparisons and adds nothing.  One lane per (agent,
 * month), no atomics and no cross-lane traffic: run-to-run identical.  The
 * outputs are month-major [12][n] -- the k = 12 plane-major planes
 * dgen_segment_sums takes.  A NULL member is not written.  Replaces nothing in
 * the reference (it drops the hourly lists before agent_outputs,
 * dgen_model.py:441-458, and derives no per-agent grid exchange).            */
typedef struct {            /* each [12][n], month-major: value (m, i) at [m * n + i]; any may be NULL */
    double  *import_kwh, *export_kwh, *peak_import_kw, *peak_export_kw;
    int32_t *peak_import_hour, *peak_export_hour;   /* hour of year 0..8759, -1 = none */
} dgen_digest_out;

int32_t dgen_plane_digest(dgen_ctx* ctx, const void* plane, int32_t plane_f64, int64_t n,
                          const dgen_digest_out* out, void* stream);

/* Evaluate a batch at caller-given sizes (additive to ABI 14):
 * dgen_size_agents with the bounded Brent search replaced by one evaluation of
 * its objective, calc_system_performance(kw[i], en_batt=False) from the agent's
 * initial tariff state (tariff0, not switched), then the same PV+battery
 * forward run at kw[i].  `kw` is [n] doubles on the device, in the batch's row
 * order.  Outputs as dgen_size_agents writes them with system_kw = x_last =
 * kw[i] bit for bit and nfev = 1; a size that is not finite or not positive
 * (0 is not supported: the net-billing split and the demand envelopes
 * degenerate there) gets DGEN_ST_BOUNDS, nfev 0 and NaN outputs.  Argument
 * checks, plane forms, the chunk pipeline, the dgen_set_battery / _pipeline /
 * _hourly_segment / _nb_scan / _dc_records / _ts_rows / _nem_rows settings and
 * the dgen_kernel_times accounting (the evaluation in the k_size slot) are
 * dgen_size_agents'; dgen_hourly_planes, dgen_export_plane and
 * dgen_state_hourly_rows take its outputs as they take a sizing call's.
 * dgen_set_exact does not apply: there is no search path to certify, nothing
 * of that machinery is allocated or launched and a following
 * dgen_exact_count reports 0.  dgen_set_dc_prebuild does not apply either: the
 * split and the envelopes cover the evaluated size's generation range, not the
 * bracket's, and are built inside the evaluation (dgen_last_paths out[6] is
 * 0).  Replaces nothing in the reference (its only way to the objective is the
 * search, ff:440-447).                                                        */
int32_t dgen_eval_agents(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                         const dgen_outputs* out, const double* kw, int64_t n, void* workspace,
                         size_t ws_bytes, int64_t n_scratch, void* stream);

/* The PV-only objective at K sizes per agent (additive to ABI 14).  xs is
 * [K][n] doubles on the device, point-major (point k of agent i at
 * xs[k * n + i]), 1 <= K <= 64.  Every point is evaluated on its own from the
 * agent's initial tariff state, as dgen_eval_agents does, so column k equals a
 * dgen_eval_agents call at xs[k] bit for bit on the shared members; the rate
 * switch's stickiness does not carry from one point to the next.  A point that
 * is not finite or not positive gets DGEN_ST_BOUNDS in `status` and NaN, and
 * leaves the agent's other points as they are.  Launches the evaluation kernel
 * alone: no dgen_outputs, no hourly scan, no battery run, no kernel-time
 * record.  Table and agent-column checks and the workspace are
 * dgen_size_agents'.  A NULL member is not written.                          */
typedef struct {            /* each [K][n], point-major; any may be NULL */
    double  *npv, *payback_raw, *first_with, *first_without, *total_cost;
    int32_t *tariff, *switched, *status;
} dgen_curve_out;

int32_t dgen_objective_curve(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                             const double* xs, int32_t K, int64_t n, const dgen_curve_out* out,
                             void* workspace, size_t ws_bytes, int64_t n_scratch, void* stream);

/* Per-agent monthly battery dispatch summary (additive to ABI 14): a replay of
 * the hourly scan's peak-shaving dispatch for a batch dgen_size_agents or
 * dgen_eval_agents already sized (`out`: its system_kw and status are read),
 * as dgen_hourly_planes replays it, but no plane is stored: the state of charge
 * and the hour's flows are reduced per calendar month.  One lane per agent, the
 * year in hour order (SOC carries from month to month).  Per agent i:
 *   ls  = load_kwh / shape_sum[load_row]
 *   kW* = system_kw (0 for a DGEN_ST_UNIT agent, as in the scan)
 *   cs6 = (((kW* x 1000) x 0.96) / 1000) / 1e6
 *   bank, power = battery_model_sizing(kW* / 0.8 / 2, kW* / 0.8, 240 V
 *                 residential | 500 V) as the scan sizes it; 0, 0 after
 *                 dgen_set_battery(0) or for a bank that is not positive
 *   soc = batt_init_soc
 * and for every hour h of the non-leap year, in order:
 *   ld = (double)shape[h] x ls;  pv = (double)cf[h] x cs6;  nn = ld - pv
 *   at h % 24 == 0: target = the day's peak-shaving target (the scan's plan
 *       over the day's max(nn, 0) with the energy available at this SOC,
 *       raised to the month's largest earlier target with batt_month_floor)
 *   room  = max((batt_max_soc - soc) x bank / batt_eta_in, 0)
 *   avail = max((soc - batt_min_soc) x bank x batt_eta_out, 0)
 *   sur = max(-nn, 0)
 *   cc  = min(min(-nn, power), room)                   if nn < 0, else 0
 *   dd  = min(min(max(nn - target, 0), power), avail)  if nn >= 0, else 0
 *   soc, g2l = the scan's hour (soc += cc x eta_in / bank or -= dd / (eta_out
 *       x bank); g2l = 0 charging, nn - dd otherwise): the same device
 *       function, so g2l is the with-battery plane's value bit for bit
 * Members, over the hours of month m in hour order (fp64 sequential sums):
 *   pv_kwh            sum pv
 *   surplus_kwh       sum sur
 *   pv_to_batt_kwh    sum cc
 *   pv_to_grid_kwh    sum (sur - cc)
 *   pv_to_load_kwh    sum min(ld, pv)
 *   batt_to_load_kwh  sum dd
 *   grid_to_load_kwh  sum g2l
 *   surplus_mid_kwh, pv_to_batt_mid_kwh, pv_to_grid_mid_kwh
 *                     the same three sums over the hours with
 *                     mid_lo <= h % 24 <= mid_hi (default 11, 15)
 *   soc_min, soc_max  min / max of the end-of-hour SOC (a fraction of the bank)
 *   soc_end           the SOC after the month's last hour
 *   hours_charge, hours_discharge    #(cc > 0), #(dd > 0)
 *   hours_soc_bound   #(sur > 1e-6 and soc >= batt_max_soc - 1e-9)
 *   hours_power_bound #(sur > power + 1e-6 and soc < batt_max_soc - 1e-9)
 *   hours_empty       #(nn > 1e-6 and soc <= batt_min_soc + 1e-9)
 *   hours_discharge_power_bound   #(dd > power x (1 - 1e-9) and power > 0)
 * with soc the end-of-hour value in the four counts; 1e-6 (kW) and 1e-9 (SOC)
 * are part of the definition, not tolerances.  Peak shaving never discharges
 * to the grid (the battery's flow is capped by the hour's net load), so there
 * is no battery-to-grid member, and pv_to_load + batt_to_load + grid_to_load
 * is the month's load.  An agent flagged DGEN_ST_BOUNDS, _TARIFF or _YEARS
 * gets 0 in every member.  Without a bank every flow is 0, the SOC members are
 * batt_init_soc and grid_to_load is sum max(nn, 0).  Each member is
 * month-major [12][n] (value (m, i) at [m * n + i]: the k = 12 plane-major
 * planes dgen_segment_sums takes); a NULL member is not written.  No atomics
 * and no cross-lane traffic: run-to-run identical.  Table and agent-column
 * checks are dgen_hourly_planes'; no workspace.  The daily plan under the
 * constant efficiencies only: batt_update_hours == 1 or batt_loss_model == 1
 * returns DGEN_E_ARG, as does a window with mid_lo > mid_hi or outside 0..23.
 * The reference's counterpart is batt_dispatch_helpers.dispatch_export_diags,
 * one agent at a time from PySAM's hourly arrays: its soc_bound_all and
 * power_bound_all are the two charge-side counts, with the explicit 1e-9 band
 * on the SOC fraction in place of its exact >= 95.0.                        */
typedef struct { int32_t mid_lo, mid_hi; } dgen_batt_summary_opt;   /* NULL: 11, 15 */

typedef struct {            /* each [12][n], month-major; any may be NULL */
    double  *pv_kwh, *surplus_kwh, *pv_to_batt_kwh, *pv_to_grid_kwh, *pv_to_load_kwh,
            *batt_to_load_kwh, *grid_to_load_kwh, *surplus_mid_kwh, *pv_to_batt_mid_kwh,
            *pv_to_grid_mid_kwh, *soc_min, *soc_max, *soc_end;
    int32_t *hours_charge, *hours_discharge, *hours_soc_bound, *hours_power_bound, *hours_empty,
            *hours_discharge_power_bound;
} dgen_batt_summary_out;

int32_t dgen_batt_summary(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                          const dgen_outputs* out, int64_t n, const dgen_batt_summary_opt* opt,
                          const dgen_batt_summary_out* summary, void* stream);

/* Year-1 monthly bill breakdown per agent (additive to ABI 14): "bill agent i
 * at kw[i] kW under tariff[i]", month by month -- the year-1 bill of the
 * oracle (oracle/orc.c: bin_year, month_energy_charge, year_bill, year_demand,
 * dc_tier_charge) at degradation factor 1 and escalation factor 1, with every
 * ingredient the year-lane kernels reduce to one scalar.  kw: [n] device
 * doubles, 0 is valid (the no-system bill); tariff: [n] device int32 indices
 * into tables->tariffs, the caller's choice (not necessarily the agent's own:
 * the what-if bill under any tariff of the table).  A replay from the profile
 * rows, as dgen_batt_summary is: no dgen_outputs, no plane, no workspace.
 * One lane per agent, the year in hour order.  Per agent i:
 *   ls  = load_kwh / shape_sum[load_row]
 *   cs6 = (((kw x 1000) x 0.96) / 1000) / 1e6
 * and for every hour h of the non-leap year, in order:
 *   ld = (double)shape[h] x ls;  pv = (double)cf[h] x cs6
 *   g  = pv                                       (opt NULL or battery = 0)
 *   g  = pv + f  with battery = 1: the system output of the scan's
 *        peak-shaving dispatch at this kw (bank and power from kw / 0.8 / 2,
 *        kw / 0.8 as dgen_batt_summary sizes them; the day's plan, the month
 *        floor and the hour's step are the scan's own device functions on
 *        ld - pv, f = -cc charging, dd discharging: the value k_hourly_batt
 *        stores in its system-output scratch plane, bit for bit); the bank
 *        is 0 (g = pv) after dgen_set_battery(0) or when it is not positive
 *   d  = ld - g
 * Calendar: the year starts on a Monday, hours with (h % 168) >= 120 are
 * weekend; the hour's period p is the tariff's wkday / wkend[month][h % 24]
 * (clamped to P - 1).  Per (month, period), fp64 sequential sums in hour
 * order, all from 0:
 *   net += d;  lbin += ld;  gbin += g
 *   imp += d            when d > 0
 *   exv += (-d) x ts[h] otherwise, ts[h] = 1 without the TS sell rate
 * The TS sell rate applies when tariff.mo == 2, the agent is not CA (flags
 * bit 1), wholesale_row >= 0 (the column and price_mult given) and
 * tables->wholesale != NULL; then
 *   ts[h] = (double)(float)(wholesale[h] x price_mult).
 * Per month: peak = max over its hours of d, 0 without import; export_kwh =
 * the sequential sum of max(-d, 0) (kWh, also under TS).  Demand charges are
 * on when cfg.skip_demand_charges == 0 and tariff.dc names a record (1 ..
 * n_demand); then the peak of demand period q is the max of d (0 without
 * import) over the hours the record's wkday / wkend put in q.
 * Then the 12 months in order, with credit[p] (kWh, mo 0) and carry ($, mo 1
 * and 3) starting at 0 and living across the months, exactly as year_bill:
 *   mo 0  per p ascending: net >= 0: use = min(net, credit[p]), u[p] = net -
 *         use, credit[p] -= use; else u[p] = 0, credit[p] += -net.
 *         bill = fixed + E(u); December: bill -= (sum_p credit[p]) x
 *         nm_yearend_sell_rate
 *   mo 1  u[p] = max(net, 0); cr = sum_p max(-net, 0) x sell[p][0];
 *         e = E(u) - cr - carry; carry = max(-e, 0); bill = fixed + max(e, 0)
 *   mo 4  u[p] = lbin; cr = sum_p gbin x sell[p][0]; bill = fixed + (E(u) - cr)
 *   mo 2, 3 (and any other value)  u[p] = imp; cr = sum_p exv (TS) or
 *         sum_p exv x sell[p][0]; mo 3: e, carry and bill as mo 1;
 *         else bill = (fixed + E(u)) - cr
 * E(u) = month_energy_charge: U = sum_p u[p]; 0 unless U > 0; one tier:
 * sum_p u[p] x buy[p][0]; else over tiers k ascending, hi = cap[k] x scale
 * (infinite for the last tier; scale 1, days (unit 2), peak (unit 1) or peak x
 * days (unit 3)), amt = max(min(U, hi) - prev, 0), prev = max(prev, hi), and
 * per p ascending the charge grows by ((u[p] / U) x amt) x buy[p][k].
 * Members, each [12][n] month-major (value (m, i) at [m x n + i]):
 *   energy_charge  E(u)
 *   export_credit  cr of mo 1 to 4; mo 0: 0, except December's
 *                  (sum_p credit[p]) x nm_yearend_sell_rate
 *   fixed_charge   tariff.fixed
 *   demand_flat    dc_tier_charge of `peak` over the record's month tiers
 *   demand_tou     sum over q ascending of dc_tier_charge of period q's peak;
 *                  both 0 when demand charges are off
 *   total          (bill + demand_flat) + demand_tou.  For mo 1 and 3 the bill
 *                  carries the floor at 0: energy_charge - export_credit -
 *                  (the carry before the month) may be negative, and
 *                  total = fixed + max(that, 0) + demand
 *   carry          after the month: sum_p credit[p] in kWh (mo 0; December's
 *                  is the bank the true-up pays out), the carried dollars
 *                  (mo 1, 3), 0 otherwise
 *   import_kwh     sum_p imp
 *   export_kwh     as above
 *   billed_kwh     U
 *   peak_kw        peak
 * Every sum over periods and over tiers runs in ascending order, and a x b + c
 * stays two roundings (the library is built with -ffp-contract=off).
 * status[i] ([n], required): 0, or DGEN_ST_TARIFF for an index outside
 * 0 .. n_tariffs - 1 (or a tariff whose P exceeds tables->max_periods), the
 * tariff's own flags (DGEN_ST_EMPTY_EC, _UNIT, _DEMAND; _DEMAND also for a
 * demand schedule beyond tables->max_dc_periods), DGEN_ST_BOUNDS for a kw that
 * is not finite or is negative; DGEN_ST_YEARS does not apply.  An agent with a
 * non-zero status gets NaN in every double member.  A NULL member is not
 * written.  No atomics and no cross-lane sums: run-to-run identical.  Table
 * and agent-column checks are dgen_batt_summary's.  battery = 1 under
 * batt_update_hours == 1 or batt_loss_model == 1 returns DGEN_E_ARG.
 * Utilityrate5's counterparts are its year1_monthly_* and charge_w_sys_*_ym
 * outputs, which the reference drops.                                       */
typedef struct { int32_t battery; int32_t pad; } dgen_bill_opt;      /* NULL: battery = 0 */

typedef struct {   /* each [12][n] month-major, any may be NULL, except status [n] */
    double *energy_charge, *export_credit, *fixed_charge, *demand_flat, *demand_tou, *total,
           *carry, *import_kwh, *export_kwh, *billed_kwh, *peak_kw;
    int32_t *status;
} dgen_bill_out;

int32_t dgen_bill_months(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                         const double* kw, const int32_t* tariff, int64_t n, const dgen_bill_opt* opt,
                         const dgen_bill_out* out, void* stream);

/* Battery size what-if (additive to ABI 14): the with-battery economics of a
 * batch dgen_size_agents or dgen_eval_agents already sized (`sized`: its
 * system_kw, tariff_final, switched and status are read, nothing is written) at
 * K caller-given banks per agent.  A point is one more
 * calc_system_performance(kW*, en_batt=True) on the agent as the sizing call
 * left it (oracle/orc.c, the PV+battery run of size_agent_impl) with the
 * battery's desired kWh and kW supplied instead of kW* / 0.8 and kW* / 0.8 / 2.
 * kwh: [K][n] device doubles, point-major (point k of agent i at [k x n + i]);
 * kw_pts: [K][n] or NULL (then desired_kw = desired_kwh / 2.0, the reference's
 * 2-hour bank).  One lane per (agent, point); per point, with kW* = system_kw:
 *   bank, power = battery_model_sizing(desired_kw, desired_kwh, 240 V
 *       residential | 500 V) as the scan sizes it (a positive desired_kwh below
 *       half a string still buys one string); 0, 0 for desired_kwh = 0 (a valid
 *       point: no bank) and after dgen_set_battery(0)
 *   dispatch: dgen_batt_summary's replay (ls, cs6 at kW*, the day's plan, the
 *       month floor, the scan's hour) -> the system output sys[h]
 *   storage rate switch, when bank > 0: exactly one of the agent's sw_storage
 *       rows with min_kw <= bank < max_kw moves the point to that row's tariff
 *       (switched = 1, otc = its one-time charge); otherwise the point keeps
 *       the tariff_final and switched it was handed and otc = 0 (the sticky,
 *       in-place semantics of elec.py:838-863)
 *   bins, per (month, period) of that tariff's energy schedule, fp64
 *       sequential in hour order: lbin = sum ld, gbin = sum sys
 *   years y = 1 .. N (economic life): s_y = (1 - pv_deg)^(y-1), r_y = (1 +
 *       inflation + escalator)^(y-1), sequential products; bill_w[y] = r_y x
 *       year_bill at net bins lbin - s_y x gbin (mo 4: load lbin, generation
 *       s_y x gbin), bill_wo[y] = r_y x year_bill at lbin alone (year_bill and
 *       month_energy_charge as under dgen_bill_months, fixed charge and the
 *       December true-up included); aev[y] = (bill_wo[y] - bill_w[y]) + vor
 *   cost = ((kW* > 0 ? capex_combined : capex) x kW* + batt_capex_kwh x bank x
 *       0.7) x ccm + otc
 *   Cashloan as the sizing call's (loan_inputs, orc_cashloan); payback_raw by
 *       its chain (1e99: none); npv = atcf[0] + sum_y atcf[y] x rr^y added in
 *       year order with rr^y a running product (the oracle's Horner chain to
 *       rounding)
 * Members, each [K][n] point-major, any may be NULL (a NULL member is not
 * written): npv, payback_raw, total_cost (cost), bank_kwh, power_kw,
 * bill_w_year1, bill_wo_year1, lifetime_savings (sum of aev[y], y = 1 .. N, in
 * year order), tariff and switched (after the switch), status.
 * Covered: tariffs that bill from bins -- metering options 0, 1 and 4, tier
 * units 0 and 2, no demand charge billed.  A point whose tariff after the
 * switch bills hourly imports (options 2, 3), carries billed demand charges or
 * has kWh/kW tier units gets DGEN_ST_HOURLY_FORM, as does every point of a
 * DGEN_ST_UNIT agent.  A point whose kwh is not finite or is negative, or whose
 * kw_pts is not finite or not positive while kwh > 0, gets DGEN_ST_BOUNDS.  An
 * agent the sizing call flagged DGEN_ST_BOUNDS, _TARIFF or _YEARS keeps that
 * status in every point.  A switch to an index outside the table, or to a
 * tariff beyond tables->max_periods, gets DGEN_ST_TARIFF.  Every double member
 * of such a point is NaN; other points carry the agent's informational bits
 * (DGEN_ST_EMPTY_EC, _ZERO_LOAD, _DEMAND) or 0.  Points are independent:
 * column k of a K-point call is the K = 1 call at that point bit for bit.  No
 * atomics and no cross-lane sums: run-to-run identical.  No workspace.
 * 1 <= K <= DGEN_BATT_CURVE_MAX_POINTS, else DGEN_E_ARG; batt_update_hours == 1
 * or batt_loss_model == 1 returns DGEN_E_ARG, as in dgen_batt_summary.  The
 * kernel keeps 26 x max_periods x 512 B of LDS per 64 points.                 */
#define DGEN_BATT_CURVE_MAX_POINTS 16

typedef struct {            /* each [K][n], point-major; any may be NULL */
    double  *npv, *payback_raw, *total_cost, *bank_kwh, *power_kw,
            *bill_w_year1, *bill_wo_year1, *lifetime_savings;   /* sum_y aev[y], y = 1..N */
    int32_t *tariff, *switched, *status;
} dgen_batt_curve_out;

int32_t dgen_batt_curve(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                        const dgen_outputs* sized, int64_t n, int32_t K, const double* kwh,
                        const double* kw_pts, const dgen_batt_curve_out* out, void* stream);

/* Battery size what-if under net billing (additive to ABI 14): the points
 * dgen_batt_curve leaves flagged DGEN_ST_HOURLY_FORM because their tariff
 * bills hourly imports -- metering options 2 and 3, with the period sell rate
 * or the hourly TS sell rate.  Arguments, layouts, the K range, the output
 * struct and every DGEN_E_ARG case are dgen_batt_curve's.  The entry fills in:
 * called after dgen_batt_curve on the same buffers and stream it overwrites
 * exactly the points it covers and writes nothing else, so what stays flagged
 * DGEN_ST_HOURLY_FORM is kWh/kW tier units, billed demand charges and
 * overflow (below).  A covered point: the agent is sized (no DGEN_ST_BOUNDS,
 * _TARIFF, _YEARS, _UNIT), kwh and kw_pts are valid as in dgen_batt_curve, the
 * tariff after the storage rate switch is in range and within
 * tables->max_periods, its metering option is 2 or 3, its tier unit 0 or 2,
 * and no demand charge is billed.  Every other point -- bins-form tariffs
 * included -- is not written at all, members and status alike.
 * Per covered point: bank, power, dispatch replay -> sys[h], storage switch
 * (sticky on the tariff_final / switched handed in), cost and Cashloan (the
 * forward-sum NPV) are dgen_batt_curve's.  The bills are orc_ur5's hourly
 * form: for year y = 1 .. N with s_y, r_y the sequential products, per
 * (month, period) in hour order
 *     d = ld[h] - s_y x sys[h];  imp += d when d > 0, else exv += (-d) x ts[h]
 * with ts[h] = 1 without the TS rate; the month's bill is
 *     mo 2: (fixed + E(imp)) - cr          mo 3: fixed + max(E(imp) - cr - carry, 0),
 *           carry = max(-(E(imp) - cr - carry), 0) to the next month (lost at year end)
 * E = month_energy_charge (as under dgen_bill_months), cr = sum_p exv[p] x
 * sell[p][0], or sum_p exv[p] under the TS rate; bill_w[y] = r_y x the twelve
 * months' sum; the no-system year bills imp = lbin with cr = 0.  The TS rate
 * applies exactly as in dgen_bill_months: mo 2, not CA, wholesale_row >= 0,
 * tables->wholesale non-NULL, ts[h] = (double)(float)(wholesale[h] x
 * price_mult).
 * The kernel re-associates the hourly sums as the scan's battery-case split
 * does: over the agent's degradation range [s_N, 1] an hour importing at both
 * ends (above -1e-10 x (|ld| + |sys| x s_hi): a near-zero battery hour counts
 * as an import) adds ld and sys to two sums per (month, period), an hour
 * exporting at both ends adds sys x ts and ld x ts to two more, and any other
 * hour joins the month's mixed list, evaluated per year in hour order.  Results
 * equal the hourly order to rounding, not bit for bit.
 * opt->cap: the mixed hours a month's list holds per point, 1 ..
 * DGEN_NB_CAPM (NULL or cap <= 0: DGEN_NB_CAPM; above it: DGEN_E_ARG).  A point
 * with a month beyond cap is not written (overflow): it keeps what the buffers
 * held, DGEN_ST_HOURLY_FORM after dgen_batt_curve.  Nothing is stored past cap.
 * The lists live in a ctx-owned workspace sized by the blocks resident on the
 * device (a persistent, grid-stride launch), not by K x n: per block 51,200 B
 * of per-year accumulators and cap x 1024 B of entries, grown on demand and
 * freed by dgen_close; calls on one ctx must be stream-ordered.  Points are
 * independent (column k of a K-point call is the K = 1 call bit for bit), no
 * atomics and no cross-lane sums: run-to-run identical.  The kernel keeps 7 x
 * max_periods x 512 B of LDS per 64 points.                                   */
typedef struct { int32_t cap; int32_t pad; } dgen_batt_net_opt;   /* NULL or cap <= 0: DGEN_NB_CAPM */

int32_t dgen_batt_curve_net(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                            const dgen_outputs* sized, int64_t n, int32_t K, const double* kwh,
                            const double* kw_pts, const dgen_batt_net_opt* opt,
                            const dgen_batt_curve_out* out, void* stream);

/* Battery size what-if with month peaks (additive to ABI 14): the points the
 * two entries above leave flagged DGEN_ST_HOURLY_FORM because their tariff
 * bills demand charges or has kWh/kW tier units (codes 1, 3), under every
 * metering option.  Arguments, layouts, the K range, the output struct and
 * every DGEN_E_ARG case are dgen_batt_curve_net's.  The entry fills in: called
 * after dgen_batt_curve (and dgen_batt_curve_net, in either order) on the same
 * buffers and stream it overwrites exactly the points it covers and writes
 * nothing else, members and status alike.  A covered point: the agent is sized
 * (no DGEN_ST_BOUNDS, _TARIFF, _YEARS, _UNIT), kwh and kw_pts are valid as in
 * dgen_batt_curve, the tariff after the storage rate switch is in range and
 * within tables->max_periods, and that tariff has tier unit 1 or 3 or demand
 * charges are billed for it (cfg.skip_demand_charges == 0 and tariff.dc names
 * a record in 1 .. n_demand).  Not written, so still flagged: a point whose
 * tariff or demand record carries DGEN_ST_DEMAND, one whose demand schedule
 * names a period at or beyond tables->max_dc_periods, and overflow (below).
 * After the three calls DGEN_ST_HOURLY_FORM means a DGEN_ST_UNIT agent, a
 * malformed demand table or list overflow.
 * Per covered point: bank, power, dispatch replay -> sys[h], storage switch
 * (sticky on the tariff_final / switched handed in), cost and Cashloan (the
 * forward-sum NPV) are dgen_batt_curve's.  The bills are orc_ur5's with peaks:
 * for year y = 1 .. N with s_y, r_y the sequential products, month m, demand
 * period q (the record's schedule; one period when a kWh/kW tariff has no
 * record)
 *     peak_y[m][q] = max(0, max over the hours of (m, q) of ld[h] - s_y x sys[h])
 *     flat_y[m]    = max_q peak_y[m][q]
 * E(u, peak) = month_energy_charge with the tier caps x flat_y[m] (unit 1) or
 * x flat_y[m] x days (unit 3).  The month's energy side is dgen_batt_curve's
 * for metering options 0, 1 and 4 (from the month's bins at lbin - s_y x gbin)
 * and dgen_batt_curve_net's for options 2 and 3 (hourly imports and exports,
 * the TS rate as there, re-associated by its linear-sums / mixed-list rule
 * with the same 1e-10 slack: equal to the hourly order to rounding).  The
 * month's demand charge, when billed, is dc_tier_charge(flat_y[m], the
 * month's flat tiers), then + dc_tier_charge(peak_y[m][q], period q's tiers)
 * for q ascending.  Each year keeps two running sums in month order and adds
 * them once: bill_w[y] = r_y x (sum_m energy bill + sum_m demand charge); the
 * no-system year bills ld alone, its peaks the (m, q) maxima of the load.
 * The peaks come from a per-point demand record, built per month by the
 * scan's rule over [s_lo, s_hi] = [s_N, 1]: per (m, q) the running
 * lb = max_h min(d(s_lo), d(s_hi)) and, in hour order, the hours whose
 * max(d(s_lo), d(s_hi)) exceeds lb as it stood before them, compacted at the
 * month's end against the final lb.  fl(ld - fl(sys x s)) is monotone in s, so
 * a dropped hour is at or below an earlier hour in every year and lb is at or
 * below every year's peak: each year's peak over the kept hours, started from
 * lb, is its peak over all hours bit for bit.
 * opt->cap_mixed: dgen_batt_curve_net's cap (default and maximum
 * DGEN_NB_CAPM); opt->cap_kept: the kept hours a month's list holds per point
 * before compaction, 1 .. DGEN_BATT_PEAK_CAPK_MAX (a month's 744 hours: no
 * overflow), default DGEN_BATT_PEAK_CAPK, the maximum as well: a bank that
 * covers the whole load leaves lb at 0 and keeps nearly every hour (DESIGN.md
 * section 5).  NULL or a value <= 0: the default; above the maximum:
 * DGEN_E_ARG.  A point with a month beyond either cap is
 * not written; nothing is stored past a cap.  The lists and the per-year state
 * (energy total, demand total, dollar carry, and the kWh credit bank per
 * period of option 0, for the no-system year and N years) live in a ctx-owned
 * workspace sized by the blocks resident on the device (a persistent,
 * grid-stride launch), not by K x n: per block 26,112 x (3 + max_periods) B
 * of per-year state and (cap_mixed + cap_kept) x 1024 B of entries, grown on
 * demand and freed by dgen_close; calls on one ctx must be stream-ordered.
 * Points are independent (column k of a K-point call is the K = 1 call bit
 * for bit), no atomics and no cross-lane sums: run-to-run identical.  The
 * kernel keeps (7 x max_periods + 3 x max_dc_periods) x 512 B of LDS per 64
 * points.                                                                     */
#define DGEN_BATT_PEAK_CAPK      744   /* default kept hours per month and point */
#define DGEN_BATT_PEAK_CAPK_MAX  744   /* a month's hours                        */
typedef struct { int32_t cap_mixed; int32_t cap_kept; } dgen_batt_peak_opt;   /* NULL or <= 0: the defaults */

int32_t dgen_batt_curve_peak(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                             const dgen_outputs* sized, int64_t n, int32_t K, const double* kwh,
                             const double* kw_pts, const dgen_batt_peak_opt* opt,
                             const dgen_batt_curve_out* out, void* stream);

/* PV sizing on the with-battery objective (additive to ABI 14): the bounded
 * scalar search of the sizing call (scipy's minimize_scalar(method='bounded'),
 * op for op) over the PV size x, minimising the reference's perf_with_batt
 *     f(x) = -npv of calc_system_performance(x, en_batt=True)
 * (financial_functions.py:427-435), whose battery is sized from x.  The
 * reference builds this objective and evaluates it once, at the PV-only
 * optimum; it never searches on it, so there is no reference path to
 * reproduce.  f is therefore defined as a function of x alone: every
 * evaluation starts from (tariff0[i], not switched), dgen_objective_curve's
 * convention, and the storage rate switch's stickiness is not carried from one
 * evaluation to the next.  A path-dependent objective could not be checked
 * point by point; this one is the dgen_batt_curve point with
 *     sized.system_kw = x, sized.tariff_final = tariff0, sized.switched = 0,
 *     kwh = x / ratio, kw_pts = (x / ratio) / hours
 * bit for bit, in every member: bank and power (battery_model_sizing),
 * dispatch replay, storage rate switch on the bank, (month, period) bins, the
 * N years' bills, cost = (capex_combined x x + batt_capex_kwh x bank x 0.7) x
 * ccm + otc, Cashloan and the forward-sum NPV, each as defined under
 * dgen_batt_curve.
 * opt: pv_to_batt_ratio (<= 0 or NaN: 0.8, ff:140), hours (<= 0 or NaN: 2.0,
 * ff:141), trace_n in 0 .. DGEN_SWB_TRACE_MAX; opt NULL: 0.8, 2.0, no trace.
 * Bracket: lo and hi are device arrays [n], both given or both NULL.  NULL:
 * the sizing call's bracket bit for bit, max_load = load_kwh / cf_naep[cf_row],
 * lo = 0.8 x max_load, hi = 1.25 x max_load (ff:440-443).  In both cases
 * xatol = max(2, floor(max(1, hi - lo) x 1e-3)) (ff:444).  A bracket that is
 * not finite, has lo <= 0 or has lo >= hi gives DGEN_ST_BOUNDS; load_kwh == 0
 * adds DGEN_ST_ZERO_LOAD as in the sizing call.
 * Members, each [n], any may be NULL except status: system_kw is the x the
 * search returns (always an evaluated point), nfev its number of evaluations;
 * npv, payback_raw, total_cost, bank_kwh, power_kw, bill_w_year1,
 * bill_wo_year1, lifetime_savings, tariff and switched are the bits of the
 * evaluation at system_kw (so npv = -min over the evaluations of f).
 * trace_x, trace_f: [n][trace_n] agent-major, evaluation k's x and f(x) for
 * k < min(nfev, trace_n), NaN beyond; either may be NULL.
 * Covered tariffs are dgen_batt_curve's: metering options 0, 1 and 4, tier
 * units 0 and 2, no demand charge billed.  Status: DGEN_ST_YEARS (economic
 * life outside 1 .. DGEN_MAXY) and DGEN_ST_TARIFF (tariff0 outside the
 * table; a switch to an index outside it or to a tariff beyond
 * tables->max_periods) as dgen_batt_curve assigns them; an agent whose tariff0
 * carries DGEN_ST_UNIT gets DGEN_ST_HOURLY_FORM without an evaluation.  When
 * the tariff after the switch of any evaluation bills hourly imports (options
 * 2, 3), bills demand charges or has kWh/kW tier units, the agent gets
 * DGEN_ST_HOURLY_FORM, tariff and switched of that evaluation, and nfev counts
 * the evaluations up to and including it: no later evaluation of that agent
 * walks the year.  Every double member of an agent with DGEN_ST_BOUNDS,
 * _TARIFF, _YEARS or _HOURLY_FORM is NaN (its trace keeps what was recorded).
 * Other agents carry DGEN_ST_ZERO_LOAD and the DGEN_ST_EMPTY_EC / _DEMAND flags
 * of tariff0 and of the tariff billed at system_kw, or 0.
 * After dgen_set_battery(ctx, 0) every bank is 0 and the search runs on the
 * PV-only bills with capex_combined.  batt_update_hours == 1 or
 * batt_loss_model == 1, trace_n out of range, one of lo / hi NULL and
 * out->status NULL return DGEN_E_ARG.  Agent i's results do not depend on n or
 * on its neighbours; no atomics, no cross-lane sums, no workspace and no
 * dgen_outputs: run-to-run identical.  One lane per agent walks the year once
 * per evaluation; the kernel keeps 26 x max_periods x 512 B of LDS per 64
 * agents.
 * dgen_size_with_batt_net (below), called next on the same buffers, searches
 * the agents this entry ends on options 2 and 3.  After both calls
 * DGEN_ST_HOURLY_FORM is left on an agent whose tariff0 carries DGEN_ST_UNIT,
 * one with an evaluation on billed demand charges or kWh/kW tier units, and
 * one whose net-billing month overflowed that entry's cap.                    */
#define DGEN_SWB_TRACE_MAX 32

typedef struct {
    double  pv_to_batt_ratio;   /* desired_kwh = x / ratio; <= 0 or NaN: 0.8 (ff:140) */
    double  hours;              /* desired_kw = desired_kwh / hours; <= 0 or NaN: 2.0 (ff:141) */
    int32_t trace_n;            /* evaluations recorded per agent, 0 .. DGEN_SWB_TRACE_MAX */
    int32_t pad;
} dgen_swb_opt;                 /* NULL: 0.8, 2.0, no trace */

typedef struct {                /* each [n]; any may be NULL except status */
    double  *system_kw, *npv, *payback_raw, *total_cost, *bank_kwh, *power_kw,
            *bill_w_year1, *bill_wo_year1, *lifetime_savings;
    int32_t *nfev, *tariff, *switched, *status;
    double  *trace_x, *trace_f; /* [n][trace_n] agent-major, unused entries NaN; may be NULL */
} dgen_swb_out;

int32_t dgen_size_with_batt(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents, int64_t n,
                            const double* lo, const double* hi, const dgen_swb_opt* opt,
                            const dgen_swb_out* out, void* stream);

/* The net-billing tariffs of that search (additive to ABI 14): the agents
 * dgen_size_with_batt ends with DGEN_ST_HOURLY_FORM because an evaluation's
 * tariff bills hourly imports -- metering options 2 and 3, with the period
 * sell rate or the hourly TS sell rate.  The entry fills in: called after
 * dgen_size_with_batt with the same lo, hi and opt on the same out buffers and
 * stream it writes its candidates in full and nothing else.  ctx, tables,
 * agents, n, lo, hi, opt, out and stream are dgen_size_with_batt's.
 * Candidates are decided from the tables and the agent columns alone (out is
 * not read).  Agent i is a candidate when all of these hold:
 *   - its bracket (lo, hi, or the default bracket when both are NULL) is valid
 *     under dgen_size_with_batt's rules, bit for bit;
 *   - its economic life is in 1 .. DGEN_MAXY;
 *   - tariff0[i] is inside the table and does not carry DGEN_ST_UNIT;
 *   - tariff0[i], or the tariff of at least one of its sw_storage rows whose
 *     index is inside the table, has metering option 2 or 3.
 * Every other agent is not written at all: no member, no status, no trace row
 * (a batch without such tariffs leaves at that check); an agent the first call
 * valued and that cannot reach net billing keeps its bits.
 * A candidate runs dgen_size_with_batt's search: the same bounded minimiser,
 * xatol by ff:444, every evaluation from (tariff0, not switched), ratio, hours
 * and trace_n from opt.  f(x) = -npv takes the form of the tariff after the
 * storage rate switch on that evaluation's bank:
 *   bins form (options 0, 1, 4; tier units 0, 2; no demand charge billed):
 *       the dgen_batt_curve point, bit for bit, as in dgen_size_with_batt;
 *   options 2 or 3, tier unit 0 or 2, no demand charge billed:
 *       the dgen_batt_curve_net point at nopt->cap, bit for bit, the TS sell
 *       rate included,
 * in both cases with sized.system_kw = x, sized.tariff_final = tariff0,
 * sized.switched = 0, kwh = x / ratio, kw_pts = kwh / hours.  One search may be
 * billed under both forms when a storage row's edge lies between the banks of
 * the bracket's ends.
 * An evaluation ends the agent when the tariff after the switch bills demand
 * charges or has kWh/kW tier units, is outside the table or beyond
 * tables->max_periods (this one adds DGEN_ST_TARIFF), or has a month with more
 * than cap mixed hours.  dgen_size_with_batt's rule for such a lane holds: NaN
 * in every double member, DGEN_ST_HOURLY_FORM, tariff and switched of that
 * evaluation, nfev up to and including it; no later request walks the year.
 * Nothing is stored past cap.
 * Every candidate is written in full by dgen_size_with_batt's rule (the
 * members of the evaluation at system_kw, nfev, the trace rows NaN beyond
 * nfev, DGEN_ST_ZERO_LOAD and the DGEN_ST_EMPTY_EC / _DEMAND flags of tariff0
 * and of the tariff billed at system_kw), so a candidate whose evaluations were
 * all of the bins form gets the bits the first call wrote.  NULL members are
 * not written; status must be given.
 * nopt->cap: the mixed hours a month's list holds per agent, 1 ..
 * DGEN_NB_CAPM (NULL or cap <= 0: DGEN_NB_CAPM; above it: DGEN_E_ARG).
 * nopt->max_blocks: a positive value caps the persistent blocks of the launch
 * and so the workspace; NULL or <= 0: the blocks resident on the device.
 * Results do not depend on it.  The lists live in dgen_batt_curve_net's
 * ctx-owned workspace, sized by the blocks, not by n: per block 51,200 B of
 * per-year accumulators and cap x 1024 B of entries (508 MB at the resident
 * count of an MI355X and the default cap), grown on demand and freed by
 * dgen_close; calls on one ctx must be stream-ordered.  One lane per
 * candidate walks the year once per evaluation; every evaluation starts its
 * lists and accumulators afresh.  Agent i's results do not depend on n, on its
 * neighbours or on the blocks; no atomics, no cross-lane traffic: run-to-run
 * identical.  The kernel keeps the larger of the two forms' layouts, 26 x
 * max_periods x 512 B of LDS per 64 agents.
 * Argument errors are dgen_size_with_batt's (trace_n out of range, one of
 * lo / hi NULL, out->status NULL, batt_update_hours == 1 or
 * batt_loss_model == 1: DGEN_E_ARG); after dgen_set_battery(ctx, 0) every bank
 * is 0 and the search runs on the PV-only hourly bills.
 * After both calls DGEN_ST_HOURLY_FORM means: tariff0 carries DGEN_ST_UNIT, an
 * evaluation met billed demand charges or kWh/kW tier units, or a month's
 * mixed list overflowed cap.                                                  */
typedef struct { int32_t cap; int32_t max_blocks; } dgen_swb_net_opt;   /* NULL or <= 0: the defaults */

int32_t dgen_size_with_batt_net(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents, int64_t n,
                                const double* lo, const double* hi, const dgen_swb_opt* opt,
                                const dgen_swb_net_opt* nopt, const dgen_swb_out* out, void* stream);

/* The demand-charge and kWh/kW tariffs of that search (additive to ABI 14):
 * the agents the two entries above end with DGEN_ST_HOURLY_FORM because an
 * evaluation's tariff is of peak form -- kWh/kW tier units (codes 1, 3), or a
 * demand charge that is billed (cfg.skip_demand_charges == 0 and the tariff's
 * dc names a record in 1 .. n_demand), under any metering option.  The entry
 * fills in with dgen_size_with_batt_net's contract: same lo, hi, opt, out
 * buffers and stream, its candidates written in full and nothing else.
 * Call it LAST: after dgen_size_with_batt, and after dgen_size_with_batt_net
 * where that one is used.  Unlike the what-if fill-ins the order matters: an
 * agent may be a candidate of both fill-ins (a net-billing tariff0 with a
 * storage row onto a demand tariff); the net entry ends it at its first
 * peak-form evaluation, this entry values it, and the last writer's bits stay.
 * Candidates are decided from the tables, cfg and the agent columns alone (out
 * is not read).  Agent i is a candidate when all of these hold:
 *   - its bracket (lo, hi, or the default bracket when both are NULL) is valid
 *     under dgen_size_with_batt's rules, bit for bit;
 *   - its economic life is in 1 .. DGEN_MAXY;
 *   - tariff0[i] is inside the table and does not carry DGEN_ST_UNIT;
 *   - tariff0[i], or the tariff of at least one of its sw_storage rows whose
 *     index is inside the table, is of peak form.
 * Every other agent is not written at all: no member, no status, no trace row
 * (a batch without such tariffs leaves at that check).
 * A candidate runs dgen_size_with_batt's search: the same bounded minimiser,
 * xatol by ff:444, every evaluation from (tariff0, not switched), ratio, hours
 * and trace_n from opt.  f(x) = -npv takes the form of the tariff after the
 * storage rate switch on that evaluation's bank:
 *   peak form (any metering option):
 *       the dgen_batt_curve_peak point at popt->cap_mixed / popt->cap_kept,
 *       bit for bit;
 *   options 2 or 3 without peaks:
 *       the dgen_batt_curve_net point at cap = popt->cap_mixed, bit for bit;
 *   bins form:
 *       the dgen_batt_curve point, bit for bit,
 * each with sized.system_kw = x, sized.tariff_final = tariff0,
 * sized.switched = 0, sized.status = 0, kwh = x / ratio, kw_pts = kwh / hours.
 * One search may cross all three forms; a candidate whose evaluations never
 * met the peak form gets the bits the earlier calls wrote, or would have
 * written.
 * An evaluation ends the agent when its tariff after the switch is outside the
 * table or beyond tables->max_periods (this one adds DGEN_ST_TARIFF), when the
 * tariff or its demand record carries DGEN_ST_DEMAND (the bit stays in the
 * status), when its demand schedule names a period at or beyond
 * tables->max_dc_periods, or when a month holds more than cap_mixed mixed or
 * cap_kept kept hours.  dgen_size_with_batt's rule for such a lane holds: NaN
 * in every double member, DGEN_ST_HOURLY_FORM, tariff and switched of that
 * evaluation, nfev up to and including it; no later request walks the year.
 * Nothing is stored past a cap.
 * Every candidate is written in full by dgen_size_with_batt's rule (the
 * members of the evaluation at system_kw, nfev, the trace rows NaN beyond
 * nfev, DGEN_ST_ZERO_LOAD and the DGEN_ST_EMPTY_EC / _DEMAND flags of tariff0
 * and of the tariff billed at system_kw).  NULL members are not written;
 * status must be given.
 * popt->cap_mixed: 1 .. DGEN_NB_CAPM, popt->cap_kept: 1 ..
 * DGEN_BATT_PEAK_CAPK_MAX (NULL or <= 0: DGEN_NB_CAPM and
 * DGEN_BATT_PEAK_CAPK; above the maximum: DGEN_E_ARG).  popt->max_blocks: a
 * positive value caps the persistent blocks of the launch and so the
 * workspace; NULL or <= 0: the blocks resident on the device.  Results do not
 * depend on it.  The lists live in dgen_batt_curve_peak's ctx-owned workspace,
 * sized by the blocks, not by n (per block (DGEN_MAXY + 1) x (3 +
 * max_periods) x 512 B of per-year state, cap_mixed x 1024 B and cap_kept x
 * 1024 B of entries), grown on demand and freed by dgen_close; calls on one
 * ctx must be stream-ordered.  The net-billing evaluations use the same slice.
 * One lane per candidate walks the year once per evaluation; every evaluation
 * starts its lists and accumulators afresh.  Agent i's results do not depend
 * on n, on its neighbours or on the blocks; no atomics, no cross-lane traffic:
 * run-to-run identical.  The kernel keeps the largest of the three forms'
 * layouts, max(26 x max_periods, 7 x max_periods + 3 x max_dc_periods) x
 * 512 B of LDS per 64 agents.
 * Argument errors are dgen_size_with_batt's (trace_n out of range, one of
 * lo / hi NULL, out->status NULL, batt_update_hours == 1 or
 * batt_loss_model == 1: DGEN_E_ARG); after dgen_set_battery(ctx, 0) every bank
 * is 0 and the search bills the PV-only peaks.
 * After the three calls DGEN_ST_HOURLY_FORM means: tariff0 carries
 * DGEN_ST_UNIT, an evaluation met a tariff or demand record flagged
 * DGEN_ST_DEMAND or a demand schedule beyond max_dc_periods, or a month's list
 * overflowed its cap.                                                         */
typedef struct { int32_t cap_mixed; int32_t cap_kept; int32_t max_blocks; int32_t pad; } dgen_swb_peak_opt;  /* NULL or <= 0: the defaults */

int32_t dgen_size_with_batt_peak(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents, int64_t n,
                                 const double* lo, const double* hi, const dgen_swb_opt* opt,
                                 const dgen_swb_peak_opt* popt, const dgen_swb_out* out, void* stream);

/* Dispatch replay at a caller-given PV size and bank (additive to ABI 14):
 * dgen_batt_summary's monthly summary and the scan's three hourly planes for
 * "agent i with kw[i] kW of PV and a battery of bank_kwh[i] kWh / bank_kw[i]
 * kW", the point a what-if call (dgen_batt_curve, dgen_size_with_batt) priced.
 * A replay from the profile rows: no dgen_outputs, no workspace, and tariff
 * state plays no part.  kw, bank_kwh: [n] device doubles; bank_kw: [n] or NULL
 * (then desired_kw = bank_kwh / 2.0, the reference's 2-hour bank, exactly as
 * in dgen_batt_curve); status: [n] device int32; all but bank_kw required.
 * bank_out, power_out: [n] device doubles, either may be NULL.  At least one
 * of `summary` and `planes` must be non-NULL.  One lane per agent, the year in
 * hour order.  Per agent i:
 *   ls  = load_kwh / shape_sum[load_row]
 *   cs6 = (((kw x 1000) x 0.96) / 1000) / 1e6
 *   bank, power = battery_model_sizing(desired_kw, bank_kwh, 240 V residential
 *                 | 500 V) as the scan sizes it (a positive bank_kwh below half
 *                 a string still buys one string); 0, 0 for bank_kwh = 0 (a
 *                 valid point: no bank) and after dgen_set_battery(0)
 *   soc = batt_init_soc
 * and for every hour h of the non-leap year, in order, dgen_batt_summary's
 * hour operation for operation: ld, pv, nn; at h % 24 == 0 the day's
 * peak-shaving target over the day's max(nn, 0) with the energy available at
 * this SOC (raised to the month's largest earlier target with
 * batt_month_floor); the scan's hour for soc and g2l; cc, dd and sur from the
 * pre-hour SOC.
 * summary: dgen_batt_summary_out's 19 members with their definitions above,
 * month-major [12][n]; a NULL member is not written; the midday window is
 * opt's (NULL: 11, 15).
 * planes: the scan's values with one size for both runs,
 *   baseline = ld;  pvonly = max(ld - pv, 0);  with_batt = g2l
 * each rounded to float when f64 == 0, in the hour-quad tiles of dgen_outputs'
 * hourly planes (the layout dgen_state_hourly and dgen_plane_digest take); a
 * NULL plane is not written.  At kw = system_kw and bank_kwh = system_kw / 0.8
 * (bank_kw NULL) the summary is dgen_batt_summary's and the planes are
 * dgen_eval_agents' at that size, bit for bit.
 * status[i]: 0, or DGEN_ST_BOUNDS when kw is not finite or is negative (kw = 0
 * is valid: no PV, the bank never charges), when bank_kwh is not finite or is
 * negative, or when bank_kw is given and is not finite or not positive while
 * bank_kwh > 0 (dgen_batt_curve's rule).  A flagged agent gets 0 in every
 * summary member, in its plane values and in bank_out / power_out, as
 * dgen_batt_summary treats a skipped agent; no other agent's bits change.
 * DGEN_ST_UNIT, _TARIFF and _YEARS do not arise.
 * bank_out, power_out: bank and power as sized (dgen_batt_curve's bank_kwh and
 * power_kw at the same point).
 * The daily plan under the constant efficiencies only: batt_update_hours == 1
 * or batt_loss_model == 1 returns DGEN_E_ARG, as does a window with mid_lo >
 * mid_hi or outside 0..23, planes->f64 outside 0..1, a plane that is not
 * 16-byte aligned (a lane stores its hour quad as 16-B vectors), and n >= 2^27
 * when planes are given (the lane's 32-bit tile offset).  Table and agent-column checks
 * are dgen_batt_summary's.  No atomics and no cross-lane traffic: run-to-run
 * identical, and agent i's results do not depend on n or on its neighbours.
 * A call that asks for the summary and the planes runs the year once for each
 * (two launches on `stream`); every value has the bits of the call that asks
 * for it alone.                                                             */
typedef struct {           /* hour-quad tiles: (h, i) at ((h / 4) * n + i) * 4 + h % 4; 16-byte aligned; any may be NULL */
    void *baseline, *pvonly, *with_batt;
    int32_t f64;           /* 0: float32 planes, 1: float64 */
    int32_t pad;
} dgen_replay_planes;

int32_t dgen_replay_at(dgen_ctx* ctx, const dgen_tables* tables, const dgen_agents* agents,
                       const double* kw, const double* bank_kwh, const double* bank_kw, int64_t n,
                       const dgen_batt_summary_opt* opt, const dgen_batt_summary_out* summary,
                       const dgen_replay_planes* planes, double* bank_out, double* power_out,
                       int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DGEN_HIP_H */
