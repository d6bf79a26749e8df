"""The populations of the search-audit tests (test_search_audit.py on the CPU,
test_gpu_search_trace.py on the device) and the oracle's own search traces of
them, computed once per session."""
from functools import lru_cache

import numpy as np

from oracle import oracle as orc
from tests import helpers
from tests.test_gpu_exact import _small

# test_gpu_exact's eight populations (its _small tables) at reduced n;
# national_mixed with the long-life edit (33..50-year lives on every third agent)
POPULATIONS = (("de_res", 48, False), ("res_1m_nem_tou", 48, False), ("ca_res_storage", 48, False),
               ("com_8m", 48, False), ("com_kwkw", 48, False), ("com_dc_batt", 48, False),
               ("metering_mix", 64, False), ("national_mixed", 96, True))
IDS = [p[0] for p in POPULATIONS]


@lru_cache(maxsize=None)
def population(cfg, n, long_life):
    return _small(cfg, n, long_life=long_life)


@lru_cache(maxsize=None)
def oracle_case(cfg, n, long_life):
    """(pop, traces, results): traces[i] the oracle's [nfev, 2] (x, f) pairs of
    agent i's search, results[i] its outputs.  com_dc_batt bills its demand
    charges (the extension mode, as tests/test_gpu_demand.py sets it up)."""
    pop = population(cfg, n, long_life)
    opop = helpers.oracle_population(pop.cols, pop.tariffs, pop.switches, pop.shapes, pop.cfs, pop.wholesale,
                                     demand=None if pop.skip_demand_charges else pop.demand)
    ocfg = orc.make_cfg()
    traces, results = [], []
    for i in range(n):
        t, res = orc.brent_trace(opop, ocfg, i)
        traces.append(t.copy())
        results.append(res[0])
    return pop, traces, results


def brackets(pop):
    """(low, high, xatol) per agent, from the columns (numpy's row sums)."""
    from dgen_amd.search_audit import bracket_of
    naep = (pop.cfs.astype(np.float64) / 1e6).sum(axis=1)             # ff:350-351: gen_per_kw.sum()
    return [bracket_of(pop.cols["load_kwh"][i], naep[pop.cols["cf_row"][i]]) for i in range(len(pop.cols["load_kwh"]))]
