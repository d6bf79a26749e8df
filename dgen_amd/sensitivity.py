"""NPV against PV size: how flat is an agent's optimum?

npv_curve() evaluates every agent of an uploaded batch at a grid of sizes
relative to a base size (default: the size whose annual generation equals the
agent's load, load_kwh / naep -- the centre of the search's bracket) in one
device call (Engine.objective_curve).  Each point is its own
calc_system_performance(kw, en_batt=False) from the agent's initial tariff, so
a curve shows the rate switch's thresholds as steps.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib

DEFAULT_REL = (0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4, 1.5)


def size_grid(base, rel: Sequence[float] = DEFAULT_REL) -> np.ndarray:
    """xs[k, i] = rel[k] * base[i] (float64, [K, n]): the sizes of the curve."""
    r = np.asarray(rel, np.float64).reshape(-1)
    b = np.asarray(base, np.float64).reshape(-1)
    if not 1 <= r.size <= _lib.CURVE_MAX_POINTS:
        raise ValueError(f"rel must hold 1..{_lib.CURVE_MAX_POINTS} factors (got {r.size})")
    return r[:, None] * b[None, :]


def to_device_order(a: np.ndarray, perm: Optional[np.ndarray]) -> np.ndarray:
    """Caller-order columns [..., n] -> the batch's device order (device row j
    holds caller agent perm[j])."""
    return a if perm is None else a[..., np.asarray(perm, np.int64)]


def to_caller_order(a: np.ndarray, perm: Optional[np.ndarray]) -> np.ndarray:
    """Device-order columns [..., n] -> caller order (the inverse of
    to_device_order)."""
    if perm is None:
        return a
    out = np.empty_like(a)
    out[..., np.asarray(perm, np.int64)] = a
    return out


def npv_curve(engine, batch, rel: Sequence[float] = DEFAULT_REL, base=None,
              want=("npv", "payback_raw", "tariff", "switched", "status")) -> Dict[str, np.ndarray]:
    """The objective of every agent of `batch` at xs[k, i] = rel[k] * base[i].
    base: one size per agent in caller order (default load_kwh / naep).
    Returns host arrays in caller order: "kw" ([K, n], the sizes) and the
    members named by `want` ([K, n] each, _lib.CURVE_FIELDS)."""
    if base is None:
        naep = engine.profile_sums()[1]
        base_dev = batch.cols["load_kwh"].cpu().numpy() / naep[batch.cols["cf_row"].cpu().numpy()]
    else:
        base = np.asarray(base, np.float64).reshape(-1)
        if base.size != batch.n:
            raise ValueError(f"base must hold one size per agent ({batch.n}), got {base.size}")
        base_dev = to_device_order(base, batch.perm)
    xs = size_grid(base_dev, rel)
    res = engine.objective_curve(batch, xs, want=want)
    import torch
    torch.cuda.current_stream(engine.dev).synchronize()
    out = {"kw": to_caller_order(xs, batch.perm)}
    for k, v in res.items():
        out[k] = to_caller_order(v.cpu().numpy(), batch.perm)
    return out
