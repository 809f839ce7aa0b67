"""Rolling-origin forecasts on the device (``mpst_rolling_forecasts``, csrc/mpst_rolling.inl): how well the model forecasts, horizon by
horizon, from every point of a series.

For every complete series i, every origin t = 0 .. T-1 and every horizon h = 1 .. H with u = t + h - 1 < T, entry ``[i, t, h - 1]`` of
every output describes the predictive distribution of ``x_u`` given ``x_0 .. x_{t-1}`` only - the Born rule of
``marginal_conditionals`` on the suffix mask of t, read at site u - for all origins from one walk per series against model-only tables.
Entries with t + h > T are NaN.  A series is forecast under the MPS of its class, or - where the class is not known, as at an early
origin it usually is not - under the class mixture, every class weighted by the likelihood of the values seen so far
(``prefix_posteriors`` at length t).

Everything after the device call is NumPy on those arrays: ``valid_forecast_triangle``, ``horizon_errors_from``,
``interval_coverage_from`` and ``pinball_loss_from`` take (N, T, H) arrays and the values, and nothing else.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

from . import _lib as L
from .engine import SweepEngine, check_levels, model_to_abi


@dataclass
class RollingForecasts:
    x: np.ndarray                       # (N, T) the observed values, in the units of the forecasts
    median: np.ndarray                  # (N, T, H)
    mean: np.ndarray                    # (N, T, H) trapezoid(x p) / Z
    wmad: Optional[np.ndarray]          # (N, T, H) WMAD in the encoding's domain, None without get_wmad
    levels: Optional[np.ndarray]        # (N, T, H, nq), None without quantiles
    nll: np.ndarray                     # (N, T, H) -ln p(x_u | x_0 .. x_{t-1}) in the encoding's domain
    pit: np.ndarray                     # (N, T, H) F(x_u | x_0 .. x_{t-1})
    seconds: float = 0.0                # device seconds of the call


class Backtest(NamedTuple):
    mae: np.ndarray                     # (H,) mean absolute error of the median by horizon
    rmse: np.ndarray                    # (H,)
    coverage: Optional[np.ndarray]      # (H,) share of the values inside [lowest, highest] level; None with fewer than two levels
    pinball: Optional[np.ndarray]       # (H, nq) mean pinball loss of every level; None without levels
    nll: np.ndarray                     # (H,) mean -ln p
    pit: list                           # H arrays: the PIT values of the horizon over the valid triangle
    forecasts: RollingForecasts


def rolling_forecasts_model(eng: SweepEngine, W, phi, label_index, max_horizon, x, grid_x, grid_phi, levels=None, get_wmad=True,
                            label_site=None):
    """mpst_rolling_forecasts on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) the encoded values of complete series, real or complex; ``label_index`` (N,) their classes, -1 for the class
    mixture; ``max_horizon`` in 1 .. T; ``x`` (N, T) the values in the encoding's domain, or None (no pit); ``grid_x`` (ngrid,) evenly
    spaced candidate values and ``grid_phi`` their states, (ngrid, d) or one table per site (T, ngrid, d); ``levels``: up to 16 numbers
    inside (0, 1).  Returns (nll, pit, median, err, mean, q, seconds): (N, T, H) arrays with entry [i, t, h - 1], pit None without
    ``x``, q (N, T, H, nq) or None."""
    lv = check_levels(levels)
    cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi) or np.iscomplexobj(grid_phi)
    dt = np.complex128 if cx else np.float64
    model, keep = model_to_abi([np.asarray(t, dtype=dt) for t in W], np.asarray(phi, dtype=dt), "f64", label_site)
    N, T, d = int(model.N), int(model.T), int(model.d)
    H = int(max_horizon)
    lab = np.ascontiguousarray(label_index, dtype=np.int32)
    xs = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    gx = np.ascontiguousarray(grid_x, dtype=np.float64)
    gp = np.ascontiguousarray(grid_phi, dtype=dt)
    assert lab.shape == (N,) and (xs is None or xs.shape == (N, T)) and gp.shape in ((len(gx), d), (T, len(gx), d))
    model.label_idx = lab.ctypes.data_as(C.POINTER(C.c_int32))
    dp = C.POINTER(C.c_double)
    nq = 0 if lv is None else len(lv)
    o = L.SiteCondOpts(int(gp.ndim == 3), int(bool(get_wmad)), nq, 0, None if lv is None else lv.ctypes.data_as(dp))
    Hs = max(H, 0)
    nll, med, err, mean = (np.zeros((N, T, Hs)) for _ in range(4))
    pit = None if xs is None else np.zeros((N, T, Hs))
    q = np.zeros((N, T, Hs, nq)) if nq else None
    sec = C.c_double()
    eng._chk(eng.lib.mpst_rolling_forecasts(eng.ctx, C.byref(model), H, None if xs is None else xs.ctypes.data_as(dp), gx.ctypes.data_as(dp),
                                            C.c_void_p(gp.ctypes.data), len(gx), C.byref(o), nll.ctypes.data_as(dp),
                                            None if pit is None else pit.ctypes.data_as(dp), med.ctypes.data_as(dp), err.ctypes.data_as(dp),
                                            mean.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), C.byref(sec)))
    del keep
    return nll, pit, med, err if get_wmad else None, mean, q, sec.value


def _check_horizon(max_horizon, T):
    if int(max_horizon) != max_horizon or not 1 <= int(max_horizon) <= T:
        raise ValueError(f"max_horizon must be an integer in 1 .. T = {T}, not {max_horizon!r}")
    return int(max_horizon)


def rolling_forecasts(imp, max_horizon, rows=None, quantiles=(0.05, 0.95), classes: str = "label", invert_transform: bool = True,
                      get_wmad: bool = True, engine: Optional[SweepEngine] = None, device: int = 0) -> RollingForecasts:
    """The rolling-origin forecasts of the complete series ``imp.X_test[rows]`` (default: all): a ``RollingForecasts`` with entry
    ``[i, t, h - 1]`` for the forecast of site t + h - 1 from the first t values, NaN where t + h > T.  ``classes="label"``: each series
    under the MPS of its class ``imp.y_test``; ``"mixture"``: under the class mixture, every class weighted by the likelihood of the
    values seen so far, so that no label is used.

    The series go through the pre-processing of ``site_conditionals`` - ONE test transform per row, of the complete row.  A row's
    out-of-bounds rescale has therefore seen the row's later values: a row that leaves the training range is rescaled by its own
    extremes, whichever side of an origin they lie on.  Rows inside the range are not touched by it.

    With ``invert_transform`` the medians, the levels and ``x`` go back to the original units through ``invert_test_transform`` with the
    row's own rescale; quantiles commute with that monotone map.  The MEAN does not: the mean of the encoding's domain is mapped, which
    is not the mean in the original units under a nonlinear transform (the sigmoid).  ``nll``, ``pit`` and ``wmad`` stay in the encoding's
    domain.  Raises ValueError on a NaN or non-finite value in a selected row, KeyError on a label the model was not trained on."""
    from .conditionals import _selected_rows
    from .imputation import _scaled_instances, invert_test_transform
    if classes not in ("label", "mixture"):
        raise ValueError(f'classes must be "label" or "mixture", not {classes!r}')
    levels = check_levels(quantiles)
    T = imp.X_test.shape[1]
    H = _check_horizon(max_horizon, T)
    rows = _selected_rows(imp, rows, "rolling_forecasts conditions every origin")
    mask = np.zeros((len(rows), T), dtype=bool)
    enc, norms, _, _, scaled, oob = _scaled_instances(imp, rows, mask)
    if classes == "label":
        lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test)[rows].tolist()], dtype=np.int32)
    else:
        lab = np.full(len(rows), -1, dtype=np.int32)
    N = scaled.shape[0]
    nq = 0 if levels is None else len(levels)
    if N == 0:
        z = np.zeros((0, T, H))
        return RollingForecasts(np.zeros((0, T)), z, z.copy(), z.copy() if get_wmad else None, None if levels is None else np.zeros((0, T, H, nq)),
                                z.copy(), z.copy())
    xr = imp.x_guess_range
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        nll, pit, med, err, mean, q, secs = rolling_forecasts_model(eng, imp.mps, imp.encoder(scaled), lab, H, scaled, xr.xvals, xr.xvals_enc,
                                                                    levels=levels, get_wmad=get_wmad)
    finally:
        if own:
            eng.close()
    x = scaled
    if invert_transform:
        def back(a):            # (N, T, H): elementwise and per row, NaN stays NaN
            return invert_test_transform(a.reshape(N, T * H), oob, norms, imp.opts, enc.range).reshape(N, T, H)
        x = invert_test_transform(scaled, oob, norms, imp.opts, enc.range)
        med, mean = back(med), back(mean)
        if q is not None:
            q = np.stack([back(q[..., l]) for l in range(nq)], axis=3)
    return RollingForecasts(x, med, mean, err, q, nll, pit, secs)


# ---- NumPy on the arrays --------------------------------------------------------------------------------------------------------------
def valid_forecast_triangle(T, H):
    """(T, H) bool: the target of horizon h = column + 1 from the origin t = row lies inside the series, t + h <= T"""
    return np.arange(T)[:, None] + np.arange(1, H + 1)[None, :] <= T


def targets_of(x, H):
    """(N, T, H): ``x[i, t + h - 1]`` at [i, t, h - 1], NaN beyond the series"""
    x = np.asarray(x, dtype=np.float64)
    N, T = x.shape
    u = np.arange(T)[:, None] + np.arange(H)[None, :]
    return np.where((u < T)[None], x[:, np.minimum(u, T - 1)], np.nan)


def _counted(a, x, min_origin):
    a = np.asarray(a, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if a.ndim < 3 or x.shape != a.shape[:2] or not 1 <= a.shape[2] <= max(a.shape[1], 1):
        raise ValueError(f"forecasts must be (N, T, H[, ..]) with 1 <= H <= T and x (N, T), got {a.shape} and {x.shape}")
    T, H = a.shape[1:3]
    if int(min_origin) != min_origin or not 0 <= int(min_origin) < max(T, 1):
        raise ValueError(f"min_origin must be an integer in 0 .. T - 1 = {T - 1}, not {min_origin!r}")
    keep = valid_forecast_triangle(T, H) & (np.arange(T)[:, None] >= int(min_origin))
    return a, targets_of(x, H), keep


def _mean_over(v, ok):
    """per horizon the mean of v (N, T, H) over ok; NaN for a horizon without an entry"""
    n = ok.sum(axis=(0, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, v, 0.0).sum(axis=(0, 1)) / n


def horizon_errors_from(point, x, min_origin=0):
    """(mae (H,), rmse (H,)) of the point forecasts ``point`` (N, T, H) against ``x`` (N, T) over the valid triangle from the origin
    ``min_origin`` on; entries whose forecast is NaN are left out, a horizon without an entry gives NaN."""
    p, tgt, keep = _counted(point, x, min_origin)
    ok = keep[None] & np.isfinite(p) & np.isfinite(tgt)
    e = np.where(ok, p - tgt, 0.0)
    return _mean_over(np.abs(e), ok), np.sqrt(_mean_over(e * e, ok))


def interval_coverage_from(lo, hi, x, min_origin=0):
    """(H,) the share of the values with ``lo <= x <= hi`` (both (N, T, H)) over the valid triangle from ``min_origin`` on"""
    lo, tgt, keep = _counted(lo, x, min_origin)
    hi = np.asarray(hi, dtype=np.float64)
    if hi.shape != lo.shape:
        raise ValueError("lo and hi must have the same shape")
    ok = keep[None] & np.isfinite(lo) & np.isfinite(hi) & np.isfinite(tgt)
    with np.errstate(invalid="ignore"):
        inside = (lo <= tgt) & (tgt <= hi)
    return _mean_over(inside.astype(np.float64), ok)


def pinball_loss_from(levels, q, x, min_origin=0):
    """(H, nq) the mean pinball loss ``max(tau (x - q), (tau - 1) (x - q))`` of the quantile forecasts ``q`` (N, T, H, nq) at the levels
    ``levels`` (nq,) over the valid triangle from ``min_origin`` on"""
    q, tgt, keep = _counted(q, x, min_origin)
    tau = np.asarray(levels, dtype=np.float64)
    if q.ndim != 4 or tau.shape != (q.shape[3],):
        raise ValueError("q must be (N, T, H, nq) and levels (nq,)")
    out = np.zeros((q.shape[2], len(tau)))
    for l, a in enumerate(tau):
        ok = keep[None] & np.isfinite(q[..., l]) & np.isfinite(tgt)
        diff = np.where(ok, tgt - q[..., l], 0.0)
        out[:, l] = _mean_over(np.maximum(a * diff, (a - 1.0) * diff), ok)
    return out


def backtest(imp, max_horizon, min_origin=0, rows=None, quantiles=(0.05, 0.95), classes: str = "label", invert_transform: bool = True,
             engine: Optional[SweepEngine] = None, device: int = 0) -> Backtest:
    """``rolling_forecasts`` and its summaries by horizon over the origins from ``min_origin`` on: MAE and RMSE of the median, the
    coverage of the band between the lowest and the highest level, the pinball loss of every level, the mean ``nll`` and the PIT values.
    Errors, coverage and pinball loss are in the units of the forecasts (``invert_transform``)."""
    f = rolling_forecasts(imp, max_horizon, rows, quantiles, classes, invert_transform, get_wmad=False, engine=engine, device=device)
    levels = check_levels(quantiles)
    mae, rmse = horizon_errors_from(f.median, f.x, min_origin)
    cover = pin = None
    if levels is not None:
        pin = pinball_loss_from(levels, f.levels, f.x, min_origin)
        if len(levels) >= 2:
            cover = interval_coverage_from(f.levels[..., int(np.argmin(levels))], f.levels[..., int(np.argmax(levels))], f.x, min_origin)
    _, _, keep = _counted(f.nll, f.x, min_origin)
    ok = keep[None] & np.isfinite(f.nll)
    pits = [f.pit[:, :, h][keep[None, :, h] & np.isfinite(f.pit[:, :, h])] for h in range(f.pit.shape[2])]
    return Backtest(mae, rmse, cover, pin, _mean_over(f.nll, ok), pits, f)
