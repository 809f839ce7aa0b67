"""Leave-one-out site conditionals on the device (``mpst_site_conditionals``, csrc/mpst_sitecond.inl).

Given a COMPLETE series, how surprising is each single value given all the others?  For every site t the engine forms the
conditional ``p(x_t | x_{!=t})`` under the series' class - the distribution the median imputer would read its value from if t were
the only missing site - from one left and one right walk over the chain, and reads off it

* ``nll``: ``-ln p`` at the observed value (per unit of the encoding's domain, at the exact encoded state): anomaly localisation, and a
  proper score to tune imputation models on;
* ``pit``: the probability integral transform ``F(x_t | x_{!=t})``: uniform on (0, 1) for a calibrated model;
* ``median`` / ``err`` / ``quantiles``: the median imputer's value, its WMAD and more levels of the same distribution.

``window_conditionals`` asks the same of a SUBSEQUENCE (``mpst_window_conditionals``, csrc/mpst_window.inl): ``-ln`` of the Born
probability of the values of a window ``t .. t+w-1`` given all the others, for every start and every width up to ``max_width`` from
one pass per start - an anomaly map over (position, scale) for samples that are each plausible alone and implausible together.

Everything is in the encoding's domain, as ``get_cdfs`` leaves its results (the transform is nonlinear under the sigmoid; a density
in raw units would need its Jacobian).  Series with missing values are not this call's business: ``log_marginals`` scores them,
``impute_dataset`` fills them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .engine import SweepEngine, check_levels, model_to_abi


@dataclass
class SiteConditionals:
    x: np.ndarray                       # (N, T) the observed values in the encoding's domain
    nll: np.ndarray                     # (N, T) -ln p(x_t | x_{!=t})
    pit: np.ndarray                     # (N, T) F(x_t | x_{!=t})
    median: np.ndarray                  # (N, T)
    err: Optional[np.ndarray]           # (N, T) WMAD, None without get_wmad
    quantiles: Optional[np.ndarray]     # (N, T, nq), None without levels


def site_conditionals_model(eng: SweepEngine, W, phi, label_index, x, grid_x, grid_phi, levels=None, get_wmad=True, compute="f64",
                            label_site=None):
    """mpst_site_conditionals on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) the encoded values of complete series, real or complex; ``label_index`` (N,) their classes; ``x`` (N, T) the
    values themselves in the encoding's domain; ``grid_x`` (ngrid,) evenly spaced candidate values and ``grid_phi`` their states,
    (ngrid, d) or one table per site (T, ngrid, d); ``levels``: up to 16 numbers inside (0, 1).
    Returns (nll, pit, median, err, q, seconds): (N, T) arrays, q (N, T, nq) or None."""
    lv = check_levels(levels)
    if compute not in ("f64", "f32"):
        raise ValueError('compute must be "f64" or "f32"')
    cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi) or np.iscomplexobj(grid_phi)
    dt = np.complex128 if cx else np.float64
    model, keep = model_to_abi([np.asarray(t, dtype=dt) for t in W], np.asarray(phi, dtype=dt), compute, label_site)
    N, T, d = int(model.N), int(model.T), int(model.d)
    lab = np.ascontiguousarray(label_index, dtype=np.int32)
    xs = np.ascontiguousarray(x, dtype=np.float64)
    gx = np.ascontiguousarray(grid_x, dtype=np.float64)
    gp = np.ascontiguousarray(grid_phi, dtype=dt)
    assert lab.shape == (N,) and xs.shape == (N, T) and gp.shape in ((len(gx), d), (T, len(gx), d))
    model.label_idx = lab.ctypes.data_as(C.POINTER(C.c_int32))
    dp = C.POINTER(C.c_double)
    nq = 0 if lv is None else len(lv)
    o = L.SiteCondOpts(int(gp.ndim == 3), int(bool(get_wmad)), nq, 0, None if lv is None else lv.ctypes.data_as(dp))
    nll, pit, med, err = (np.zeros((N, T)) for _ in range(4))
    q = np.zeros((N, T, nq)) if nq else None
    sec = C.c_double()
    eng._chk(eng.lib.mpst_site_conditionals(eng.ctx, C.byref(model), xs.ctypes.data_as(dp), gx.ctypes.data_as(dp), C.c_void_p(gp.ctypes.data),
                                            len(gx), C.byref(o), nll.ctypes.data_as(dp), pit.ctypes.data_as(dp), med.ctypes.data_as(dp),
                                            err.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), C.byref(sec)))
    del keep
    return nll, pit, med, err, q, sec.value


def _selected_rows(imp, rows, what="site_conditionals conditions every site"):
    rows = np.arange(imp.X_test.shape[0]) if rows is None else np.atleast_1d(np.asarray(rows))
    raw = np.asarray(imp.X_test, dtype=np.float64)[rows]
    if not np.all(np.isfinite(raw)):
        raise ValueError(f"{what} on all the others: a selected row holds a NaN or non-finite value. "
                         "Incomplete series are scored by log_marginals and filled by impute_dataset")
    return rows


def site_conditionals(imp, rows=None, quantiles=None, get_wmad: bool = True, engine: Optional[SweepEngine] = None, device: int = 0,
                      return_seconds: bool = False):
    """The leave-one-out conditionals of the complete series ``imp.X_test[rows]`` (default: all), each under the MPS of its class
    ``imp.y_test``: a ``SiteConditionals`` in the encoding's domain.  The series go through imputation's own pre-processing
    (``_scaled_instances`` with an empty mask) and the fitted encoder; the candidate grid and its table - one per site for
    time-dependent encodings - are those ``init_imputation_problem`` tabulated.  ``quantiles``: up to 16 levels inside (0, 1).
    Raises ValueError on a NaN or non-finite value in a selected row, KeyError on a label the model was not trained on (as
    ``impute_dataset`` does)."""
    from .imputation import _scaled_instances
    levels = check_levels(quantiles)
    rows = _selected_rows(imp, rows)
    mask = np.zeros((len(rows), imp.X_test.shape[1]), dtype=bool)
    scaled = _scaled_instances(imp, rows, mask)[4]
    lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test)[rows].tolist()], dtype=np.int32)
    xr = imp.x_guess_range
    N, T = scaled.shape
    if N == 0:
        z = np.zeros((0, T))
        out = SiteConditionals(z, z.copy(), z.copy(), z.copy(), z.copy() if get_wmad else None,
                               None if levels is None else np.zeros((0, T, len(levels))))
        return (out, 0.0) if return_seconds else out
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        nll, pit, med, err, q, secs = site_conditionals_model(eng, imp.mps, imp.encoder(scaled), lab, scaled, xr.xvals, xr.xvals_enc,
                                                              levels=levels, get_wmad=get_wmad)
    finally:
        if own:
            eng.close()
    out = SiteConditionals(scaled, nll, pit, med, err if get_wmad else None, q)
    return (out, secs) if return_seconds else out


def anomaly_scores(imp, rows=None, reduce="mean", engine: Optional[SweepEngine] = None, device: int = 0):
    """``-ln p(x_t | x_{!=t})`` of the complete series ``imp.X_test[rows]``, reduced over the sites: ``"mean"`` or ``"max"`` give (N,),
    ``None`` the (N, T) profile that localises the anomaly."""
    if reduce not in ("mean", "max", None):
        raise ValueError(f'reduce must be "mean", "max" or None, not {reduce!r}')
    _selected_rows(imp, rows)
    nll = site_conditionals(imp, rows, get_wmad=False, engine=engine, device=device).nll
    if reduce is None:
        return nll
    return nll.mean(axis=1) if reduce == "mean" else nll.max(axis=1)


@dataclass
class WindowConditionals:
    x: np.ndarray                       # (N, T) the observed values in the encoding's domain
    nll: np.ndarray                     # (N, T, max_width) [i, t, w-1]: -ln P(x_t .. x_{t+w-1} | the rest); NaN where t + w > T


def window_conditionals_model(eng: SweepEngine, W, phi, label_index, max_width, label_site=None):
    """mpst_window_conditionals on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) the encoded values of complete series, real or complex; ``label_index`` (N,) their classes.
    Returns (nll, seconds): nll (N, T, max_width), entry [i, t, w-1] for the window of width w that starts at t, NaN where it would
    pass the end of the chain."""
    cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi)
    dt = np.complex128 if cx else np.float64
    model, keep = model_to_abi([np.asarray(t, dtype=dt) for t in W], np.asarray(phi, dtype=dt), "f64", label_site)
    N, T = int(model.N), int(model.T)
    lab = np.ascontiguousarray(label_index, dtype=np.int32)
    assert lab.shape == (N,)
    model.label_idx = lab.ctypes.data_as(C.POINTER(C.c_int32))
    nll = np.zeros((N, T, max(int(max_width), 1)))
    sec = C.c_double()
    eng._chk(eng.lib.mpst_window_conditionals(eng.ctx, C.byref(model), int(max_width), nll.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sec)))
    del keep
    return nll, sec.value


def _check_width(width, T, name="max_width"):
    if int(width) != width or not 1 <= int(width) <= T:
        raise ValueError(f"{name} must be an integer in 1 .. T = {T}, not {width!r}")
    return int(width)


def window_conditionals(imp, max_width, rows=None, engine: Optional[SweepEngine] = None, device: int = 0, return_seconds: bool = False):
    """The window conditionals of the complete series ``imp.X_test[rows]`` (default: all), each under the MPS of its class
    ``imp.y_test``, for every start and every width 1 .. ``max_width``: a ``WindowConditionals``.  The series go through the same
    pre-processing as ``site_conditionals``.  Raises ValueError on a NaN or non-finite value in a selected row and on a ``max_width``
    outside 1 .. T, KeyError on a label the model was not trained on."""
    from .imputation import _scaled_instances
    max_width = _check_width(max_width, imp.X_test.shape[1])
    rows = _selected_rows(imp, rows, "window_conditionals conditions every window")
    mask = np.zeros((len(rows), imp.X_test.shape[1]), dtype=bool)
    scaled = _scaled_instances(imp, rows, mask)[4]
    lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test)[rows].tolist()], dtype=np.int32)
    N, T = scaled.shape
    if N == 0:
        out = WindowConditionals(np.zeros((0, T)), np.zeros((0, T, max_width)))
        return (out, 0.0) if return_seconds else out
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        nll, secs = window_conditionals_model(eng, imp.mps, imp.encoder(scaled), lab, max_width)
    finally:
        if own:
            eng.close()
    out = WindowConditionals(scaled, nll)
    return (out, secs) if return_seconds else out


def window_anomaly_scores(imp, width, rows=None, per_site: bool = False, reduce="max", engine: Optional[SweepEngine] = None, device: int = 0):
    """``-ln P(window | rest)`` of every window of ``width`` samples of the complete series ``imp.X_test[rows]``:
    ``window_conditionals(imp, width).nll[:, :T-width+1, width-1]``, divided by ``width`` with ``per_site``.  ``reduce``: ``"max"`` or
    ``"mean"`` over the starts give (N,), ``None`` the (N, T-width+1) profile."""
    if reduce not in ("mean", "max", None):
        raise ValueError(f'reduce must be "mean", "max" or None, not {reduce!r}')
    T = imp.X_test.shape[1]
    width = _check_width(width, T, "width")
    nll = window_conditionals(imp, width, rows, engine=engine, device=device).nll[:, :T - width + 1, width - 1]
    if per_site:
        nll = nll / width
    if reduce is None:
        return nll
    return nll.mean(axis=1) if reduce == "mean" else nll.max(axis=1)
