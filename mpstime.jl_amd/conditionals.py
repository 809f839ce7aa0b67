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
in raw units would need its Jacobian).  Both calls take COMPLETE series.

``marginal_conditionals`` is the same question for INCOMPLETE series (``mpst_marginal_conditionals``, csrc/mpst_margcond.inl): the
distribution of every site, known or missing, given only the values that were observed at the other sites, the missing ones summed
out under the Born rule.  At a missing site it is the predictive distribution ``p(x_t | observed)`` - not the sequential imputer's
chain of point estimates, whose bands narrow along a gap and depend on ``impute_order``; at a known site the leave-one-out score of a
series with dropped samples.  ``impute_marginal`` fills every missing site from its own marginal conditional, ``forecast`` masks the
last ``horizon`` sites and returns the point forecast and its bands, ``anomaly_scores(..., missing_mask=)`` scores incomplete series.
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


def anomaly_scores(imp, rows=None, reduce="mean", engine: Optional[SweepEngine] = None, device: int = 0, missing_mask=None):
    """``-ln p(x_t | x_{!=t})`` of the complete series ``imp.X_test[rows]``, reduced over the sites: ``"mean"`` or ``"max"`` give (N,),
    ``None`` the (N, T) profile that localises the anomaly.  ``missing_mask`` (rows, T): the series are incomplete - the scores of
    the known sites are leave-one-out scores with the missing sites summed out (``marginal_conditionals``), the masked sites are NaN
    in the profile and left out of the reduction (a row with nothing known reduces to NaN)."""
    if reduce not in ("mean", "max", None):
        raise ValueError(f'reduce must be "mean", "max" or None, not {reduce!r}')
    if missing_mask is not None:
        mask = np.asarray(missing_mask, dtype=bool)
        nll = np.where(mask, np.nan, marginal_conditionals(imp, mask, rows, get_wmad=False, engine=engine, device=device).nll)
        if reduce is None:
            return nll
        out = np.full(nll.shape[0], np.nan)
        some = ~mask.all(axis=1)
        out[some] = np.nanmean(nll[some], axis=1) if reduce == "mean" else np.nanmax(nll[some], axis=1)
        return out
    _selected_rows(imp, rows)
    nll = site_conditionals(imp, rows, get_wmad=False, engine=engine, device=device).nll
    if reduce is None:
        return nll
    return nll.mean(axis=1) if reduce == "mean" else nll.max(axis=1)


@dataclass
class MarginalConditionals:
    x: np.ndarray                       # (N, T) the values in the encoding's domain; NaN at a missing site without a true value
    missing: np.ndarray                 # (N, T) bool
    nll: np.ndarray                     # (N, T) -ln p(x_t | known others): leave-one-out at known sites, held-out at missing ones; NaN without a value
    pit: np.ndarray                     # (N, T) F(x_t | known others), NaN likewise
    median: np.ndarray                  # (N, T)
    err: Optional[np.ndarray]           # (N, T) WMAD, None without get_wmad
    mean: np.ndarray                    # (N, T) trapezoid(x p) / Z
    quantiles: Optional[np.ndarray]     # (N, T, nq), None without levels
    seconds: float = 0.0                # device seconds of the call


def marginal_conditionals_model(eng: SweepEngine, W, phi, label_index, missing, x, grid_x, grid_phi, levels=None, get_wmad=True,
                                label_site=None):
    """mpst_marginal_conditionals on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) the encoded values, real or complex - read at the known sites, and at a missing site only where ``x`` is finite;
    ``label_index`` (N,) the classes; ``missing`` (N, T) True where a site is missing, None: nothing is; ``x`` (N, T) the values in the
    encoding's domain, at a missing site the held-out true value or NaN; ``grid_x`` (ngrid,) evenly spaced candidate values and
    ``grid_phi`` their states, (ngrid, d) or one table per site (T, ngrid, d); ``levels``: up to 16 numbers inside (0, 1).
    Returns a ``MarginalConditionals``."""
    lv = check_levels(levels)
    cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi) or np.iscomplexobj(grid_phi)
    dt = np.complex128 if cx else np.float64
    model, keep = model_to_abi([np.asarray(t, dtype=dt) for t in W], np.asarray(phi, dtype=dt), "f64", label_site)
    N, T, d = int(model.N), int(model.T), int(model.d)
    lab = np.ascontiguousarray(label_index, dtype=np.int32)
    xs = np.ascontiguousarray(x, dtype=np.float64)
    m8 = None if missing is None else np.ascontiguousarray(np.asarray(missing) != 0, dtype=np.uint8)
    gx = np.ascontiguousarray(grid_x, dtype=np.float64)
    gp = np.ascontiguousarray(grid_phi, dtype=dt)
    assert lab.shape == (N,) and xs.shape == (N, T) and gp.shape in ((len(gx), d), (T, len(gx), d))
    assert m8 is None or m8.shape == (N, T)
    model.label_idx = lab.ctypes.data_as(C.POINTER(C.c_int32))
    dp = C.POINTER(C.c_double)
    nq = 0 if lv is None else len(lv)
    o = L.SiteCondOpts(int(gp.ndim == 3), int(bool(get_wmad)), nq, 0, None if lv is None else lv.ctypes.data_as(dp))
    nll, pit, med, err, mean = (np.zeros((N, T)) for _ in range(5))
    q = np.zeros((N, T, nq)) if nq else None
    sec = C.c_double()
    eng._chk(eng.lib.mpst_marginal_conditionals(eng.ctx, C.byref(model), None if m8 is None else m8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                xs.ctypes.data_as(dp), gx.ctypes.data_as(dp), C.c_void_p(gp.ctypes.data), len(gx), C.byref(o),
                                                nll.ctypes.data_as(dp), pit.ctypes.data_as(dp), med.ctypes.data_as(dp), err.ctypes.data_as(dp),
                                                mean.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), C.byref(sec)))
    del keep
    miss = np.zeros((N, T), dtype=bool) if m8 is None else m8.astype(bool)
    return MarginalConditionals(xs, miss, nll, pit, med, err if get_wmad else None, mean, q, sec.value)


def _true_values(imp, enc, norms, raw, oob):
    """The raw values through the test transform of the MASKED series: the train-fitted transforms, then the out-of-bounds rescale its
    row got in ``_scaled_instances`` (not the one the complete series would get).  NaN stays NaN."""
    from .encodings import transform_test_data
    fin = np.isfinite(raw)
    t, _ = transform_test_data(np.where(fin, raw, 0.0), norms, imp.opts, (0.0, 1.0), rescale_out_of_bounds=False)
    for i, lo, hi in oob:
        t[int(i)] = (t[int(i)] - lo) / hi
    a, b = enc.range
    return np.where(fin, (b - a) * t + a, np.nan)


def _marginal_run(imp, missing_mask, rows, quantiles, get_wmad, engine, device):
    from .imputation import _scaled_instances
    levels = check_levels(quantiles)
    rows = np.arange(imp.X_test.shape[0]) if rows is None else np.atleast_1d(np.asarray(rows))
    mask = np.asarray(missing_mask, dtype=bool)
    if mask.shape != (len(rows), imp.X_test.shape[1]):
        raise ValueError(f"missing_mask must have the shape (rows, T) = {(len(rows), imp.X_test.shape[1])}, not {mask.shape}")
    raw = np.asarray(imp.X_test, dtype=np.float64)[rows]
    if not np.all(np.isfinite(raw[~mask])):
        raise ValueError("a selected row holds a NaN or non-finite value at a site missing_mask calls known")
    enc, norms, _, _, scaled, oob = _scaled_instances(imp, rows, mask)
    lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test)[rows].tolist()], dtype=np.int32)
    xr = imp.x_guess_range
    N, T = scaled.shape
    if N == 0:
        z = np.zeros((0, T))
        return MarginalConditionals(z, mask, z.copy(), z.copy(), z.copy(), z.copy() if get_wmad else None, z.copy(),
                                    None if levels is None else np.zeros((0, T, len(levels)))), (enc, norms, scaled, oob, mask)
    true = _true_values(imp, enc, norms, raw, oob)
    a, b = enc.range
    inside = np.isfinite(true) & (true >= a) & (true <= b)
    x = np.where(mask, true, scaled)                                        # held-out values where the test set has them, NaN elsewhere
    states = imp.encoder(np.where(mask & inside, true, scaled))             # a value outside the range is not encoded: its nll is NaN below
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        out = marginal_conditionals_model(eng, imp.mps, states, lab, mask, x, xr.xvals, xr.xvals_enc, levels=levels, get_wmad=get_wmad)
    finally:
        if own:
            eng.close()
    out.nll[mask & np.isfinite(true) & ~inside] = np.nan
    return out, (enc, norms, scaled, oob, mask)


def marginal_conditionals(imp, missing_mask, rows=None, quantiles=None, get_wmad: bool = True, engine: Optional[SweepEngine] = None,
                          device: int = 0):
    """The marginal site conditionals of ``imp.X_test[rows]`` (default: all) with the sites of ``missing_mask`` (rows, T) treated as
    missing, each series under the MPS of its class ``imp.y_test``: a ``MarginalConditionals`` in the encoding's domain, as
    ``site_conditionals`` leaves its results.  Pre-processing is imputation's own (``_scaled_instances``), so split and time-dependent
    encodings go through the fitted encoder and the per-site tables.  Where the test set holds a finite value at a masked site it goes
    through the same per-series transform as the masked series and gives the held-out ``nll`` / ``pit`` there (NaN where it holds
    none); a true value outside the encoding's range gives ``nll`` NaN and ``pit`` 0 or 1.  ``quantiles``: up to 16 levels inside
    (0, 1).  Raises ValueError on a non-finite value at a site the mask calls known, KeyError on a label the model was not trained on."""
    return _marginal_run(imp, missing_mask, rows, quantiles, get_wmad, engine, device)[0]


def impute_marginal(imp, missing_mask, rows=None, statistic: str = "median", quantiles=None, invert_transform: bool = True,
                    engine: Optional[SweepEngine] = None, device: int = 0):
    """Fill every missing site of ``imp.X_test[rows]`` with the ``statistic`` - ``"median"`` or ``"mean"`` - of its own marginal
    conditional ``p(x_t | observed)``; known values are kept.  Unlike ``impute_dataset`` no site is conditioned on a value imputed
    before it, so the result does not depend on an order.  Returns ``X_imputed`` (N, T), or ``(X_imputed, bands)`` with ``quantiles``:
    bands (N, T, nq), the known value in every level at a known site.  Units and bands follow ``impute_dataset(..., quantiles=)``:
    ``invert_transform`` maps everything back with the instance's own out-of-bounds rescale.  Quantiles and the median commute with
    that monotone transform; the MEAN does not - with ``invert_transform`` the mean of the encoding's domain is mapped, which is not
    the mean in the original units under a nonlinear transform (the sigmoid)."""
    from .imputation import invert_test_transform
    if statistic not in ("median", "mean"):
        raise ValueError(f'statistic must be "median" or "mean", not {statistic!r}')
    mc, (enc, norms, scaled, oob, mask) = _marginal_run(imp, missing_mask, rows, quantiles, False, engine, device)
    ts = np.where(mask, mc.median if statistic == "median" else mc.mean, scaled)
    bands = None if mc.quantiles is None else np.where(mask[:, :, None], mc.quantiles, scaled[:, :, None])
    if invert_transform and ts.shape[0]:
        ts = invert_test_transform(ts, oob, norms, imp.opts, enc.range)
        if bands is not None:
            bands = np.stack([invert_test_transform(bands[:, :, l], oob, norms, imp.opts, enc.range) for l in range(bands.shape[2])], axis=2)
    return ts if bands is None else (ts, bands)


def forecast(imp, horizon, rows=None, quantiles=(0.05, 0.95), statistic: str = "median", invert_transform: bool = True,
             engine: Optional[SweepEngine] = None, device: int = 0):
    """``impute_marginal`` with the last ``horizon`` sites masked: ``p(x_{T-horizon+k} | x_0 .. x_{T-horizon-1})`` for every step k of
    the horizon from one call.  Returns ``(point, bands)``: the (N, horizon) point forecast and the (N, horizon, nq) bands."""
    T = imp.X_test.shape[1]
    if int(horizon) != horizon or not 1 <= int(horizon) <= T:
        raise ValueError(f"horizon must be an integer in 1 .. T = {T}, not {horizon!r}")
    h = int(horizon)
    n = imp.X_test.shape[0] if rows is None else len(np.atleast_1d(np.asarray(rows)))
    mask = np.zeros((n, T), dtype=bool)
    mask[:, T - h:] = True
    ts, bands = impute_marginal(imp, mask, rows, statistic=statistic, quantiles=quantiles, invert_transform=invert_transform, engine=engine,
                                device=device)
    return ts[:, T - h:], bands[:, T - h:]


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
