"""Noisy and censored observations on the device (``mpst_observed_conditionals``, csrc/mpst_observed.inl).

Every other query of this package takes a value as exactly known or entirely missing.  Here a site carries a MEASUREMENT: an exact
value, nothing, a value with Gaussian noise of its own standard deviation (a light-curve point with its error bar), an interval (a
clipped sensor: "at least 4.2"; a quantised channel: "between 0.5 and 0.6") or, as the escape hatch, a Hermitian operator the caller
supplies.  A measurement with the likelihood ``k(y | x)`` enters the Born-rule density walk as the operator
``E = int k(y | x) phi(x) phi(x)^H dx`` where an exact value has ``phi phi^H`` and a missing one the identity; nothing else changes.
For every site the engine returns

* the PREDICTIVE group (``pred_*``): the distribution of the true value given the OTHER sites' observations;
* the POSTERIOR group (``post_*``): the same given ALL observations, the site's own included (``k_k p_k`` on the grid) - the denoised
  value and its bands; NaN at exact and operator sites;
* ``nll_obs``: ``-ln`` of the likelihood of the observation as it was made given the others - an anomaly score that respects the error
  bar; ``pit`` at exact sites;

and per series ``logev``, the log of the un-normalised chain value under its class, from which ``noisy_log_likelihoods``,
``noisy_class_posteriors`` and ``classify_noisy`` are read.  Everything is in the encoding's domain unless stated otherwise.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .engine import SweepEngine, check_levels, model_to_abi

EXACT, MISSING, GAUSS, INTERVAL, OPERATOR = 0, 1, 2, 3, 4


@dataclass
class ObservationModel:
    """What was observed at every site of N series: ``kind`` (N, T) of EXACT / MISSING / GAUSS / INTERVAL / OPERATOR and the two
    parameters ``a``, ``b`` (N, T): EXACT ``a`` = the value; GAUSS ``a`` = the observed value, ``b`` = the noise sd; INTERVAL
    ``a <= x <= b``.  ``operators`` (N, T, d, d): read at the OPERATOR sites only."""
    kind: np.ndarray
    a: np.ndarray
    b: np.ndarray
    operators: Optional[np.ndarray] = None

    def __post_init__(self):
        self.kind = np.ascontiguousarray(self.kind, dtype=np.uint8)
        self.a = np.ascontiguousarray(self.a, dtype=np.float64)
        self.b = np.ascontiguousarray(self.b, dtype=np.float64)
        if self.kind.ndim != 2 or self.a.shape != self.kind.shape or self.b.shape != self.kind.shape:
            raise ValueError(f"kind, a and b must share one (N, T) shape, got {self.kind.shape}, {self.a.shape}, {self.b.shape}")
        if self.kind.size and self.kind.max() > OPERATOR:
            raise ValueError("kind holds a value outside 0 .. 4 (EXACT, MISSING, GAUSS, INTERVAL, OPERATOR)")
        g, iv = self.kind == GAUSS, self.kind == INTERVAL
        if np.any(g & ~(np.isfinite(self.a) & np.isfinite(self.b) & (self.b > 0))):
            raise ValueError("a GAUSS site needs a finite value and a positive finite sd")
        if np.any(iv & (np.isnan(self.a) | np.isnan(self.b) | (self.a > self.b))):
            raise ValueError("an INTERVAL site needs lower <= upper")
        if np.any((self.kind == EXACT) & ~np.isfinite(self.a)):
            raise ValueError("an EXACT site needs a finite value: mark it missing instead")
        if np.any(self.kind == OPERATOR):
            if self.operators is None:
                raise ValueError("an OPERATOR site needs ``operators`` (N, T, d, d)")
            op = np.asarray(self.operators)
            if op.ndim != 4 or op.shape[:2] != self.kind.shape or op.shape[2] != op.shape[3]:
                raise ValueError(f"operators must have the shape (N, T, d, d), got {op.shape}")

    @property
    def shape(self):
        return self.kind.shape

    def rows(self, idx):
        return ObservationModel(self.kind[idx], self.a[idx], self.b[idx], None if self.operators is None else np.asarray(self.operators)[idx])


def gaussian_noise(x, sigma, missing_mask=None) -> ObservationModel:
    """Values ``x`` (N, T) observed with Gaussian noise of sd ``sigma`` - a scalar, (T,) or (N, T); ``sigma == 0`` marks an EXACT site;
    ``missing_mask`` (and every non-finite ``x``) a MISSING one."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), x.shape).copy()
    if np.any(~(s >= 0) | ~np.isfinite(s)):
        raise ValueError("sigma must be finite and >= 0")
    miss = ~np.isfinite(x)
    if missing_mask is not None:
        m = np.asarray(missing_mask, dtype=bool)
        if m.shape != x.shape:
            raise ValueError(f"missing_mask must have the shape of x {x.shape}, not {m.shape}")
        miss |= m
    kind = np.where(miss, MISSING, np.where(s == 0, EXACT, GAUSS)).astype(np.uint8)
    return ObservationModel(kind, np.where(miss, 0.0, x), np.where(miss, 0.0, s))


def interval_observations(lower, upper, missing_mask=None) -> ObservationModel:
    """``lower <= x <= upper`` at every site ((N, T) each).  Equal ends are an EXACT value; ``-inf`` / ``+inf`` ends are clipped to the
    grid when the model is used; both ends infinite (or ``missing_mask``) mark a MISSING site."""
    lo = np.atleast_2d(np.asarray(lower, dtype=np.float64))
    hi = np.atleast_2d(np.asarray(upper, dtype=np.float64))
    if lo.shape != hi.shape:
        raise ValueError(f"lower and upper must share a shape, got {lo.shape} and {hi.shape}")
    if np.any(np.isnan(lo) | np.isnan(hi) | (lo > hi)):
        raise ValueError("every interval needs lower <= upper (NaN is not an end)")
    miss = np.isinf(lo) & np.isinf(hi)
    if missing_mask is not None:
        miss = miss | np.asarray(missing_mask, dtype=bool)
    kind = np.where(miss, MISSING, np.where(lo == hi, EXACT, INTERVAL)).astype(np.uint8)
    return ObservationModel(kind, np.where(miss, 0.0, lo), np.where(miss, 0.0, hi))


@dataclass
class ObservedConditionals:
    kind: np.ndarray                        # (N, T)
    a: np.ndarray                           # (N, T) the parameters the device was given (encoding's domain)
    b: np.ndarray
    pred_median: np.ndarray                 # (N, T) of p(x_t | the other sites' observations)
    pred_err: Optional[np.ndarray]          # WMAD, None without get_wmad
    pred_mean: np.ndarray
    pred_quantiles: Optional[np.ndarray]    # (N, T, nq), None without levels
    post_median: np.ndarray                 # (N, T) of p(x_t | all observations); NaN at EXACT and OPERATOR sites
    post_err: Optional[np.ndarray]
    post_mean: np.ndarray
    post_quantiles: Optional[np.ndarray]
    nll_obs: np.ndarray                     # (N, T) -ln(tr(E_t rho_t) / Z)
    pit: np.ndarray                         # (N, T) at EXACT sites, NaN elsewhere
    logev: np.ndarray                       # (N,) ln of the un-normalised chain value under the series' class
    operators: Optional[np.ndarray]         # (N, T, d, d) the operators the walk used, with return_operators
    seconds: float = 0.0


def observed_conditionals_model(eng: SweepEngine, W, phi, label_index, model: ObservationModel, x, grid_x, grid_phi, levels=None,
                                get_wmad=True, label_site=None, return_operators=False, groups=("pred", "post", "score")):
    """mpst_observed_conditionals on arrays: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C); ``phi`` (N, T, d) the
    encoded values, read at EXACT sites (and at MISSING ones where ``x`` is finite); ``label_index`` (N,); ``model`` in the ENCODING'S
    domain; ``x`` (N, T) the values of the EXACT sites (held-out values or NaN at MISSING ones), or None; ``grid_x`` (ngrid,) evenly
    spaced and ``grid_phi`` its states, (ngrid, d) or (T, ngrid, d).  ``groups``: which of the predictive group, the posterior group
    and the scores (nll_obs, pit) are computed; ``logev`` always is.  Returns an ``ObservedConditionals`` (skipped arrays are None)."""
    lv = check_levels(levels)
    cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi) or np.iscomplexobj(grid_phi)
    dt = np.complex128 if cx else np.float64
    mdl, keep = model_to_abi([np.asarray(t, dtype=dt) for t in W], np.asarray(phi, dtype=dt), "f64", label_site)
    N, T, d = int(mdl.N), int(mdl.T), int(mdl.d)
    lab = np.ascontiguousarray(label_index, dtype=np.int32)
    gx = np.ascontiguousarray(grid_x, dtype=np.float64)
    gp = np.ascontiguousarray(grid_phi, dtype=dt)
    xs = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    if model.shape != (N, T):
        raise ValueError(f"the observation model has the shape {model.shape}, the series (N, T) = {(N, T)}")
    assert lab.shape == (N,) and (xs is None or xs.shape == (N, T)) and gp.shape in ((len(gx), d), (T, len(gx), d))
    ops = None
    if np.any(model.kind == OPERATOR):
        ops = np.ascontiguousarray(model.operators, dtype=dt)
        if ops.shape != (N, T, d, d):
            raise ValueError(f"operators must have the shape {(N, T, d, d)}, got {ops.shape}")
    mdl.label_idx = lab.ctypes.data_as(C.POINTER(C.c_int32))
    dp = C.POINTER(C.c_double)
    nq = 0 if lv is None else len(lv)
    o = L.SiteCondOpts(int(gp.ndim == 3), int(bool(get_wmad)), nq, 0, None if lv is None else lv.ctypes.data_as(dp))
    z = lambda on, *s: np.zeros(s) if on else None
    pred, post, score = "pred" in groups, "post" in groups, "score" in groups
    arr = dict(pred_med=z(pred, N, T), pred_err=z(pred and get_wmad, N, T), pred_mean=z(pred, N, T), pred_q=z(pred and nq, N, T, nq),
               post_med=z(post, N, T), post_err=z(post and get_wmad, N, T), post_mean=z(post, N, T), post_q=z(post and nq, N, T, nq),
               nll_obs=z(score, N, T), pit=z(score and xs is not None, N, T), logev=np.zeros(N))
    E = np.zeros((N, T, d, d), dtype=dt) if return_operators else None
    out = L.ObservedOut(**{k: None if v is None else v.ctypes.data_as(dp) for k, v in arr.items()},
                        E_out=None if E is None else C.c_void_p(E.ctypes.data))
    sec = C.c_double()
    eng._chk(eng.lib.mpst_observed_conditionals(eng.ctx, C.byref(mdl), model.kind.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                model.a.ctypes.data_as(dp), model.b.ctypes.data_as(dp),
                                                None if ops is None else C.c_void_p(ops.ctypes.data),
                                                None if xs is None else xs.ctypes.data_as(dp), gx.ctypes.data_as(dp), C.c_void_p(gp.ctypes.data),
                                                len(gx), C.byref(o), C.byref(out), C.byref(sec)))
    del keep
    return ObservedConditionals(model.kind, model.a, model.b, arr["pred_med"], arr["pred_err"], arr["pred_mean"], arr["pred_q"], arr["post_med"],
                                arr["post_err"], arr["post_mean"], arr["post_q"], arr["nll_obs"], arr["pit"], arr["logev"], E, sec.value)


def _transform_slope(imp, norms, raw, oob, enc_range):
    """d(encoded) / d(raw) of the test transform at the raw values ``raw`` (N, T), each row with its own out-of-bounds rescale"""
    s = np.ones_like(raw)
    if norms.sigmoid is not None:
        med, iqr = norms.sigmoid
        sg = 1.0 / (1.0 + np.exp(-(raw - med) / (iqr / 1.35)))
        s = sg * (1.0 - sg) / (iqr / 1.35)
    if norms.minmax is not None:
        lo, hi = norms.minmax
        s = s / (hi - lo)
    if imp.opts.minmax:
        lb, ub = imp.opts.data_bounds
        s = s * (ub - lb)
    for i, _, hi in oob:
        s[int(i)] = s[int(i)] / hi
    a, b = enc_range
    return s * (b - a)


@dataclass
class _Encoded:
    model: ObservationModel     # in the encoding's domain, ends clipped to the grid
    x: np.ndarray               # (N, T) the encoded value at EXACT sites, NaN elsewhere
    states: np.ndarray          # (N, T, d)
    lab: np.ndarray             # (N,)
    enc: object
    norms: object
    oob: list


def encode_observations(imp, model: ObservationModel, rows=None, domain="raw") -> _Encoded:
    """The host half of ``observed_conditionals``: ``model`` (one row per selected series) through imputation's own pre-processing.
    The values of the EXACT and GAUSS sites take the place of ``imp.X_test[rows]`` in ``_scaled_instances`` - every other site is
    filled as a missing one is - so the per-series out-of-bounds rescale sees the series as it was observed.  Interval ends go through
    the same monotone transform exactly and are clipped to the grid; a raw-unit sd is multiplied by the local slope of the transform
    at the observed value: exact when the transform is affine (``sigmoid_transform=False``), the delta method otherwise.
    ``domain="encoded"``: the parameters are taken as they are."""
    from .conditionals import _true_values
    from .imputation import _scaled_instances
    from .encodings import opts_encoding
    if domain not in ("raw", "encoded"):
        raise ValueError(f'domain must be "raw" or "encoded", not {domain!r}')
    rows = np.arange(imp.X_test.shape[0]) if rows is None else np.atleast_1d(np.asarray(rows))
    T = imp.X_test.shape[1]
    if model.shape != (len(rows), T):
        raise ValueError(f"the observation model must have the shape (rows, T) = {(len(rows), T)}, not {model.shape}")
    kind = model.kind
    valued = (kind == EXACT) | (kind == GAUSS)
    lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test)[rows].tolist()], dtype=np.int32)
    xr = imp.x_guess_range
    g0, g1 = float(xr.xvals[0]), float(xr.xvals[-1])
    dx = float(xr.xvals[1] - xr.xvals[0])
    a, b = model.a.copy(), model.b.copy()
    if domain == "raw":
        sub = dataclasses.replace(imp, X_test=np.where(valued, model.a, 0.0), y_test=np.asarray(imp.y_test)[rows])
        enc, norms, raw, _, scaled, oob = _scaled_instances(sub, np.arange(len(rows)), ~valued)
        if len(rows):
            iv = kind == INTERVAL
            a = np.where(valued, scaled, a)
            lo = _true_values(imp, enc, norms, np.where(iv & np.isfinite(model.a), model.a, np.nan), oob)
            hi = _true_values(imp, enc, norms, np.where(iv & np.isfinite(model.b), model.b, np.nan), oob)
            a = np.where(iv, np.where(np.isfinite(model.a), lo, -np.inf), a)
            b = np.where(iv, np.where(np.isfinite(model.b), hi, np.inf), b)
            b = np.where(kind == GAUSS, model.b * _transform_slope(imp, norms, raw, oob, enc.range), b)
    else:
        enc, norms, oob = opts_encoding(imp.opts, imp.custom_encoding), None, []
        scaled = np.where(valued, model.a, 0.5 * (g0 + g1))
    iv = kind == INTERVAL
    a = np.where(iv, np.clip(a, g0, g1), a)
    b = np.where(iv, np.clip(b, g0, g1), b)
    g = kind == GAUSS
    if np.any(g & (b < dx)):
        i, t = np.argwhere(g & (b < dx))[0]
        raise ValueError(f"the noise sd of site ({i}, {t}) is {b[i, t]:.3g} in the encoding's domain, below the grid spacing {dx:.3g}: the "
                         "quadrature cannot resolve it - pass the value as exact (sigma = 0)")
    em = ObservationModel(kind, np.where(valued | iv, a, 0.0), np.where(g | iv, b, 0.0), model.operators)
    x = np.where(kind == EXACT, scaled, np.nan)
    states = imp.encoder(scaled) if len(rows) else np.zeros((0, T, imp.opts.d))
    return _Encoded(em, x, np.asarray(states), lab, enc, norms, oob)


def _with_engine(engine, device, f):
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        return f(eng)
    finally:
        if own:
            eng.close()


def observed_conditionals(imp, model: ObservationModel, rows=None, quantiles=None, get_wmad: bool = True, domain: str = "raw",
                          return_operators: bool = False, engine: Optional[SweepEngine] = None, device: int = 0):
    """The observed conditionals of the series ``model`` describes (one row per entry of ``rows``, default all of ``imp.X_test``; the
    labels are ``imp.y_test[rows]``), each under the MPS of its class: an ``ObservedConditionals`` in the encoding's domain.
    Pre-processing: ``encode_observations``; split and time-dependent encodings go through the fitted encoder and the per-site tables.
    Raises ValueError where a noise sd falls below the grid spacing in the encoding's domain, KeyError on an unknown label."""
    levels = check_levels(quantiles)
    e = encode_observations(imp, model, rows, domain)
    xr = imp.x_guess_range
    if e.model.shape[0] == 0:
        raise ValueError("no series selected")
    return _with_engine(engine, device, lambda eng: observed_conditionals_model(
        eng, imp.mps, e.states, e.lab, e.model, e.x, xr.xvals, xr.xvals_enc, levels=levels, get_wmad=get_wmad, return_operators=return_operators))


def denoise(imp, sigma, rows=None, statistic: str = "median", quantiles=(0.05, 0.95), invert_transform: bool = True, missing_mask=None,
            engine: Optional[SweepEngine] = None, device: int = 0):
    """``imp.X_test[rows]`` read as noisy observations with sd ``sigma`` (scalar, (T,) or (rows, T), raw units; 0: exact, kept as it
    is): the posterior ``statistic`` - ``"median"`` or ``"mean"`` - of every site given ALL observations, and its bands.  Returns
    ``(X_denoised (N, T), bands (N, T, nq))``, in the original units with ``invert_transform``.  Bands and the median commute with that
    monotone transform; the MEAN does not - the mean of the encoding's domain is mapped, which is not the mean in the original units
    under a nonlinear transform (the sigmoid), as in ``impute_marginal``.  Non-finite values and ``missing_mask`` are missing sites:
    they get the predictive distribution."""
    from .imputation import invert_test_transform
    if statistic not in ("median", "mean"):
        raise ValueError(f'statistic must be "median" or "mean", not {statistic!r}')
    rows = np.arange(imp.X_test.shape[0]) if rows is None else np.atleast_1d(np.asarray(rows))
    model = gaussian_noise(np.asarray(imp.X_test, dtype=np.float64)[rows], sigma, missing_mask)
    levels = check_levels(quantiles)
    e = encode_observations(imp, model, rows, "raw")
    xr = imp.x_guess_range
    oc = _with_engine(engine, device, lambda eng: observed_conditionals_model(
        eng, imp.mps, e.states, e.lab, e.model, e.x, xr.xvals, xr.xvals_enc, levels=levels, get_wmad=False, groups=("post",)))
    exact = model.kind == EXACT
    ts = np.where(exact, e.x, oc.post_median if statistic == "median" else oc.post_mean)
    bands = None if oc.post_quantiles is None else np.where(exact[:, :, None], e.x[:, :, None], oc.post_quantiles)
    if invert_transform:
        ts = invert_test_transform(ts, e.oob, e.norms, imp.opts, e.enc.range)
        if bands is not None:
            bands = np.stack([invert_test_transform(bands[:, :, l], e.oob, e.norms, imp.opts, e.enc.range) for l in range(bands.shape[2])], axis=2)
    return ts, bands


def noisy_log_likelihoods(imp, model: ObservationModel, rows=None, normalise_classes: bool = False, domain: str = "raw",
                          engine: Optional[SweepEngine] = None, device: int = 0):
    """ln of the un-normalised chain value of every series under EVERY class, (N, C), columns in the order of the training labels:
    ``logev`` of the series replicated once per class with ``label_index = 0 .. C-1``.  One row of MISSING sites per class travels
    along and gives ``ln ||W_c||^2``; ``normalise_classes`` subtracts it (the likelihood under the normalised class MPS).  The labels
    ``imp.y_test`` are not used.  With EXACT kinds only this is ``ln |<phi|W_c>|^2``, what ``classify`` compares."""
    rows = np.arange(imp.X_test.shape[0]) if rows is None else np.atleast_1d(np.asarray(rows))
    e = encode_observations(dataclasses.replace(imp, y_test=np.full(imp.X_test.shape[0], next(iter(imp.class_map)))), model, rows, domain)
    N, T = e.model.shape
    Cn = len(imp.class_map)
    if N == 0:
        return np.zeros((0, Cn))
    rep = lambda v, fill: np.concatenate([np.tile(v, (Cn,) + (1,) * (v.ndim - 1)), np.full((Cn,) + v.shape[1:], fill, dtype=v.dtype)])
    ops = None if e.model.operators is None else rep(np.asarray(e.model.operators), 0)
    big = ObservationModel(rep(e.model.kind, MISSING), rep(e.model.a, 0.0), rep(e.model.b, 0.0), ops)
    lab = np.concatenate([np.repeat(np.arange(Cn, dtype=np.int32), N), np.arange(Cn, dtype=np.int32)])
    states = rep(e.states, 0)
    xr = imp.x_guess_range
    oc = _with_engine(engine, device, lambda eng: observed_conditionals_model(
        eng, imp.mps, states, lab, big, None, xr.xvals, xr.xvals_enc, get_wmad=False, groups=()))
    lev = oc.logev[:Cn * N].reshape(Cn, N).T
    return lev - oc.logev[Cn * N:][None, :] if normalise_classes else lev


def noisy_class_posteriors(imp, model: ObservationModel, rows=None, domain: str = "raw", engine: Optional[SweepEngine] = None, device: int = 0):
    """p(c | observations) under a uniform prior over classes: the softmax of ``noisy_log_likelihoods`` over the classes, (N, C).  A
    row that is -inf in every class is a NaN row."""
    lp = noisy_log_likelihoods(imp, model, rows, domain=domain, engine=engine, device=device)
    with np.errstate(invalid="ignore"):
        w = np.exp(lp - lp.max(axis=1, keepdims=True))
        return w / w.sum(axis=1, keepdims=True)


def classify_noisy(imp, model: ObservationModel, rows=None, domain: str = "raw", engine: Optional[SweepEngine] = None, device: int = 0):
    """The label (original label values) of the largest ``noisy_log_likelihoods``."""
    labels = np.array(sorted(imp.class_map, key=imp.class_map.get))
    lp = noisy_log_likelihoods(imp, model, rows, domain=domain, engine=engine, device=device)
    if lp.shape[0] == 0:
        return np.zeros(0, dtype=labels.dtype)
    return labels[np.argmax(lp, axis=1)]
