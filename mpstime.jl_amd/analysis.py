"""Analysis API of the reference (src/Analysis/analyse.jl): entanglement entropies of a trained model on the device.

``bipartite_spectrum`` (the bipartite entanglement entropy at every bond of each class MPS), ``single_site_spectrum`` (the
von Neumann entropy of every site's one-site reduced density matrix) and ``see_variation`` (the single-site entropies after
the first k sites of an instance have been measured, for every k) keep the reference's names and argument meaning.  The
work runs in ``mpst_entanglement`` / ``mpst_see_variation`` (csrc/mpst_analysis.hip); the pre-processing of the measured
series is the imputation engine's (imputation._scaled_instances), and the log base is changed on the host.

One intended divergence: an eigenvalue of a reduced density matrix that is exactly 0 (and not clamped by rho_correct)
contributes 0 to the entropy, where the reference's matrix ``log`` would give NaN.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .encodings import fit_encoding_from_training_data, transform_test_data, transform_train_data
from .engine import SweepEngine, label_site_of, model_to_abi
from .options import safe_options

_LOGS = {"log": 1.0, "log2": 1.0 / math.log(2.0), "log10": 1.0 / math.log(10.0)}
_LOGFN = {np.log: "log", np.log2: "log2", np.log10: "log10", math.log: "log", math.log2: "log2", math.log10: "log10"}


def _log_scale(logfn) -> float:
    name = logfn if isinstance(logfn, str) else _LOGFN.get(logfn)
    if name not in _LOGS:
        raise ValueError("logfn must be one of: log, log2, or log10")
    return _LOGS[name]


class _Model:
    """The model of ``W`` as an ``mpst_impute_model`` (the buffers stay alive with this object).  Refuses complex models
    before anything reaches the device: the reference's analysis is Float64-only."""

    def __init__(self, W, phi=None):
        mps = W.mps if hasattr(W, "mps") else W
        if any(np.iscomplexobj(t) for t in mps):
            raise ValueError("entanglement analysis of a complex-valued MPS is not supported (the reference computes it in Float64 only)")
        self.struct, self._keep = model_to_abi(mps, phi, label_site=label_site_of(mps, ValueError))
        self.T, self.C = int(self.struct.T), int(self.struct.C)


def _check(lib, ctx, rc):
    if rc:
        msg = (lib.mpst_last_error(ctx) or b"").decode()
        raise (L.DomainError if rc == L.MPST_ERR_DOMAIN else L.SVDError if rc == L.MPST_ERR_SVD else L.MPSTError)(rc, msg)


def _entanglement(W, engine: Optional[SweepEngine], device: int):
    m = _Model(W)
    bee, see = np.zeros((m.C, m.T)), np.zeros((m.C, m.T))
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        dp = C.POINTER(C.c_double)
        _check(eng.lib, eng.ctx, eng.lib.mpst_entanglement(eng.ctx, C.byref(m.struct), bee.ctypes.data_as(dp), see.ctypes.data_as(dp)))
    finally:
        if own:
            eng.close()
    return bee, see


def bipartite_spectrum(W, logfn="log", engine: Optional[SweepEngine] = None, device: int = 0):
    """bipartite_spectrum(mps::TrainedMPS; logfn) (analyse.jl:47-64): one array of length T per class; entry i < T-1 is the
    entanglement entropy across the bond between sites i and i+1, entry T-1 repeats entry T-2 (the reference's last cut is the
    same bond).  Only Schmidt weights p > 1e-12 contribute.  ``logfn``: "log", "log2", "log10" or np.log / np.log2 /
    np.log10; anything else is a ValueError (Julia: ArgumentError)."""
    scale = _log_scale(logfn)
    bee, _ = _entanglement(W, engine, device)
    return [row * scale if scale != 1.0 else row for row in bee]


def single_site_spectrum(W, engine: Optional[SweepEngine] = None, device: int = 0):
    """single_site_spectrum(mps::TrainedMPS) (analyse.jl:122-138): one array of length T per class, the von Neumann entropy
    (natural log) of every site's one-site reduced density matrix after rho_correct.  Raises DomainError where that fails."""
    _, see = _entanglement(W, engine, device)
    return list(see)


def see_variation(W, measure_series, cls: int = 0, engine: Optional[SweepEngine] = None, device: int = 0, return_seconds=False):
    """see_variation(mps::TrainedMPS, measure_series, class) (analyse.jl:168-194): an (n, T, T) array whose [i, k, j] is the
    single-site entropy at site j of class ``cls``'s MPS after sites 0..k-1 were measured at series i's values (row 0: the
    unmeasured spectrum; zero at sites j < k).  The series are unscaled; they are transformed with the training data's
    normalisations and encoded with the model's encoding, as the imputation engine does.  (The reference's docstring names
    the last two dimensions the other way round; this follows its code.)"""
    X = np.asarray(measure_series, dtype=np.float64)
    if X.ndim == 1:
        X = X[None, :]
    mps = W.mps
    if any(np.iscomplexobj(t) for t in mps):
        raise ValueError("entanglement analysis of a complex-valued MPS is not supported (the reference computes it in Float64 only)")
    T = len(mps)
    Cn = int(mps[label_site_of(mps, ValueError)].shape[3])
    if not 0 <= int(cls) < Cn:
        raise ValueError(f"class {cls} out of range: the model has {Cn} classes (0-based)")
    if X.ndim != 2 or X.shape[1] != T:
        raise ValueError(f"measure_series must be (n, {T}): one series of the model's length per row, got shape {X.shape}")
    if X.shape[0] == 0:
        return np.zeros((0, T, T))
    opts = safe_options(W.opts)
    enc, _, encoder = fit_encoding_from_training_data(opts, W.train_data.original_data, W.train_data.labels, getattr(W, "custom_encoding", None))
    _, norms = transform_train_data(W.train_data.original_data, opts, enc.range)
    scaled, _ = transform_test_data(X, norms, opts, enc.range)
    phi = encoder(scaled)
    if np.iscomplexobj(phi):
        raise ValueError(f"entanglement analysis with the complex encoding {enc.name} is not supported (Float64 only)")
    m = _Model(W, phi)
    out = np.zeros((X.shape[0], T, T))
    sec = C.c_double()
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        _check(eng.lib, eng.ctx, eng.lib.mpst_see_variation(eng.ctx, C.byref(m.struct), int(cls), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                            C.byref(sec)))
    finally:
        if own:
            eng.close()
    return (out, sec.value) if return_seconds else out


# ---------------------------------------------------------------------------------------
# pair analysis (mpst_pair_analysis): which sites has the model coupled to which
# ---------------------------------------------------------------------------------------
PAIR_MI_MAX_D = 11      # the pair matrix is d^2 x d^2 and the device's in-workgroup Jacobi holds n <= 128


@dataclass
class PairAnalysis:
    """Result of ``pair_analysis``: ``mutual_information`` (C, T, T) - I(i:j) off the diagonal, the single-site entropies S(rho_i)
    on it, in the base of ``logfn`` - and, under the observable, ``mean`` (C, T), ``covariance`` (C, T, T) and ``correlation``
    (C, T, T) = covariance over the product of the roots of its diagonal, NaN where a variance is not positive.  A field that was
    not computed is None."""
    mutual_information: Optional[np.ndarray]
    mean: Optional[np.ndarray]
    covariance: Optional[np.ndarray]
    correlation: Optional[np.ndarray]
    seconds: float = 0.0


def position_operator(W, npoints: int = 2001):
    """The position observable of every site in the model's encoding, (T, d, d):
    X_t[s, s'] = integral over the encoding's range of x phi_{t,s}(x) phi_{t,s'}(x) dx, by the composite trapezoid rule on
    ``npoints`` evenly spaced values, through the encoder fitted from the model's training data (as ``see_variation`` encodes), so
    split and time-dependent bases need nothing further.  For a basis orthonormal on the range, tr(rho_t X_t) is the model's mean
    of the (scaled) series at site t."""
    opts = safe_options(W.opts)
    enc, _, encoder = fit_encoding_from_training_data(opts, W.train_data.original_data, W.train_data.labels, getattr(W, "custom_encoding", None))
    T = len(W.mps)
    a, b = enc.range
    x = np.linspace(a, b, int(npoints))
    tab = np.asarray(encoder.table(x, T))
    if np.iscomplexobj(tab):
        raise ValueError(f"entanglement analysis with the complex encoding {enc.name} is not supported (Float64 only)")
    if tab.ndim == 2:
        tab = np.broadcast_to(tab, (T,) + tab.shape)
    w = np.full(x.shape, (b - a) / (len(x) - 1))
    w[0] *= 0.5
    w[-1] *= 0.5
    X = np.einsum("n,tns,tnu->tsu", w * x, tab, tab)
    return np.ascontiguousarray(0.5 * (X + X.transpose(0, 2, 1)))


def _correlation(cov):
    var = np.diagonal(cov, axis1=1, axis2=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.where(var > 0.0, np.sqrt(np.where(var > 0.0, var, 1.0)), np.nan)
        return cov / (sd[:, :, None] * sd[:, None, :])


def pair_analysis(W, observable="position", logfn="log", engine: Optional[SweepEngine] = None, device: int = 0, return_seconds=False):
    """Pairwise diagnostics of every class MPS on the device (``mpst_pair_analysis``): the two-site reduced density matrix rho_ij
    of every pair of sites gives the mutual information I(i:j) = S(rho_i) + S(rho_j) - S(rho_ij) and, under a real symmetric
    observable O, the model's mean tr(rho_i O_i) and covariance tr(rho_ij O_i (x) O_j) - mean_i mean_j.

    ``observable``: "position" (``position_operator(W)``, one table per site), a (d, d) array for all sites, a (T, d, d) array, or
    None (no moments: those fields are None).  ``logfn`` scales the entropies on the host, as ``bipartite_spectrum`` does.  The
    other sites are marginalised by summing their physical index (the convention of ``log_marginals``): that is the model's
    distribution exactly for encodings that are orthonormal on their domain.  The entropy of a density matrix is
    -sum lam ln lam over the positive eigenvalues of its symmetric part: no rho_correct, no threshold, so the call cannot raise a
    DomainError.  For d > 11 ``mutual_information`` is None (with a warning): the moments have no such limit."""
    scale = _log_scale(logfn)
    m = _Model(W)
    T, Cn, d = m.T, m.C, int(m.struct.d)
    obs = None
    if observable is not None:
        obs = position_operator(W) if isinstance(observable, str) and observable == "position" else np.asarray(observable, dtype=np.float64)
        if isinstance(observable, str) and observable != "position":
            raise ValueError('observable must be "position", an array or None')
        if obs.shape not in ((d, d), (T, d, d)):
            raise ValueError(f"observable must be ({d}, {d}) or ({T}, {d}, {d}), got {obs.shape}")
        if not np.allclose(obs, np.swapaxes(obs, -1, -2), rtol=0, atol=1e-12 * max(1.0, float(np.abs(obs).max()))):
            raise ValueError("observable must be symmetric")
        obs = np.ascontiguousarray(obs)
    want_mi = d <= PAIR_MI_MAX_D
    if not want_mi:
        warnings.warn(f"mutual_information is not computed for d = {d} > {PAIR_MI_MAX_D} (the pair matrix is d^2 x d^2)", RuntimeWarning,
                      stacklevel=2)
    if not want_mi and obs is None:
        return (PairAnalysis(None, None, None, None), 0.0) if return_seconds else PairAnalysis(None, None, None, None)
    mi = np.zeros((Cn, T, T)) if want_mi else None
    mean = np.zeros((Cn, T)) if obs is not None else None
    cov = np.zeros((Cn, T, T)) if obs is not None else None
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None
    sec = C.c_double()
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        _check(eng.lib, eng.ctx, eng.lib.mpst_pair_analysis(eng.ctx, C.byref(m.struct), ptr(obs), int(obs is not None and obs.ndim == 3),
                                                            ptr(mi), ptr(mean), ptr(cov), C.byref(sec)))
    finally:
        if own:
            eng.close()
    if mi is not None and scale != 1.0:
        mi = mi * scale
    out = PairAnalysis(mi, mean, cov, _correlation(cov) if cov is not None else None, sec.value)
    return (out, sec.value) if return_seconds else out


def mutual_information(W, logfn="log", engine: Optional[SweepEngine] = None, device: int = 0):
    """One (T, T) matrix per class: I(i:j) off the diagonal, S(rho_i) on it (``pair_analysis`` without an observable)."""
    return list(pair_analysis(W, observable=None, logfn=logfn, engine=engine, device=device).mutual_information)


def model_correlations(W, observable="position", engine: Optional[SweepEngine] = None, device: int = 0):
    """(mean, correlation): per class, the model's mean series (T,) and correlation matrix (T, T) under ``observable``."""
    r = pair_analysis(W, observable=observable, engine=engine, device=device)
    return list(r.mean), list(r.correlation)
