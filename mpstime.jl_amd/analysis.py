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
    enc, _, encoder = fit_encoding_from_training_data(opts, W.train_data.original_data, W.train_data.labels)
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
