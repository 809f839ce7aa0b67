"""Marginal likelihoods of incomplete series on the device (``mpst_marginal_model``, csrc/mpst_marginal.inl).

The trained MPS is a generative model of whole series.  ``classify`` scores complete ones, the imputation engine conditions a
class MPS on the known values of an incomplete one and traces the missing sites out; ``log_marginals`` is the number that joins
the two: for every instance and every class c the natural log of

    l_c = sum over s_j, j missing, of | < (x)_{j known} phi_j  (x)_{j missing} e_{s_j} | W_c > |^2,

the squared norm of what ``precondition`` (src/Imputation/MPS_methods.jl:42-99) leaves behind for the label slice ``W_c`` of the
model as stored.  This is the Born rule on the known values, not the ``|rho phi|^2`` convention of the imputed densities.
``class_posteriors`` and ``classify(..., missing_mask=)`` are read off it.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .encodings import EncodedTimeSeriesSet
from .engine import SweepEngine, model_to_abi
from .options import safe_options


model_struct = model_to_abi       # (mpst_impute_model without label_idx, the arrays it points into) of (W, phi, compute, label_site)


def marginal_model(eng: SweepEngine, W, phi, missing, compute="f64", label_site=None):
    """mpst_marginal_model on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) encoded values, real or complex, not read where ``missing`` (N, T) is set (NaN allowed there);
    ``missing`` None: nothing missing.  Returns (logp (N, C), seconds): ln l_c, -inf where l_c is zero."""
    model, keep = model_struct(W, phi, compute, label_site)
    N, T, Cn = int(model.N), int(model.T), int(model.C)
    m = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    assert m is None or m.shape == (N, T)
    logp, sec = np.zeros((N, Cn)), C.c_double()
    eng._chk(eng.lib.mpst_marginal_model(eng.ctx, C.byref(model), None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         logp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sec)))
    del keep
    return logp, sec.value


def marginal_states(mps, X, missing_mask):
    """(phi (N, T, d), mask (N, T) bool) of a ``log_marginals`` call, checked: ``X`` an EncodedTimeSeriesSet (the mask in the
    set's order) or raw series, which go through imputation's pre-processing (``imputation._scaled_instances``, imputation.jl:283-297:
    masked entries are overwritten with the training mean BEFORE the test transform, so its per-series out-of-bounds rescale sees
    what imputation would see) and the encoder fitted from the training data.  Raises ValueError on a mask of another shape and on
    a non-finite value at an unmasked position; values at masked positions may be anything."""
    from .imputation import ImputationProblem, _scaled_instances
    from .encodings import fit_encoding_from_training_data
    mask = np.asarray(missing_mask)
    if mask.dtype != bool:
        mask = mask != 0
    if isinstance(X, EncodedTimeSeriesSet):
        phi = np.asarray(X.phi)
        if phi.ndim != 3 or mask.shape != phi.shape[:2]:
            raise ValueError(f"missing_mask has shape {mask.shape}, the encoded set holds {phi.shape[:2]} (instances, sites)")
        if not np.all(np.isfinite(phi[~mask])):
            raise ValueError("the encoded set holds a non-finite state at an unmasked position")
        return phi, mask
    raw = np.asarray(X, dtype=np.float64)
    if raw.ndim != 2 or mask.shape != raw.shape:
        raise ValueError(f"missing_mask has shape {mask.shape}, X has shape {raw.shape}")
    if not np.all(np.isfinite(raw[~mask])):
        raise ValueError("X holds a NaN or non-finite value at an unmasked position: mask it or remove it")
    opts = safe_options(mps.opts)
    td = mps.train_data
    custom = getattr(mps, "custom_encoding", None)
    encoder = fit_encoding_from_training_data(opts, td.original_data, td.labels, custom)[2]
    filled = np.where(mask, np.mean(td.original_data), raw)          # (the unmasked transform of _scaled_instances must not see NaN)
    imp = ImputationProblem(mps.mps, td.original_data, np.asarray(td.labels), filled, np.zeros(len(filled), dtype=np.int64), opts, None,
                            {}, encoder, custom)
    scaled = _scaled_instances(imp, np.arange(len(filled)), mask)[4]
    return np.asarray(encoder(scaled)), mask


def log_marginals(mps, X, missing_mask, normalise_classes: bool = False, compute: str = "f64", engine: Optional[SweepEngine] = None,
                  device: int = 0, return_seconds: bool = False):
    """ln l_c(i) of the known values of every series under every class, the sites where ``missing_mask`` is set marginalised:
    (N, C), columns in the order of ``np.unique(train labels)``, -inf where the likelihood is zero.  ``X``: raw series (N, T) or an
    EncodedTimeSeriesSet (see ``marginal_states``).  The class MPS is the label slice of the model as stored;
    ``normalise_classes=True`` subtracts ln ||W_c||^2 - the all-missing row, obtained in the same call - which gives the
    likelihood under ``expand_label_index``'s normalised class MPS, the model imputation conditions on.  Split and
    time-dependent encodings go through the same encoder as everywhere else."""
    phi, mask = marginal_states(mps, X, missing_mask)
    if compute not in ("f64", "f32"):
        raise ValueError('compute must be "f64" or "f32"')
    N = phi.shape[0]
    Cn = int(mps.mps[-1].shape[3])
    if N == 0:
        out = np.zeros((0, Cn))
        return (out, 0.0) if return_seconds else out
    if normalise_classes:
        phi = np.concatenate([phi, np.zeros((1,) + phi.shape[1:], dtype=phi.dtype)])
        mask = np.concatenate([mask, np.ones((1, mask.shape[1]), dtype=bool)])
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        logp, secs = marginal_model(eng, mps.mps, phi, mask, compute=compute)
    finally:
        if own:
            eng.close()
    if normalise_classes:
        logp = logp[:N] - logp[N]
    return (logp, secs) if return_seconds else logp


def class_posteriors(mps, X, missing_mask, compute: str = "f64", engine: Optional[SweepEngine] = None, device: int = 0):
    """p(c | known values) under a uniform prior over classes: the softmax of the unnormalised ``log_marginals`` over the classes,
    (N, C).  A row that is -inf in every class is a NaN row."""
    lp = log_marginals(mps, X, missing_mask, compute=compute, engine=engine, device=device)
    with np.errstate(invalid="ignore"):
        w = np.exp(lp - lp.max(axis=1, keepdims=True))
        return w / w.sum(axis=1, keepdims=True)


def classify_incomplete(mps, X, missing_mask, engine: Optional[SweepEngine] = None, device: int = 0):
    """``classify(..., missing_mask=)``: the label (original label values) of the largest marginal likelihood."""
    labels = np.unique(mps.train_data.labels)
    lp = log_marginals(mps, X, missing_mask, engine=engine, device=device)
    if lp.shape[0] == 0:
        return np.zeros(0, dtype=labels.dtype)
    return labels[np.argmax(lp, axis=1)]
