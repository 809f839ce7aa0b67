"""Prefix marginals on the device (``mpst_prefix_marginals``, csrc/mpst_prefix.inl): how early a classifier can decide, and how
surprising a sample is given only what came before it.

For every series, every prefix length t = 0 .. T and every class c,

    lp[i, t, c] = ln l_c(i; t),   l_c(i; t) = sum over s_t .. s_{T-1} of | < phi_0 .. phi_{t-1} e_{s_t} .. e_{s_{T-1}} | W_c > |^2,

the number ``log_marginals`` gives for the suffix mask ``mask[:, t:] = True`` - the Born rule on the known values, for the label slice
``W_c`` of the model as stored - for all T + 1 masks from one walk per series.  ``lp[:, 0]`` is ln ||W_c||^2 whatever the series,
``lp[:, T]`` the complete series.

Everything after the device call is NumPy on that array: ``posteriors_from``, ``early_decisions``, ``accuracy_curve_from`` and
``causal_scores_from`` take an ``lp`` array and nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from .encodings import EncodedTimeSeriesSet
from .engine import SweepEngine, model_to_abi
from .marginal import marginal_states


class EarlyClassification(NamedTuple):
    labels: np.ndarray          # (N,) the decided label, in the original label values
    lengths: np.ndarray         # (N,) the prefix length at which it was decided; T where no prefix reached the threshold
    posteriors: np.ndarray      # (N, C) the class posteriors at that length


def prefix_model(eng: SweepEngine, W, phi, compute="f64", label_site=None):
    """mpst_prefix_marginals on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) encoded values, real or complex, all of them read.  Returns (lp (N, T + 1, C), seconds): ln l_c(i; t), -inf
    where the likelihood is zero."""
    model, keep = model_to_abi(W, phi, compute, label_site)
    N, T, Cn = int(model.N), int(model.T), int(model.C)
    lp, sec = np.zeros((N, T + 1, Cn)), C.c_double()
    eng._chk(eng.lib.mpst_prefix_marginals(eng.ctx, C.byref(model), lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sec)))
    del keep
    return lp, sec.value


# ---- NumPy on an lp array -----------------------------------------------------------------------------------------------------------
def posteriors_from(lp):
    """The softmax of ``lp`` (..., C) over the classes: p(c | prefix) under a uniform prior.  A row that is -inf (or NaN) in every
    class is a NaN row."""
    lp = np.asarray(lp, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(lp - np.max(lp, axis=-1, keepdims=True))
        return w / np.sum(w, axis=-1, keepdims=True)


def early_decisions(lp, threshold=0.9, min_length=1):
    """The decision rule of ``classify_early`` on ``lp`` (N, T + 1, C): for every series the first prefix length t >= ``min_length``
    whose largest posterior is >= ``threshold``, and the class index there (the lowest index on a tie); where no prefix qualifies -
    a NaN row never does - the length is T and the class the arg-max of ``lp[:, T]``.  Returns (class index (N,), length (N,),
    posteriors at that length (N, C)).  ``min_length`` outside 0 .. T is a ValueError."""
    lp = np.asarray(lp, dtype=np.float64)
    if lp.ndim != 3 or lp.shape[1] < 1:
        raise ValueError(f"lp must be (N, T + 1, C), got {lp.shape}")
    N, T = lp.shape[0], lp.shape[1] - 1
    if not 0 <= int(min_length) <= T:
        raise ValueError(f"min_length must lie in 0 .. T = {T} (got {min_length})")
    post = posteriors_from(lp)
    with np.errstate(invalid="ignore"):
        ok = np.max(post, axis=2) >= threshold          # (NaN compares false)
    ok[:, :int(min_length)] = False
    lengths = np.where(ok.any(axis=1), np.argmax(ok, axis=1), T).astype(np.int64)
    rows = np.arange(N)
    at = lp[rows, lengths]
    cls = np.argmax(np.where(np.isnan(at), -np.inf, at), axis=1) if N else np.zeros(0, dtype=np.int64)
    return cls.astype(np.int64), lengths, post[rows, lengths]


def accuracy_curve_from(lp, y_index):
    """(T + 1,): the share of series whose arg-max class of ``lp[:, t]`` (the lowest index on a tie) equals ``y_index`` (N,), at every
    prefix length.  NaN for an empty set."""
    lp = np.asarray(lp, dtype=np.float64)
    y = np.asarray(y_index)
    if lp.ndim != 3 or y.shape != lp.shape[:1]:
        raise ValueError(f"lp must be (N, T + 1, C) and y_index (N,), got {lp.shape} and {y.shape}")
    if lp.shape[0] == 0:
        return np.full(lp.shape[1], np.nan)
    pred = np.argmax(np.where(np.isnan(lp), -np.inf, lp), axis=2)
    return np.mean(pred == y[:, None], axis=0)


def causal_scores_from(lp, label_index=None):
    """(N, T): ``lp[:, t, c] - lp[:, t + 1, c]`` at each series' class ``label_index[i]``, or - None - the same difference of
    ``logsumexp_c lp[:, t]``, the posterior mixture.  Where the later prefix has zero likelihood the score is +inf; where the earlier
    one has too, NaN."""
    lp = np.asarray(lp, dtype=np.float64)
    if lp.ndim != 3:
        raise ValueError(f"lp must be (N, T + 1, C), got {lp.shape}")
    if label_index is None:
        m = np.max(lp, axis=2, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        with np.errstate(divide="ignore"):
            a = np.log(np.sum(np.exp(lp - m), axis=2)) + m[..., 0]
    else:
        idx = np.asarray(label_index, dtype=np.int64)
        if idx.shape != lp.shape[:1] or (idx.size and (idx.min() < 0 or idx.max() >= lp.shape[2])):
            raise ValueError("label_index must be (N,) class indices in 0 .. C - 1")
        a = lp[np.arange(lp.shape[0]), :, idx]
    with np.errstate(invalid="ignore"):
        return a[:, :-1] - a[:, 1:]


# ---- the public calls -----------------------------------------------------------------------------------------------------------------
def prefix_log_marginals(mps, X, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0,
                         return_seconds: bool = False):
    """ln l_c(i; t) of the first t values of every series under every class, the rest of the series marginalised: (N, T + 1, C),
    columns in the order of ``np.unique(train labels)``, -inf where the likelihood is zero.  ``X``: raw series (N, T) or an
    EncodedTimeSeriesSet, as in ``log_marginals`` with nothing masked.  ``normalise_classes=True`` subtracts the t = 0 row,
    ln ||W_c||^2, which gives the likelihood under the normalised class MPS - the meaning it has in ``log_marginals``."""
    shape = np.asarray(X.phi).shape[:2] if isinstance(X, EncodedTimeSeriesSet) else np.shape(X)
    phi, _ = marginal_states(mps, X, np.zeros(shape, dtype=bool))
    N, T = phi.shape[:2]
    Cn = int(mps.mps[-1].shape[3])
    if N == 0:
        out = np.zeros((0, T + 1, Cn))
        return (out, 0.0) if return_seconds else out
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        lp, secs = prefix_model(eng, mps.mps, phi)
    finally:
        if own:
            eng.close()
    if normalise_classes:
        lp = lp - lp[:, :1]
    return (lp, secs) if return_seconds else lp


def prefix_posteriors(mps, X, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0,
                      return_seconds: bool = False):
    """p(c | first t values) under a uniform prior over classes, at every prefix length: (N, T + 1, C), the softmax of
    ``prefix_log_marginals`` over the classes.  A row that is -inf in every class is a NaN row, as in ``class_posteriors``."""
    lp, secs = prefix_log_marginals(mps, X, normalise_classes, engine=engine, device=device, return_seconds=True)
    post = posteriors_from(lp)
    return (post, secs) if return_seconds else post


def classify_early(mps, X, threshold: float = 0.9, min_length: int = 1, normalise_classes: bool = False,
                   engine: Optional[SweepEngine] = None, device: int = 0, return_seconds: bool = False):
    """Decide every series as early as the model is sure: ``EarlyClassification(labels, lengths, posteriors)`` with, per series, the
    first prefix length t >= ``min_length`` whose largest class posterior is >= ``threshold``, the label of that class (original
    label values) and the posteriors there.  Where no prefix qualifies ``lengths`` is T and the label the arg-max at T - what
    ``classify`` returns."""
    labels = np.unique(mps.train_data.labels)
    lp, secs = prefix_log_marginals(mps, X, normalise_classes, engine=engine, device=device, return_seconds=True)
    cls, lengths, post = early_decisions(lp, threshold, min_length)
    out = EarlyClassification(labels[cls] if len(cls) else np.zeros(0, dtype=labels.dtype), lengths, post)
    return (out, secs) if return_seconds else out


def early_accuracy_curve(mps, X, y, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0,
                         return_seconds: bool = False):
    """(T + 1,): the accuracy of the arg-max class at every prefix length against the labels ``y`` (original label values)."""
    labels = np.unique(mps.train_data.labels)
    y = np.asarray(y)
    idx = np.searchsorted(labels, y)
    idx = np.where((idx < len(labels)) & (labels[np.minimum(idx, len(labels) - 1)] == y), idx, -1)      # an unknown label matches no class
    lp, secs = prefix_log_marginals(mps, X, normalise_classes, engine=engine, device=device, return_seconds=True)
    curve = accuracy_curve_from(lp, idx)
    return (curve, secs) if return_seconds else curve


def causal_scores(mps, X, labels=None, engine: Optional[SweepEngine] = None, device: int = 0, return_seconds: bool = False):
    """(N, T): how surprising x_t is given only x_0 .. x_{t-1}: ``lp[:, t, c] - lp[:, t + 1, c]`` under the class of ``labels[i]``
    (original label values), or - ``labels=None`` - under the posterior mixture, ``logsumexp_c lp[:, t] - logsumexp_c lp[:, t + 1]``.

    Convention: this is minus the log of the Born weight of the encoded state phi(x_t), the convention of ``log_marginals`` - not a
    density on a grid of values.  For unit-norm states the weight is at most one (Cauchy-Schwarz), so the score is non-negative,
    and it sums over t to ``lp[:, 0] - lp[:, T]``."""
    idx = None
    if labels is not None:
        known = np.unique(mps.train_data.labels)
        y = np.asarray(labels)
        idx = np.searchsorted(known, y)
        if y.size and (np.any(idx >= len(known)) or np.any(known[np.minimum(idx, len(known) - 1)] != y)):
            raise ValueError("labels holds a value that is not a class of the model")
    lp, secs = prefix_log_marginals(mps, X, engine=engine, device=device, return_seconds=True)
    s = causal_scores_from(lp, idx)
    return (s, secs) if return_seconds else s
