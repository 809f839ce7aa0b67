"""Segment marginals on the device (``mpst_segment_marginals``, csrc/mpst_segment.inl): which stretch of a series carries the class
evidence, and at what scale.

For every series, every start a, every width w = 1 .. max_width with a + w <= T and every class c,

    lp[i, a, w - 1, c] = ln l_c(i; a, w),   l_c(i; a, w) = sum over s_j, j outside a .. a+w-1, of | < phi_a .. phi_{a+w-1} (x) e_s | W_c > |^2,

the number ``log_marginals`` gives for the mask that is set everywhere but on the segment - the Born rule on the segment's values alone,
for the label slice ``W_c`` of the model as stored - for all starts and widths from one walk of ``max_width`` steps per (series, start).
Entries with a + w > T are NaN; ``lp[:, 0, T - 1]`` (``max_width = T``) is the complete series.

Everything after the device call is NumPy on that array: ``prefix.posteriors_from``, ``evidence_from``, ``best_segment_from`` and
``accuracy_map_from`` take an ``lp`` array and class indices, and nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from .encodings import EncodedTimeSeriesSet
from .engine import SweepEngine, model_to_abi
from .marginal import marginal_states
from .prefix import posteriors_from


class BestSegment(NamedTuple):
    start: np.ndarray           # (N,) the first site of the segment
    width: np.ndarray           # (N,) its number of sites
    posterior: np.ndarray       # (N,) the posterior of the series' class from that segment alone; NaN where no segment has one


def segment_model(eng: SweepEngine, W, phi, max_width, label_site=None):
    """mpst_segment_marginals on a model handed over in one call: ``W`` site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C);
    ``phi`` (N, T, d) encoded values, real or complex, all of them read; ``max_width`` in 1 .. T.  Returns (lp (N, T, max_width, C),
    lnorm (C,), seconds): ln l_c(i; a, w) - -inf where the likelihood is zero, NaN where a + w > T - and ln ||W_c||^2."""
    model, keep = model_to_abi(W, phi, "f64", label_site)
    N, T, Cn = int(model.N), int(model.T), int(model.C)
    mw = int(max_width)
    dp = C.POINTER(C.c_double)
    lp, lnorm, sec = np.zeros((N, T, max(mw, 0), Cn)), np.zeros(Cn), C.c_double()
    eng._chk(eng.lib.mpst_segment_marginals(eng.ctx, C.byref(model), mw, lp.ctypes.data_as(dp), lnorm.ctypes.data_as(dp), C.byref(sec)))
    del keep
    return lp, lnorm, sec.value


# ---- NumPy on an lp array -----------------------------------------------------------------------------------------------------------
def _checked(lp):
    lp = np.asarray(lp, dtype=np.float64)
    if lp.ndim != 4 or lp.shape[2] < 1 or lp.shape[2] > max(lp.shape[1], 1):
        raise ValueError(f"lp must be (N, T, max_width, C) with 1 <= max_width <= T, got {lp.shape}")
    return lp


def valid_triangle(T, max_width):
    """(T, max_width) bool: the segment of width w = column + 1 from the start a = row lies inside the series, a + w <= T"""
    return np.arange(T)[:, None] + np.arange(1, max_width + 1)[None, :] <= T


def class_index_from(lp, label_index=None):
    """(N,) class indices: ``label_index`` checked against ``lp`` (N, T, max_width, C), or - None - the arg-max class (the lowest index
    on a tie) of the widest segment from the first site, ``lp[:, 0, max_width - 1]``: with ``max_width = T`` the prediction from the
    complete series."""
    lp = _checked(lp)
    if label_index is None:
        at = lp[:, 0, lp.shape[2] - 1]
        return np.argmax(np.where(np.isnan(at), -np.inf, at), axis=1).astype(np.int64) if lp.shape[0] else np.zeros(0, dtype=np.int64)
    idx = np.asarray(label_index, dtype=np.int64)
    if idx.shape != lp.shape[:1] or (idx.size and (idx.min() < 0 or idx.max() >= lp.shape[3])):
        raise ValueError("label_index must be (N,) class indices in 0 .. C - 1")
    return idx


def evidence_from(lp, label_index=None, width=1):
    """(N, T): the log odds of each series' class c = ``label_index[i]`` (None: ``class_index_from``) against all the others from the
    segment of ``width`` sites at every start, ``lp[i, a, width - 1, c] - logsumexp_{c' != c} lp[i, a, width - 1, c']``.  NaN where
    a + width > T and where both terms are -inf; +inf where only the others are (always, with one class)."""
    lp = _checked(lp)
    w = int(width)
    if not 1 <= w <= lp.shape[2]:
        raise ValueError(f"width must lie in 1 .. max_width = {lp.shape[2]} (got {width})")
    idx = class_index_from(lp, label_index)
    N, T, _, Cn = lp.shape
    at = lp[:, :, w - 1]                                            # (N, T, C)
    own = np.take_along_axis(at, idx[:, None, None], axis=2)[..., 0]
    rest = np.where(np.arange(Cn)[None, None, :] == idx[:, None, None], -np.inf, at)
    m = np.max(rest, axis=2, keepdims=True) if Cn else np.full((N, T, 1), -np.inf)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        other = np.log(np.sum(np.exp(rest - m0), axis=2)) + m0[..., 0]
        return own - other


def best_segment_from(lp, label_index=None):
    """``BestSegment(start, width, posterior)``: per series the segment inside the triangle whose posterior of the series' class
    (``label_index[i]``; None: ``class_index_from``), the softmax of ``lp`` over the classes, is largest; on a tie the shortest, then
    the earliest.  A segment whose row is -inf in every class has no posterior and is never chosen; a series without any gives
    (0, 1, NaN)."""
    lp = _checked(lp)
    idx = class_index_from(lp, label_index)
    N, T, mw, _ = lp.shape
    post = np.take_along_axis(posteriors_from(lp), idx[:, None, None, None], axis=3)[..., 0]       # (N, T, mw)
    post = np.where(valid_triangle(T, mw)[None], post, np.nan)
    flat = np.transpose(post, (0, 2, 1)).reshape(N, mw * T)         # width-major: the first arg-max is the shortest, then the earliest
    k = np.argmax(np.where(np.isnan(flat), -np.inf, flat), axis=1) if N else np.zeros(0, dtype=np.int64)
    return BestSegment((k % T).astype(np.int64), (k // T + 1).astype(np.int64), flat[np.arange(N), k])


def accuracy_map_from(lp, y_index):
    """(T, max_width): the share of series whose arg-max class of ``lp[:, a, w - 1]`` (the lowest index on a tie; class 0 for a row
    that is -inf everywhere) equals ``y_index`` (N,); NaN where a + w > T, and everywhere for an empty set."""
    lp = _checked(lp)
    y = np.asarray(y_index)
    if y.shape != lp.shape[:1]:
        raise ValueError(f"y_index must be (N,) = ({lp.shape[0]},), got {y.shape}")
    T, mw = lp.shape[1:3]
    if lp.shape[0] == 0:
        return np.full((T, mw), np.nan)
    pred = np.argmax(np.where(np.isnan(lp), -np.inf, lp), axis=3)
    return np.where(valid_triangle(T, mw), np.mean(pred == y[:, None, None], axis=0), np.nan)


# ---- the public calls -----------------------------------------------------------------------------------------------------------------
def _label_index(mps, y, strict):
    """class indices of the label values ``y``; an unknown label is an error (strict) or -1, which matches no class"""
    known = np.unique(mps.train_data.labels)
    y = np.asarray(y)
    idx = np.searchsorted(known, y)
    ok = (idx < len(known)) & (known[np.minimum(idx, len(known) - 1)] == y)
    if strict and not np.all(ok):
        raise ValueError("y holds a value that is not a class of the model")
    return np.where(ok, idx, -1).astype(np.int64)


def segment_log_marginals(mps, X, max_width, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0,
                          return_seconds: bool = False):
    """ln l_c(i; a, w) of the values of the sites a .. a+w-1 of every series alone under every class, every other site marginalised:
    (N, T, max_width, C), columns in the order of ``np.unique(train labels)``, -inf where the likelihood is zero, NaN where
    a + w > T.  ``X``: raw series (N, T) or an EncodedTimeSeriesSet, as in ``log_marginals`` with nothing masked.
    ``normalise_classes=True`` subtracts ln ||W_c||^2, obtained in the same call, which gives the likelihood under the normalised class
    MPS - the meaning it has in ``log_marginals``."""
    shape = np.asarray(X.phi).shape[:2] if isinstance(X, EncodedTimeSeriesSet) else np.shape(X)
    phi, _ = marginal_states(mps, X, np.zeros(shape, dtype=bool))
    N, T = phi.shape[:2]
    mw = int(max_width)
    if not 1 <= mw <= T:
        raise ValueError(f"max_width must lie in 1 .. T = {T} (got {max_width})")
    Cn = int(mps.mps[-1].shape[3])
    if N == 0:
        out = np.zeros((0, T, mw, Cn))
        return (out, 0.0) if return_seconds else out
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        lp, lnorm, secs = segment_model(eng, mps.mps, phi, mw)
    finally:
        if own:
            eng.close()
    if normalise_classes:
        lp = lp - lnorm
    return (lp, secs) if return_seconds else lp


def segment_posteriors(mps, X, max_width, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0,
                       return_seconds: bool = False):
    """p(c | the values of the sites a .. a+w-1) under a uniform prior over classes: (N, T, max_width, C), the softmax of
    ``segment_log_marginals`` over the classes.  A row that is -inf in every class is a NaN row, and so is one with a + w > T."""
    lp, secs = segment_log_marginals(mps, X, max_width, normalise_classes, engine=engine, device=device, return_seconds=True)
    post = posteriors_from(lp)
    return (post, secs) if return_seconds else post


def classify_segment(mps, X, start, width, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0):
    """Classify every series from the ``width`` values that begin at site ``start`` alone - a recording that starts late and stops
    early: the label (original label values) of the largest segment likelihood, the lowest class on a tie."""
    labels = np.unique(mps.train_data.labels)
    a, w = int(start), int(width)
    lp = segment_log_marginals(mps, X, max(w, 1), normalise_classes, engine=engine, device=device)
    if w < 1 or a < 0 or a + w > lp.shape[1]:
        raise ValueError(f"the segment must lie inside the series: 0 <= start, 1 <= width, start + width <= T = {lp.shape[1]}")
    if lp.shape[0] == 0:
        return np.zeros(0, dtype=labels.dtype)
    return labels[np.argmax(lp[:, a, w - 1], axis=1)]


def _class_index(mps, X, y, engine, device):
    """the class indices of ``y``, or - None - of the prediction from the complete series"""
    if y is not None:
        return _label_index(mps, y, strict=True)
    from .marginal import log_marginals
    shape = np.asarray(X.phi).shape[:2] if isinstance(X, EncodedTimeSeriesSet) else np.shape(X)
    full = log_marginals(mps, X, np.zeros(shape, dtype=bool), engine=engine, device=device)
    return np.argmax(full, axis=1).astype(np.int64) if full.shape[0] else np.zeros(0, dtype=np.int64)


def segment_evidence(mps, X, y=None, width: int = 1, engine: Optional[SweepEngine] = None, device: int = 0):
    """(N, T): the class-evidence map at the scale ``width``: per (series, start) the log odds of the class ``y[i]`` (original label
    values; None: the prediction from the complete series) against all the others from that segment alone, under the normalised class
    states: ``ln l_c - logsumexp_{c' != c} ln l_{c'}``.  NaN where start + width > T."""
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        idx = _class_index(mps, X, y, eng, device)
        lp = segment_log_marginals(mps, X, width, normalise_classes=True, engine=eng)
    finally:
        if own:
            eng.close()
    return evidence_from(lp, idx, width)


def most_discriminative_segment(mps, X, y=None, max_width: int = 1, normalise_classes: bool = False,
                                engine: Optional[SweepEngine] = None, device: int = 0):
    """``BestSegment(start, width, posterior)`` per series: the segment of at most ``max_width`` sites from which the posterior of
    the class ``y[i]`` (original label values; None: the prediction from the complete series) is largest; ties go to the shortest
    segment, then to the earliest."""
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        idx = _class_index(mps, X, y, eng, device)
        lp = segment_log_marginals(mps, X, max_width, normalise_classes, engine=eng)
    finally:
        if own:
            eng.close()
    return best_segment_from(lp, idx)


def segment_accuracy_map(mps, X, y, max_width, normalise_classes: bool = False, engine: Optional[SweepEngine] = None, device: int = 0):
    """(T, max_width): the accuracy of ``classify_segment(mps, X, a, w)`` over the data set against the labels ``y`` (original label
    values; an unknown label matches no class) for every start a and width w: which windows suffice to classify.  NaN where
    a + w > T."""
    lp = segment_log_marginals(mps, X, max_width, normalise_classes, engine=engine, device=device)
    return accuracy_map_from(lp, _label_index(mps, y, strict=False))
