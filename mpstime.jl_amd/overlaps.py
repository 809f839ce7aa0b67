"""Overlaps of trained models on the device (``mpst_model_overlaps``, csrc/mpst_overlap.hip).

``model_overlaps`` takes K models of one shape - the folds of a cross-validation, the seeds of ``fit_batch``, the candidates of
``tune`` - and returns the inner products of all their class states, normalised: for the L2-orthonormal bases (Legendre, Fourier) that
is the function-space overlap of the models, the measure of fold stability and ensemble diversity.  ``class_overlaps`` is the
reference's ``overlapmat`` (src/summary.jl:247-251): the fidelity of one model's class states with each other.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib as L
from .engine import SweepEngine, label_site_of, model_to_abi


@dataclass
class ModelOverlaps:
    """Result of ``model_overlaps``.  ``log_norm``: K arrays, ln ||psi_{k,c}|| (-inf for a zero state).  ``offsets`` (K + 1,): the classes
    of model k are rows ``offsets[k]:offsets[k + 1]`` of the block matrices.  ``overlap`` (sum C, sum C), real or complex:
    <psi_{a,c}|psi_{b,c'}> / (||psi_{a,c}|| ||psi_{b,c'}||), formed in the log domain, Hermitian; NaN in blocks that were not requested
    and in the rows and columns of a zero state.  ``fidelity`` = |overlap|.  ``pairs`` (P, 2), ``g`` (P, Cmax, Cmax), ``lg`` (P,): what
    the device returned, the K self pairs first - entry [c, c'] of pair (a, b) is g exp(lg), conjugate on a."""
    log_norm: List[np.ndarray]
    offsets: np.ndarray
    overlap: np.ndarray
    fidelity: np.ndarray
    pairs: np.ndarray
    g: np.ndarray
    lg: np.ndarray
    seconds: float = 0.0


def _sites(W):
    mps = W.mps if hasattr(W, "mps") else W
    mps = [np.asarray(t) for t in mps]
    cx = any(np.iscomplexobj(t) for t in mps)
    return [t.astype(np.complex128 if cx else np.float64, copy=False) for t in mps], cx       # fp32 / c32 models are upcast


def _checked_models(models):
    mods = [_sites(W) for W in models]
    if not mods:
        raise ValueError("model_overlaps needs at least one model")
    shape = None
    for k, (mps, cx) in enumerate(mods):
        if any(t.ndim not in (3, 4) for t in mps):
            raise ValueError(f"model {k}: site tensors are (Dl, d, Dr) or (Dl, d, Dr, C)")
        s = (len(mps), int(mps[0].shape[1]), label_site_of(mps, ValueError), cx)
        if shape is None:
            shape = s
        elif s != shape:
            raise ValueError(f"model {k} disagrees with model 0 in (T, d, label site, complex): {s} against {shape}")
    return [m for m, _ in mods], shape


def _checked_pairs(pairs, K):
    self_pairs = [(k, k) for k in range(K)]
    if pairs is None:
        asked = [(a, b) for a in range(K) for b in range(a, K)]
    else:
        asked = [(int(a), int(b)) for a, b in pairs]
        for a, b in asked:
            if not (0 <= a < K and 0 <= b < K):
                raise ValueError(f"pair ({a}, {b}) names a model outside 0..{K - 1}")
    return np.array(self_pairs + [q for q in asked if q[0] != q[1]], dtype=np.int32).reshape(-1, 2)


def overlaps_raw(eng: SweepEngine, models, pairs, cx: bool):
    """``mpst_model_overlaps`` on checked models (lists of float64 / complex128 site tensors) and an int32 (P, 2) pair table, or None
    for every a <= b: (g (P, Cmax, Cmax), lg (P,), device seconds)."""
    K = len(models)
    abi = [model_to_abi(m, None) for m in models]
    arr = (L.ImputeModel * K)(*[a[0] for a in abi])
    cmax = max(int(a[0].C) for a in abi)
    P = K * (K + 1) // 2 if pairs is None else len(pairs)
    g = np.zeros((P, cmax, cmax), dtype=np.complex128 if cx else np.float64)
    lg = np.zeros(P)
    sec = C.c_double()
    dp = C.POINTER(C.c_double)
    pp = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    rc = eng.lib.mpst_model_overlaps(eng.ctx, arr, K, None if pp is None else pp.ctypes.data_as(C.POINTER(C.c_int32)), P,
                                     g.ctypes.data_as(dp), lg.ctypes.data_as(dp), C.byref(sec))
    if rc:
        raise L.MPSTError(rc, (eng.lib.mpst_last_error(eng.ctx) or b"").decode())
    return g, lg, sec.value


def model_overlaps(models, pairs=None, engine: Optional[SweepEngine] = None, device: int = 0) -> ModelOverlaps:
    """Normalised overlaps of the class states of ``models``: TrainedMPS objects or lists of site tensors (Dl, d, Dr[, C]) that agree in
    T, d, label site and element type (real / complex; ValueError otherwise, before any device work); bond dimensions and class counts
    may differ.  ``pairs``: (a, b) model indices, or None for all of them; the self pairs are always computed, because they give the
    norms.  The class states are the label slices as stored, so ``log_norm`` is what ``classify`` leaves unnormalised."""
    mods, (T, d, p, cx) = _checked_models(models)
    K = len(mods)
    table = _checked_pairs(pairs, K)
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        g, lg, sec = overlaps_raw(eng, mods, table, cx)
    finally:
        if own:
            eng.close()
    ncls = [int(m[p].shape[3]) for m in mods]
    offsets = np.concatenate([[0], np.cumsum(ncls)]).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_norm = [0.5 * (np.log(np.abs(np.diagonal(g[k])[:ncls[k]].real)) + lg[k]) for k in range(K)]
        overlap = np.full((offsets[-1], offsets[-1]), np.nan, dtype=g.dtype)
        for q, (a, b) in enumerate(table):
            blk = g[q, :ncls[a], :ncls[b]]
            mag = np.abs(blk)
            phase = np.where(mag > 0, blk / np.where(mag > 0, mag, 1.0), 0.0)
            val = phase * np.exp(np.log(mag) + lg[q] - log_norm[a][:, None] - log_norm[b][None, :])
            val = np.where(np.isneginf(log_norm[a])[:, None] | np.isneginf(log_norm[b])[None, :], np.nan, np.where(mag > 0, val, 0.0))
            if a == b:
                val = 0.5 * (val + val.conj().T)
            overlap[offsets[a]:offsets[a + 1], offsets[b]:offsets[b + 1]] = val
            overlap[offsets[b]:offsets[b + 1], offsets[a]:offsets[a + 1]] = val.conj().T
    return ModelOverlaps(log_norm, offsets, overlap, np.abs(overlap), table, g, lg, sec)


def class_overlaps(W, engine: Optional[SweepEngine] = None, device: int = 0):
    """(C, C): |<psi_c|psi_c'>| of the normalised class states of one model - the reference's ``overlapmat`` (summary.jl:247-251)."""
    return model_overlaps([W], engine=engine, device=device).fidelity
