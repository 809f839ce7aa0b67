"""Imputation API of the reference (src/Imputation/imputation.jl) on top of the device-side engine ``mpst_impute``.

``init_imputation_problem`` / ``MPS_impute`` keep the reference's names and argument meaning (one instance at a time, as
the reference's callers use them); ``impute_dataset`` is the batched entry the engine is built for: every test instance
with its own set of missing sites in one call.  Values cross the C ABI in the encoding's domain; the pre-processing
of ``get_predictions`` (imputation.jl:264-410: mask with the training mean, transform with the train-fitted
normalisations, invert them on the way out) stays on the host.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .encodings import fit_encoding_from_training_data, opts_encoding, transform_test_data, transform_train_data
from .engine import SweepEngine, check_levels
from .options import MPSOptions, engine_options, safe_options

METHODS = {"median": 0, "mode": 1, "ITS": 2, "mean": 3}
ORDERS = {"forwards": 0, "backwards": 1}


def invert_test_transform(X_scaled, oob_rescales, norms, opts: MPSOptions, enc_range):
    """utils.jl:299-334 (rows are series here)."""
    X = np.array(X_scaled, dtype=np.float64, copy=True)
    one = X.ndim == 1
    X = np.atleast_2d(X)
    a, b = enc_range
    X = (X - a) / (b - a)
    for i, lb_shift, ub_scale in oob_rescales:
        X[int(i)] = X[int(i)] * ub_scale + lb_shift
    if opts.minmax:
        lb, ub = opts.data_bounds
        X = (X - lb) / (ub - lb)
    if norms.minmax is not None:                    # denormalize!, in reverse order of application
        lo, hi = norms.minmax
        X = X * (hi - lo) + lo
    if norms.sigmoid is not None:
        med, iqr = norms.sigmoid
        with np.errstate(divide="ignore", invalid="ignore"):
            X = med - (iqr / 1.35) * np.log(1.0 / X - 1.0)
    return X[0] if one else X


def mar(X, fraction_missing=0.5, rng=None):
    """mar(X, fraction, BlockMissingMAR()) (src/Simulation/missing_data_mechanisms.jl:114-152): a block of consecutive
    missing values whose start is uniform over the valid positions.  Returns (X_corrupted, missing_idxs) (0-based)."""
    if not 0.0 <= fraction_missing <= 1.0:
        raise ValueError("fraction_missing must be between 0 and 1")
    rng = rng or np.random.default_rng()
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    npts = int(round(n * fraction_missing))
    start = int(rng.integers(0, n - npts + 1))
    idx = np.arange(start, start + npts)
    Xc = X.copy()
    Xc[idx] = np.nan
    return Xc, idx


@dataclass
class EncodedDataRange:                 # imputation.jl:2-8
    dx: float
    guess_range: tuple
    xvals: np.ndarray
    xvals_enc: np.ndarray               # (ngrid, d): time-independent encodings share one table (:100-106); (T, ngrid, d): one per site (:92-99)


@dataclass
class ImputationProblem:                # imputation.jl:10-20
    mps: list                           # the trained MPS with its label index (the engine slices classes itself)
    X_train: np.ndarray
    y_train: np.ndarray
    X_test: np.ndarray
    y_test: np.ndarray
    opts: MPSOptions
    x_guess_range: EncodedDataRange
    class_map: dict
    encoder: object = None              # FittedEncoder: the reference's enc_args (:88), bound
    custom_encoding: object = None      # the Encoding behind opts.encoding == "Custom" (TrainedMPS.custom_encoding)


def init_imputation_problem(W, X_test, y_test=None, dx: float = 1e-4, guess_range=None, verbosity: int = 1):
    """init_imputation_problem(W::TrainedMPS, X_test, y_test; dx, guess_range) (imputation.jl:143-190): the candidate
    values ``range(guess_range...; step=dx)`` and their encoded states are tabulated once."""
    opts = safe_options(W.opts)
    td = W.train_data
    custom = getattr(W, "custom_encoding", None)
    enc, _, encoder = fit_encoding_from_training_data(opts, td.original_data, td.labels, custom)  # :88
    if guess_range is None:
        guess_range = tuple(enc.range)
    X_test = np.asarray(X_test, dtype=np.float64)
    y_test = np.zeros(X_test.shape[0], dtype=np.int64) if y_test is None else np.asarray(y_test)
    n = int(np.floor((guess_range[1] - guess_range[0]) / dx + 1e-9)) + 1
    xvals = guess_range[0] + dx * np.arange(n)
    classes = np.unique(td.labels)
    # a time-dependent encoding is tabulated per site (:92-99), here on the host: the grid hits bin edges exactly, where one
    # tabulation must decide for every consumer
    states = encoder.table(xvals, X_test.shape[1])
    rng = EncodedDataRange(dx, guess_range, xvals, np.ascontiguousarray(states, dtype=np.complex128 if np.iscomplexobj(states) else np.float64))
    if verbosity > 0:
        print(f" - Dataset has {td.original_data.shape[0]} training samples and {X_test.shape[0]} testing samples.")
        print(f" - {len(classes)} class(es) were detected.")
    return ImputationProblem(W.mps, td.original_data, np.asarray(td.labels), X_test, y_test, opts, rng,
                             {c: i for i, c in enumerate(classes.tolist())}, encoder, custom)


def _scaled_instances(imp: ImputationProblem, rows, masks, fill=None):
    """get_predictions' pre-processing (imputation.jl:283-297) for several instances at once: the missing region is
    overwritten with ``fill`` (default: the training mean) BEFORE the test transform (its per-series out-of-bounds rescale sees
    the masked series), the full series is transformed separately as the target in the encoding's domain."""
    enc = opts_encoding(imp.opts, imp.custom_encoding)
    if imp.encoder is None:
        imp.encoder = fit_encoding_from_training_data(imp.opts, imp.X_train, imp.y_train, imp.custom_encoding)[2]
    _, norms = transform_train_data(imp.X_train, imp.opts, enc.range)
    raw = imp.X_test[rows]
    full, _ = transform_test_data(raw, norms, imp.opts, enc.range)
    masked = raw.copy()
    masked[masks] = np.mean(imp.X_train) if fill is None else fill
    scaled, oob = transform_test_data(masked, norms, imp.opts, enc.range)
    return enc, norms, raw, full, scaled, oob


def _check_trajectories(method, num_trajectories):
    """num_trajectories of impute_ITS (MPS_methods.jl:304-347): None (one series per instance, today's shapes) or K >= 1 chains
    per instance, which only the sampling method draws."""
    if num_trajectories is None:
        return None
    K = int(num_trajectories)
    if K < 1:
        raise ValueError("num_trajectories must be at least 1")
    if method != "ITS":
        raise ValueError(f"num_trajectories needs method 'ITS': {method!r} gives one series per instance")
    return K


def _draw_uniforms(rng, N, T, trials, K=None):
    """The host-drawn uniform numbers of the sampling method: (N, T, trials), or (N, K, T, trials) for K trajectories - chain
    (i, k) reads u[i, k] exactly as a single-trajectory call reads u[i]."""
    shape = (N, T, trials) if K is None else (N, K, T, trials)
    return np.ascontiguousarray((rng or np.random.default_rng()).uniform(0.0, 1.0, shape))


def _run_engine(imp: ImputationProblem, data, kw, *, engine, device, compute):
    """The engine on ``data`` = (phi, class indices, mask): a real fp64 model through a context and its data set, everything else
    (complex states, fp32 compute) in one call that hands the model over.  ``kw``: the arguments of ``SweepEngine.impute``
    behind the grid; returns what that returns."""
    phi, lab, m8 = data
    xr = imp.x_guess_range
    cx = np.iscomplexobj(phi) or np.iscomplexobj(xr.xvals_enc) or any(np.iscomplexobj(t) for t in imp.mps)
    phi = np.ascontiguousarray(phi, dtype=np.complex128 if cx else np.float64)
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        if cx or compute != "f64":
            return eng.impute_model(imp.mps, phi, lab, m8, xr.xvals, xr.xvals_enc, compute=compute, **kw)
        eng.set_options(**engine_options(imp.opts))
        eng.set_dataset(1, phi, lab, int(imp.mps[-1].shape[3]))
        eng.set_mps(imp.mps)
        return eng.impute(1, m8, xr.xvals, xr.xvals_enc, **kw)
    finally:
        if own:
            eng.close()


def impute_dataset(imp: ImputationProblem, missing_mask, method: str = "median", rows=None, invert_transform: bool = True,
                   get_wmad: bool = True, rng=None, engine: Optional[SweepEngine] = None, device: int = 0, return_seconds=False,
                   impute_order: str = "forwards", rejection_threshold=None, max_trials: int = 10, compute: str = "f64", shard=None,
                   num_trajectories=None, rseed=None, quantiles=None):
    """Impute every instance of ``imp.X_test[rows]`` (default: all) at the sites where ``missing_mask`` is True, each
    with the MPS of its class.  Returns (X_imputed, pred_err) in the original units (``invert_transform``) or in the
    encoding's domain; pred_err is the weighted median absolute deviation for ``method="median"``, the standard
    deviation for ``"mean"`` and None otherwise.  ``"ITS"`` draws one trajectory per instance from ``rng``
    (``rejection_threshold`` None is the reference's ``:none``).  Complex encodings (Fourier, Sahand) and
    ``compute="f32"`` (fp32 chain contractions, fp64 densities) go through ``mpst_impute_model_run``.  With a ``shard``
    (distributed.Shard) every rank imputes its slice of the rows - instances are independent, there is no collective on
    the data path - and the results are gathered on every rank.

    ``num_trajectories`` = K (``method="ITS"`` only; impute_ITS's keyword): every instance is conditioned once and K chains
    are sampled from it.  X_imputed is then (N, K, T) - known sites from the scaled series, ``invert_transform`` applied
    to every trajectory with its instance's own out-of-bounds rescale - and, with a ``rejection_threshold``, pred_err holds the
    chains' weighted median absolute deviations in the same shape (None without).  ``rseed`` given: the uniform numbers come
    from the device generator keyed by (rseed; row, trajectory, site, trial) with ``rows`` as the row ids, so a chain does not
    depend on which other rows are imputed with it or on how they are dealt over ranks; ``rseed`` None: they are drawn from
    ``rng`` on the host.

    ``quantiles`` = (q1, ...) (``method="median"`` only, up to 16 levels inside (0, 1)): the return value is (X_imputed, pred_err,
    bands) with bands (N, T, nq) the grid value at every level of every missing site's conditional distribution - the distribution
    the median was read from, conditioned on the known values and the medians chosen before it; the pass that imputes builds them.
    Known sites carry the known value in every level; ``invert_transform`` maps every level like X_imputed, with the instance's own
    out-of-bounds rescale (the transform is monotone: levels stay ordered)."""
    levels = check_levels(quantiles)
    if levels is not None and method != "median":
        raise ValueError(f"quantiles are read off the median imputer's distribution: method must be 'median', not {method!r}")
    if levels is not None and num_trajectories is not None:
        raise ValueError("quantiles cannot be combined with num_trajectories")
    K = _check_trajectories(method, num_trajectories)
    if rseed is not None and K is None:
        raise ValueError("rseed seeds the device generator of a call with num_trajectories")
    if method not in METHODS:
        raise ValueError("Invalid method. Choose :mean, :mode, :median, :kNearestNeighbour, :flatBaseline or :ITS"
                         if method not in ("kNearestNeighbour", "flatBaseline") else
                         f"method {method!r} is evaluated on the host in the reference and is not part of the device engine")
    if impute_order not in ORDERS:
        raise ValueError('impute_order must be either ":forwards" or ":backwards"')
    rows = np.arange(imp.X_test.shape[0]) if rows is None else np.asarray(rows)
    mask = np.asarray(missing_mask, dtype=bool)
    assert mask.shape == (len(rows), imp.X_test.shape[1])
    if shard is not None and shard.world > 1:
        return _impute_sharded(imp, mask, method, rows, shard, invert_transform=invert_transform, get_wmad=get_wmad, rng=rng,
                               engine=engine, device=device, return_seconds=return_seconds, impute_order=impute_order,
                               rejection_threshold=rejection_threshold, max_trials=max_trials, compute=compute,
                               num_trajectories=num_trajectories, rseed=rseed, quantiles=quantiles)
    enc, norms, raw, full, scaled, oob = _scaled_instances(imp, rows, mask)
    lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test)[rows].tolist()], dtype=np.int32)
    order = np.argsort(lab, kind="stable")                      # the engine wants class-sorted data sets
    phi = imp.encoder(scaled[order])
    m8 = np.ascontiguousarray(mask[order], dtype=np.uint8)
    N, T = m8.shape
    u = None
    code, trials, thr, basis = METHODS[method], 1, 0.0, 1
    if method == "ITS":
        if rejection_threshold is not None:
            code, trials, thr = 4, int(max_trials), float(rejection_threshold)
        if rseed is None:
            u = _draw_uniforms(rng, N, T, trials, K)
    if method == "mean":
        codes = {"Legendre_Norm": 0, "Legendre_No_Norm": 1, "Fourier": 2, "Stoudenmire": 3, "Sahand": 4, "Uniform": 5}    # MPST_BASIS_*
        if enc.name not in codes:                   # (split and time-dependent encodings included)
            raise NotImplementedError("method 'mean' re-encodes the expectation value on the device: closed-form bases only "
                                      f"({', '.join(codes)}), not {enc.name}")
        basis = codes[enc.name]
    kw = dict(method=code, get_wmad=get_wmad, u=u, order=ORDERS[impute_order], max_trials=trials, rejection_threshold=thr, mean_basis=basis,
              levels=levels)
    if K is not None:
        kw.update(num_trajectories=K, seed=rseed, row_id=np.asarray(rows, dtype=np.int64)[order])
    out = _run_engine(imp, (phi, lab[order], m8), kw, engine=engine, device=device, compute=compute)
    x, err, secs = out[:3]
    qv = out[3] if levels is not None else None
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    x, err = x[inv], err[inv]
    if K is not None:
        ts = np.where(mask[:, None, :], x, scaled[:, None, :])
        pred = err if rejection_threshold is not None else None
        if invert_transform:
            inv_k = lambda a: np.stack([invert_test_transform(a[:, k], oob, norms, imp.opts, enc.range) for k in range(K)], axis=1)
            hi = inv_k(ts + pred) if pred is not None else None
            ts = inv_k(ts)
            if pred is not None:
                pred = hi - ts
        out = (ts, pred)
        return out + (secs,) if return_seconds else out
    ts = np.where(mask, x, scaled)                               # x_samps: known values as given, imputed ones filled in
    pred = err if (method in ("median", "mean") and get_wmad) else None
    if invert_transform:
        hi = None
        if pred is not None:
            hi = invert_test_transform(ts + pred, oob, norms, imp.opts, enc.range)     # :339-341: add, invert, subtract
        ts = invert_test_transform(ts, oob, norms, imp.opts, enc.range)
        if pred is not None:
            pred = hi - ts
    out = (ts, pred)
    if levels is not None:
        bands = np.where(mask[:, :, None], qv[inv], scaled[:, :, None])
        if invert_transform:
            bands = np.stack([invert_test_transform(bands[:, :, l], oob, norms, imp.opts, enc.range) for l in range(bands.shape[2])], axis=2)
        out = out + (bands,)
    return out + (secs,) if return_seconds else out


def _impute_sharded(imp, mask, method, rows, shard, return_seconds=False, rng=None, **kw):
    """Rows i with i % world == rank on every rank (the classes stay balanced), results gathered with the host-side
    process group.  The uniform numbers of the sampling method (ITS) come from one seed shared by all ranks (rank 0's draw
    from `rng`, broadcast) and one stream per rank derived from it - reproducible for a given `rng` state and world size, not
    the single-process stream.  With `rseed` (a call with `num_trajectories`) the numbers come from the device generator keyed
    by the caller's row ids instead: the gathered result IS the single-process result."""
    import torch.distributed as dist
    mine = np.arange(shard.rank, len(rows), shard.world)
    shard_rng = None
    if method == "ITS" and kw.get("rseed") is None:
        # one seed for the whole call - rank 0's draw (from `rng` if given), broadcast over the host-side group - and one
        # stream per rank derived from it: a sharded run with the same `rng` state and world size repeats itself
        seed = [int((rng or np.random.default_rng()).integers(0, 2 ** 62))]
        dist.broadcast_object_list(seed, src=0, group=shard.group)
        shard_rng = np.random.default_rng([seed[0], shard.rank])
    ts = pred = bands = None
    secs = 0.0
    nq = None if kw.get("quantiles") is None else len(np.atleast_1d(kw["quantiles"]))
    if len(mine):
        out = impute_dataset(imp, mask[mine], method, rows=np.asarray(rows)[mine], return_seconds=True, rng=shard_rng, **kw)
        ts, pred, secs = out[0], out[1], out[-1]
        if nq is not None:
            bands = out[2]
    parts = [None] * shard.world
    dist.all_gather_object(parts, (mine, ts, pred, secs, bands), group=shard.group)
    T = mask.shape[1]
    K = kw.get("num_trajectories")
    shape = (len(rows), T) if K is None else (len(rows), int(K), T)
    full = np.zeros(shape)
    perr = np.zeros(shape)
    have_err = False
    fullb = np.zeros((len(rows), T, nq)) if nq is not None else None
    for idx, t, e, _, bd in parts:
        if t is None:
            continue
        full[idx] = t
        if e is not None:
            perr[idx] = e
            have_err = True
        if fullb is not None:
            fullb[idx] = bd
    out = (full, perr if have_err else None)
    if fullb is not None:
        out = out + (fullb,)
    return out + (max(p[3] for p in parts),) if return_seconds else out


def get_cdfs(imp: ImputationProblem, class_, instance: int, missing_sites, method: str = "median", impute_order: str = "forwards",
             get_wmad: bool = True, stride: int = 1, engine: Optional[SweepEngine] = None, device: int = 0):
    """get_cdfs(imp, class, instance, missing_sites, method) (imputation.jl:581-622): the median imputer on one instance and, for
    every missing site, the cumulative distribution its median was read from.  Returns (cdfs, ts, pred_err,
    target_timeseries_full): ``cdfs`` a list with one array per missing site in ascending site order - the normalised cdf on the
    grid ``imp.x_guess_range.xvals`` (``stride`` s > 1: at the grid indices 0, s, 2s, ... and the last one) -, ``ts = [x_samps]`` and
    ``pred_err = [wmads]`` in the ENCODING's domain (the reference's get_cdfs does not invert the transform), and the fully
    transformed target series.  As in the reference the masked region is overwritten with ``mean(X_test)`` before the test
    transform (:609; get_predictions / impute_dataset use the training mean there)."""
    if method != "median":
        raise ValueError("get_cdfs only supports method=:median")
    if impute_order not in ORDERS:
        raise ValueError('impute_order must be either ":forwards" or ":backwards"')
    if int(stride) < 1:
        raise ValueError("stride must be at least 1")
    missing_sites = np.asarray(missing_sites, dtype=np.int64)
    cl = np.flatnonzero(np.asarray(imp.y_test) == class_)
    row = int(cl[instance])
    T = imp.X_test.shape[1]
    mask = np.zeros((1, T), dtype=bool)
    mask[0, missing_sites] = True
    enc, _, _, full, scaled, _ = _scaled_instances(imp, [row], mask, fill=np.mean(imp.X_test))
    lab = np.array([imp.class_map[class_]], dtype=np.int32)
    data = (imp.encoder(scaled), lab, np.ascontiguousarray(mask, dtype=np.uint8))
    kw = dict(method=0, get_wmad=get_wmad, order=ORDERS[impute_order], cdf_stride=int(stride))
    x, err, _, _, cdf = _run_engine(imp, data, kw, engine=engine, device=device, compute="f64")
    nmiss = int(mask.sum())
    cdfs = [cdf[0, r].copy() for r in range(nmiss)]
    ts = np.where(mask[0], x[0], scaled[0])
    return cdfs, [ts], [err[0] if get_wmad else None], full[0]


def kNN_impute(imp: ImputationProblem, class_, instance: int, missing_sites, k: int = 1):
    """kNN_impute (imputation.jl:215-254): the k training series of the class closest (MSE over the known sites)."""
    cl = np.flatnonzero(np.asarray(imp.y_test) == class_)
    target = imp.X_test[cl[instance]]
    known = np.setdiff1d(np.arange(imp.X_test.shape[1]), np.asarray(missing_sites))
    c_inds = np.flatnonzero(np.asarray(imp.y_train) == class_)
    mses = np.mean((imp.X_train[c_inds][:, known] - target[known]) ** 2, axis=1)
    return [imp.X_train[c_inds[j]].copy() for j in np.argsort(mses, kind="stable")[:k]]


def mae(forecast, actual):
    return float(np.mean(np.abs(np.asarray(forecast) - np.asarray(actual))))


def mape(forecast, actual):
    return float(np.mean(np.abs(np.asarray(actual) - np.asarray(forecast)) / np.abs(np.asarray(actual))))


def MPS_impute(imp: ImputationProblem, class_, instance: int, missing_sites, method: str = "median", invert_transform: bool = True,
               impute_order: str = "forwards", NN_baseline: bool = True, n_baselines: int = 1, get_metrics: bool = True,
               engine: Optional[SweepEngine] = None, device: int = 0, **kw):
    """MPS_impute(imp, class, instance, missing_sites, method) (imputation.jl:467-550) without the plots:
    returns (ts, pred_err, target, metrics) with ``ts`` / ``pred_err`` lists of series as in the reference.  With
    ``method="ITS", num_trajectories=K, rseed=...`` (and ``rejection_threshold`` / ``max_trials``) the lists and ``metrics`` have K
    entries, one per trajectory (imputation.jl:311-312, 512-522); the nearest-neighbour baseline goes on ``metrics[0]`` only."""
    missing_sites = np.asarray(missing_sites, dtype=np.int64)
    cl = np.flatnonzero(np.asarray(imp.y_test) == class_)
    row = int(cl[instance])
    T = imp.X_test.shape[1]
    mask = np.zeros((1, T), dtype=bool)
    mask[0, missing_sites] = True
    if method == "kNearestNeighbour":
        ts, pred = kNN_impute(imp, class_, instance, missing_sites, k=kw.get("k", 1)), [None]
        target = imp.X_test[row]
    elif method == "flatBaseline":
        t = imp.X_test[row].copy()
        t[missing_sites] = np.mean(imp.X_train)
        ts, pred, target = [t], [None], imp.X_test[row]
    else:
        t, e = impute_dataset(imp, mask, method, rows=[row], invert_transform=invert_transform, engine=engine, device=device,
                              impute_order=impute_order,
                              **{k: v for k, v in kw.items() if k in ("get_wmad", "rng", "rejection_threshold", "max_trials",
                                                                      "num_trajectories") or
                                 (k == "rseed" and kw.get("num_trajectories") is not None)})       # (rseed seeds the trajectories' generator)
        if kw.get("num_trajectories") is not None:          # one series per trajectory (imputation.jl:311-312)
            ts = [t[0, k] for k in range(t.shape[1])]
            pred = [None if e is None else e[0, k] for k in range(t.shape[1])]
        else:
            ts, pred = [t[0]], [None if e is None else e[0]]
        if invert_transform:
            target = imp.X_test[row]
        else:
            target = _scaled_instances(imp, [row], mask)[3][0]
    metrics = []
    if get_metrics:
        for t in ts:
            metrics.append({"MAE": mae(t[missing_sites], target[missing_sites]), "MAPE": mape(t[missing_sites], target[missing_sites])})
    if NN_baseline and method not in ("kNearestNeighbour",):
        nn = kNN_impute(imp, class_, instance, missing_sites, k=n_baselines)
        if get_metrics:
            metrics[0]["NN_MAE"] = mae(nn[0][missing_sites], imp.X_test[row][missing_sites])
            metrics[0]["NN_MAPE"] = mape(nn[0][missing_sites], imp.X_test[row][missing_sites])
    return ts, pred, target, metrics
