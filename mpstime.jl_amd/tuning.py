"""Hyperparameter tuning and k-fold evaluation (src/Training/hyperparameters/: tuning.jl, evaluate.jl, random_search.jl,
hyperopt_utils.jl) on batched device fits.

The reference farms candidate x fold fits out as ``@distributed`` tasks; here all of them are handed to ``fit_batch`` at once,
which advances fits of one shape together with ``sweep_batch`` (one launch chain for up to 64 fits), and the trained models are
scored together with ``classify_batch`` (two launches for a whole batch).  There is no sequential mode: the yardstick is a plain
loop over the public ``fitMPS`` and ``eval_loss``.

Not reproduced: the Optimization.jl solvers (a non-``MPSRandomSearch`` optimiser raises NotImplementedError), the ``distribute_*``
switches (batching replaces them) and Julia's RNG streams - folds and random grids are deterministic under a NumPy seed but are not
those of a Julia run with the same seed.
"""
from __future__ import annotations

import itertools
import json
import os
import time
from dataclasses import dataclass, fields as dc_fields
from typing import List, Optional

import numpy as np

from . import _lib as L
from .engine import SweepEngine, classify_batch, sweep_batch
from .imputation import impute_dataset, init_imputation_problem, mar
from .options import MPSOptions, engine_options, numpy_dtype, safe_options
from .training import TrainedMPS, _encode_fit, _fit_inputs, classify, classify_states, fitMPS, save_trained_mps

BATCH_HINT = 16          # gradient share count of every batched fit (SweepEngine.set_batch_hint): fixed, so that a fit's bits do not
                         # depend on how many fits happen to share its batch; fitMPS(..., batch_hint=BATCH_HINT) gives the same bits
MAX_BATCH = 64           # mpst_sweep_batch's limit


# ---- losses (hyperopt_utils.jl:1-60, 152-231) -------------------------------------------------------------------------------
class TuningLoss:
    def __repr__(self):
        return type(self).__name__ + "()"


class ClassificationLoss(TuningLoss):
    pass


class MisclassificationRate(ClassificationLoss):
    pass


class BalancedMisclassificationRate(ClassificationLoss):
    pass


class ImputationLoss(TuningLoss):
    pass


def misclassification_rate(y_val, y_pred):
    """[1 - mean(pred == y)] (hyperopt_utils.jl:170-172)"""
    return [1.0 - float(np.mean(np.asarray(y_pred) == np.asarray(y_val)))]


def balanced_misclassification_rate(y_val, y_pred):
    """One minus the mean recall over unique(y_val u y_pred), eps() in the denominator (hyperopt_utils.jl:152-168): a class that
    only appears among the predictions has recall 0 and still counts."""
    y_val, y_pred = np.asarray(y_val), np.asarray(y_pred)
    classes = np.unique(np.concatenate([y_val, y_pred]))
    recall_sum = 0.0
    for cls in classes:
        tp = int(np.sum((y_val == cls) & (y_pred == cls)))
        fn = int(np.sum((y_val == cls) & (y_pred != cls)))
        recall_sum += tp / (tp + fn + np.finfo(np.float64).eps)
    return [1.0 - recall_sum / len(classes)]


def _classification_loss(objective, y_val, y_pred):
    if isinstance(objective, BalancedMisclassificationRate):
        return balanced_misclassification_rate(y_val, y_pred)
    return misclassification_rate(y_val, y_pred)


def make_windows(windows, pms, X, rng=None):
    """make_windows (hyperopt_utils.jl:107-131): the window vectors as given (a dict: its values in key order, concatenated), or
    one block-missing window per percentage in ``pms`` drawn with ``mar``."""
    if windows is not None:
        if pms is not None:
            raise ValueError("Cannot specifiy both windows and pms!")
        if isinstance(windows, dict):
            return [w for key in sorted(windows) for w in windows[key]]
        assert all(np.ndim(w) == 1 for w in windows), "Elements of windows must be window vectors!"
        return list(windows)
    if pms is not None:
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        T = np.asarray(X).shape[1]
        return [mar(np.arange(1.0, T + 1.0), float(pm), rng=rng)[1] for pm in pms]
    raise ValueError("Must specifiy either windows or pms when measuring Imputation Loss!")


def _imputation_loss(mps, X_val, y_val, windows, method="median", engine=None, device=0):
    imp = init_imputation_problem(mps, X_val, y_val, verbosity=-5)
    X_val = np.asarray(X_val, dtype=np.float64)
    n, T = X_val.shape
    out = []
    for w in windows:                       # one device call per window over all instances
        w = np.asarray(w, dtype=np.int64)
        mask = np.zeros((n, T), dtype=bool)
        mask[:, w] = True
        ts, _ = impute_dataset(imp, mask, method, engine=engine, device=device)
        out.append(float(np.mean(np.mean(np.abs(ts[:, w] - X_val[:, w]), axis=1))))
    return out


def eval_loss(objective, mps: TrainedMPS, X_val, y_val, windows=None, method="median", device=0):
    """eval_loss (hyperopt_utils.jl:152-231), always a list.  MisclassificationRate / BalancedMisclassificationRate: from
    ``classify(mps, X_val)``.  ImputationLoss: the MAE per window averaged over the validation instances, one batched
    ``impute_dataset`` call per window (not the reference's instance-by-instance loop).  Every instance is imputed with the MPS of
    its own class; the reference's countmap re-ordering of the instances (its own comment: "This is awful, should fix") is not
    reproduced."""
    if isinstance(objective, ImputationLoss):
        if windows is None:
            raise ValueError("Must specifiy either windows or pms when measuring Imputation Loss!")
        return _imputation_loss(mps, X_val, y_val, windows, method, device=device)
    if not isinstance(objective, ClassificationLoss):
        raise TypeError(f"unknown objective {objective!r}")
    return _classification_loss(objective, y_val, classify(mps, X_val, device=device))


# ---- folds ----------------------------------------------------------------------------------------------------------------
def make_stratified_cvfolds(Xs, ys, nfolds, rng=1, shuffle=True):
    """Stratified k-fold split as (train_inds, val_inds) pairs (0-based, sorted): every class is dealt round-robin over the folds
    after an optional shuffle, so per-class fold sizes differ by at most one.  (The reference uses MLJ.StratifiedCV,
    hyperopt_utils.jl:101-105: the same guarantee, another stream.)"""
    ys = np.asarray(ys)
    n = len(ys)
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    fold_of = np.empty(n, dtype=np.int64)
    nxt = 0                                   # the deal goes on across classes: whole-fold sizes differ by at most one too
    for cls in np.unique(ys):
        idx = np.flatnonzero(ys == cls)
        if shuffle:
            idx = rng.permutation(idx)
        fold_of[idx] = (nxt + np.arange(len(idx))) % nfolds
        nxt = (nxt + len(idx)) % nfolds
    allidx = np.arange(n)
    return [(allidx[fold_of != f], allidx[fold_of == f]) for f in range(nfolds)]


# ---- the random search (random_search.jl) --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class MPSRandomSearch:
    sampling: str = "LatinHypercube"

    def __post_init__(self):
        object.__setattr__(self, "sampling", str(self.sampling).lstrip(":"))
        if self.sampling not in ("LatinHypercube", "UniformRandom", "Exhaustive"):
            raise ValueError("Unknown sampling type, expected :LatinHypercube, :UniformRandom, or :Exhaustive")


def make_grid(rng, grid_type, lb, ub, is_disc, maxiters, maxrerolls=100):
    """make_grid (random_search.jl:1-70): the raw trial vectors (indices into the value list for listed / stepped parameters)."""
    nd = len(lb)
    if grid_type == "UniformRandom":
        samps = []
        for _ in range(maxiters):
            for _roll in range(maxrerolls):
                samp = tuple(int(rng.integers(int(lb[j]), int(ub[j]) + 1)) if is_disc[j] else float((ub[j] - lb[j]) * rng.random() + lb[j])
                             for j in range(nd))
                if samp not in samps:
                    samps.append(samp)
                    break
        return [list(s) for s in samps]
    if grid_type == "LatinHypercube":
        # a random Latin hypercube, scaled like LHS.scaleLHC: continuous dimensions take the maxiters grid lines lb .. ub (one per
        # stratum), categorical ones deal their values evenly
        cols = []
        for j in range(nd):
            perm = rng.permutation(maxiters)
            if is_disc[j]:
                k = int(round(ub[j] - lb[j] + 1))
                cols.append([int(lb[j]) + int(p * k // maxiters) for p in perm])
            else:
                cols.append([float(lb[j] + (ub[j] - lb[j]) * (p / (maxiters - 1) if maxiters > 1 else 0.5)) for p in perm])
        return [[cols[j][i] for j in range(nd)] for i in range(maxiters)]
    if grid_type == "Exhaustive":
        if not all(is_disc):
            raise ValueError("All hyperparameters must be discrete if using the :Exhaustive search method")
        ranges = [range(int(lb[j]), int(ub[j]) + 1) for j in range(nd)]
        # Iterators.product: the FIRST parameter runs fastest
        return [list(reversed(t)) for t in itertools.product(*reversed(ranges))]
    raise ValueError("Unknown sampling type, expected :LatinHypercube, :UniformRandom, or :Exhaustive")


def sort_trials(trials, fields):
    """grid_search's ordering (random_search.jl:72-108): a stable descending sort by the product of the chi_max and d entries, so
    that the slow candidates come first"""
    pos = [i for i, f in enumerate(fields) if f in ("chi_max", "d")]
    if not pos:
        return list(trials)
    return sorted(trials, key=lambda t: -float(np.prod([t[i] for i in pos])))


# ---- parameters (tuning.jl:395-490) ---------------------------------------------------------------------------------------------
@dataclass
class _ParamInfo:
    fields: list
    types: list
    x0: list
    is_disc: list
    lb: list
    ub: list
    value_map: list
    logspace_eta: bool

    def safe_paramlist(self, raw):
        """safe_paramlist (tuning.jl:25-56): raw trial vector -> option values (value list lookup, integer rounding, 10^eta)"""
        out = []
        for i, x in enumerate(raw):
            v = self.value_map[i][int(round(x)) - 1] if len(self.value_map[i]) else x
            if self.types[i] is int:
                out.append(int(round(v)))
            elif self.logspace_eta and self.fields[i] == "eta":
                out.append(float(10.0 ** v))
            else:
                out.append(float(v))
        return tuple(out)


def parse_parameters(parameters, opts0: MPSOptions, logspace_eta=False) -> _ParamInfo:
    """``parameters``: a dict, or a list of (key, value) pairs (where duplicate keys can be told), of ``key=[values]``,
    ``key=(lb, ub)`` or ``key=(lb, step, ub)``."""
    items = list(parameters.items()) if isinstance(parameters, dict) else [tuple(kv) for kv in parameters]
    keys = [k for k, _ in items]
    if len(set(keys)) != len(keys):
        raise ValueError("The 'parameters' argument contains duplicates!")
    names = {f.name for f in dc_fields(MPSOptions)}
    rows = []
    for key, val in items:
        if key not in names:
            raise ValueError(f"'{key}' is not a field of MPSOptions")
        startx = getattr(opts0, key)
        if isinstance(startx, bool) or not isinstance(startx, (int, float)):
            raise ValueError(f"Cannot tune '{key}', only numeric types can be hyperoptimised.")
        ptype = int if isinstance(startx, int) else float
        if logspace_eta and key == "eta":
            if val[0] <= 0:
                raise ValueError("Lower and upper bounds on eta must be positive!")
            if isinstance(val, list) or len(val) == 3:
                raise ValueError("logspace_eta doesn't make sense with this method of specifying eta values")
            val = tuple(float(np.log10(v)) for v in val)
        vmap = []
        if isinstance(val, (list, np.ndarray)):
            vmap = sorted(list(val))
            disc, lo, hi = True, 1, len(vmap)
        elif isinstance(val, tuple) and len(val) == 3:
            nstep = int(np.floor((val[2] - val[0]) / val[1] + 1e-9))
            vmap = [val[0] + i * val[1] for i in range(nstep + 1)]
            disc, lo, hi = True, 1, len(vmap)
        elif isinstance(val, tuple) and len(val) == 2:
            disc, lo, hi = ptype is int, ptype(val[0]), ptype(val[1])
        else:
            raise ValueError("Unknown parameter format. Options are key=[vals], key=(lb,ub), key=(lb,step,ub)")
        if startx < lo or startx > hi:
            startx = lo
        rows.append((key, ptype, startx, disc, lo, hi, vmap))
    rows.sort(key=lambda r: r[0])                  # the result does not depend on the order of the parameters (tuning.jl:481-487)
    cols = list(zip(*rows))
    return _ParamInfo(*[list(c) for c in cols], logspace_eta=bool(logspace_eta))


# ---- batched fits -------------------------------------------------------------------------------------------------------------
@dataclass
class BatchFit:
    """one job of fit_batch: ``mps`` (TrainedMPS) and ``info`` as fitMPS returns them, ``batched`` - it went through the batched
    chain -, ``error`` - the SVDError that stopped it (then ``mps`` is None)"""
    mps: Optional[TrainedMPS] = None
    info: Optional[dict] = None
    test_states: object = None
    batched: bool = False
    error: Optional[Exception] = None


def _batchable(opts: MPSOptions, n_train: int) -> bool:
    """What mpst_sweep_batch takes: the headline chain (Float64, d chi_max <= 128, <= 8192 series, update_iters = 1, no track_cost,
    one loss / optimiser for all sweeps, no rescale before the decomposition)"""
    return (numpy_dtype(opts.dtype) == np.dtype(np.float64) and opts.update_iters == 1 and not opts.track_cost
            and opts.d * max(opts.chi_max, opts.chi_init) <= 128 and 2 <= opts.d <= 16 and n_train <= 8192 and not opts.rescale[0]
            and not isinstance(opts.loss_grad, tuple) and not isinstance(opts.bbopt, tuple) and not opts.use_legacy_ITensor)


class _Fit:
    """a job on its engine, between build_caches and get_mps: fit_encoded's steps (RealRealHighDimension.jl:587-890), one at a time"""

    def __init__(self, idx, W, tr, te, opts, device, custom_encoding=None):
        self.idx, self.tr, self.te, self.opts, self.custom_encoding = idx, tr, te, opts, custom_encoding
        self.has_test = len(te) > 0
        self.sweeps_done, self.done, self.error = 0, False, None
        C = int(W[-1].shape[3])
        self.key = (len(W), opts.d, C, opts.chi_max, opts.chi_init, opts.loss_grad.upper(), bool(opts.train_classes_separately),
                    (len(tr) + 255) // 256)
        self.eng = SweepEngine(device)
        self.eng.set_batch_hint(BATCH_HINT)
        self.eng.set_options(rebuild_caches=False, track_cost=False, **engine_options(opts))
        self.eng.set_dataset(0, tr.phi, tr.label_index, C, dtype=np.float64)
        if self.has_test:
            self.eng.set_dataset(1, te.phi, te.label_index, C, dtype=np.float64)
        self.eng.set_mps(W)
        self.eng.build_caches()
        keys = ("train_loss", "train_acc", "test_loss", "time_taken", "train_KL_div")
        self.info = {k: [] for k in keys}
        if self.has_test:
            self.info.update({k: [] for k in ("test_acc", "test_KL_div", "test_conf")})
        self.log(0.0)
        if opts.nsweeps <= 0:
            self.done = True

    def log(self, time_taken):
        if self.opts.log_level <= 0:
            return None
        mse, kld, acc, _ = self.eng.eval(0)
        for k, v in (("train_loss", mse), ("train_acc", acc), ("time_taken", time_taken), ("train_KL_div", kld)):
            self.info[k].append(v)
        if self.has_test:
            tm, tk, ta, conf = self.eng.eval(1)
            for k, v in (("test_loss", tm), ("test_acc", ta), ("test_KL_div", tk), ("test_conf", conf)):
                self.info[k].append(v)
        return acc

    def after_sweep(self, seconds):
        self.sweeps_done += 1
        acc = self.log(seconds)
        if self.sweeps_done >= self.opts.nsweeps or (self.opts.exit_early and acc == 1.0):
            self.done = True

    def finish(self) -> BatchFit:
        try:
            if self.error is not None:
                return BatchFit(error=self.error, batched=True)
            self.eng.normalize()
            self.log(float("nan"))
            return BatchFit(TrainedMPS(self.eng.get_mps(), self.opts, self.tr, self.custom_encoding), self.info, self.te, True)
        finally:
            self.eng.close()


def fit_batch(jobs, device: int = 0, custom_encoding=None) -> List[BatchFit]:
    """Run many fitMPS jobs to completion together.  ``jobs``: (X_train, y_train, opts) tuples (a fourth and fifth entry: X_test,
    y_test).  Every job is encoded and gets its starting MPS exactly as fitMPS would; jobs of one shape (T, d, C, chi_max, chi_init,
    loss, train_classes_separately, and the same gradient share count) then advance together, sweep by sweep, in chunks of at most
    64 fits per launch chain (``sweep_batch``; the fits may differ in their series and class counts).  ``exit_early`` and a smaller
    ``nsweeps`` take a fit out of its group; a decomposition failure stops that fit alone (``error``).  Jobs the batched chain
    does not take (typed or complex fits, update_iters > 1, d chi_max > 128, track_cost, per-sweep losses) go through ``fitMPS`` one
    by one: ``batched`` is False for them.  Results are those of ``fitMPS(..., batch_hint=BATCH_HINT)``, bit for bit.
    ``custom_encoding``: the Encoding of the jobs whose options say ``encoding="Custom"``, as fitMPS takes it."""
    out: List[Optional[BatchFit]] = [None] * len(jobs)
    fits: List[_Fit] = []
    try:
        for i, job in enumerate(jobs):
            X_train, y_train, opts = job[0], job[1], safe_options(job[2])
            X_test = job[3] if len(job) > 3 else None
            y_test = job[4] if len(job) > 4 else None
            custom = custom_encoding if opts.encoding.lower() == "custom" else None
            if not _batchable(opts, len(X_train)):
                try:
                    m, info, te = fitMPS(X_train, y_train, X_test, y_test, opts=opts, device=device, custom_encoding=custom)
                    out[i] = BatchFit(m, info, te, False)
                except L.SVDError as err:
                    out[i] = BatchFit(error=err, batched=False)
                continue
            W, Xtr, ytr, Xte, yte, opts, enc, class_keys = _fit_inputs(X_train, y_train, X_test, y_test, opts, custom)
            tr, te = _encode_fit(Xtr, ytr, Xte, yte, opts, enc, class_keys)
            if opts.verbosity > -1:
                print(f"Using {opts.update_iters} iterations per update.")
            fits.append(_Fit(i, W, tr, te, opts, device, custom))
        while True:
            live = [f for f in fits if not f.done and f.error is None]
            if not live:
                break
            groups = {}
            for f in live:
                groups.setdefault(f.key, []).append(f)
            for members in groups.values():
                for c0 in range(0, len(members), MAX_BATCH):
                    _advance(members[c0:c0 + MAX_BATCH])
        for f in fits:
            out[f.idx] = f.finish()
        fits = []
    finally:
        for f in fits:
            f.eng.close()
    return out


def _advance(chunk):
    """one sweep of a chunk of fits of one shape"""
    try:
        st = sweep_batch([f.eng for f in chunk])
        for f, s in zip(chunk, st):
            f.after_sweep(s["seconds"])
    except L.SVDError as err:
        status = getattr(err, "svd_status", [1] * len(chunk))
        for f, bad in zip(chunk, status):
            if bad:
                f.error = L.SVDError(L.MPST_ERR_SVD, "bond-tensor decomposition failed in a batched fit")
            else:
                f.after_sweep(float("nan"))
    except L.MPSTError as err:
        if err.code != L.MPST_ERR_UNSUPPORTED:
            raise
        # fits the engine will not put into one chain after all (another gradient share count): their own sweeps, the same bits
        for f in chunk:
            try:
                f.after_sweep(f.eng.sweep()["seconds"])
            except L.SVDError as e2:
                f.error = e2


# ---- batched scoring -----------------------------------------------------------------------------------------------------------
def classify_many(models: List[TrainedMPS], X_vals, device: int = 0):
    """``classify(models[k], X_vals[k])`` for all k, the models of one shape scored together by ``classify_batch``; models that
    call does not take are classified one by one.  Returns (predictions, number scored in batches)."""
    preds = [None] * len(models)
    groups = {}
    for k, m in enumerate(models):
        opts = safe_options(m.opts)
        chi = max(t.shape[2] for t in m.mps)
        if numpy_dtype(opts.dtype) == np.dtype(np.float64) and opts.d * max(chi, opts.chi_max) <= 128 and len(X_vals[k]) > 0:
            groups.setdefault((len(m.mps), opts.d, int(m.mps[-1].shape[3])), []).append(k)
        else:
            preds[k] = classify(m, X_vals[k], device=device)
    nb = 0
    for (T, d, C), ks in groups.items():
        for c0 in range(0, len(ks), MAX_BATCH):
            chunk = ks[c0:c0 + MAX_BATCH]
            engs = []
            try:
                for k in chunk:
                    m = models[k]
                    states = classify_states(m, X_vals[k])
                    e = SweepEngine(device)
                    e.set_options(**engine_options(safe_options(m.opts)))
                    e.set_dataset(0, m.train_data.phi[:1], m.train_data.label_index[:1], C)
                    e.set_dataset(1, states.phi, np.zeros(len(states), dtype=np.int32), C)
                    e.set_mps(m.mps)
                    engs.append(e)
                res = classify_batch(engs, 1)
            finally:
                for e in engs:
                    e.close()
            for k, r in zip(chunk, res):
                preds[k] = np.unique(models[k].train_data.labels)[r["pred"]]
            nb += len(chunk)
    return preds, nb


# ---- tune (tuning.jl) ---------------------------------------------------------------------------------------------------------
def default_opts0(objective):
    return MPSOptions(verbosity=-5, log_level=-1, sigmoid_transform=isinstance(objective, ClassificationLoss))


def tune(Xs, ys, nfolds, parameters, optimiser=MPSRandomSearch(), objective=None, opts0=None, windows=None, pms=None,
         logspace_eta=False, maxiters=250, rng=1, foldmethod=make_stratified_cvfolds, verbosity=1, method="median", device=0,
         return_info=False, custom_encoding=None):
    """tune (tuning.jl:209-512): k-fold cross-validated search over ``parameters`` (``key=[values]``, ``key=(lb, ub)``,
    ``key=(lb, step, ub)``; numeric MPSOptions fields only).  Returns ``(best_params, cache)`` - ``best_params`` a dict of option
    values, ``cache`` {tuple of option values in key order: mean loss over the folds}; with ``return_info`` a third entry
    {"fits", "batched_fits", "fallback_fits", "failed_fits", "batched_scores"}.  A candidate's loss is the mean over folds of
    ``mean(eval_loss(...))``, a diverged fit scores inf, the first strict minimum in trial order wins.  All trials x folds fits go
    to ``fit_batch`` at once and are scored with ``classify_batch`` (ImputationLoss: ``impute_dataset`` per model).  ``rng``: a
    NumPy seed or Generator - not Julia's stream; ``foldmethod``: a callable (Xs, ys, nfolds, rng=) or a list of
    (train_inds, val_inds) pairs, used as is.  ``custom_encoding``: the Encoding behind ``opts0.encoding == "Custom"``."""
    objective = ImputationLoss() if objective is None else objective
    opts0 = default_opts0(objective) if opts0 is None else safe_options(opts0)
    nparams = len(parameters)
    if nparams == 0 or nfolds == 0 or maxiters == 0:
        return (opts0, {}) + (({},) if return_info else ())
    if not isinstance(optimiser, MPSRandomSearch):
        raise NotImplementedError("only MPSRandomSearch is implemented (the reference's Optimization.jl solvers are not reproduced)")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    pinfo = parse_parameters(parameters, opts0, logspace_eta)
    if isinstance(objective, ImputationLoss):
        windows = make_windows(windows, pms, Xs, rng)
    Xs, ys = np.asarray(Xs, dtype=np.float64), np.asarray(ys)
    if nfolds <= 1:
        best = dict(zip(pinfo.fields, pinfo.safe_paramlist(pinfo.x0)))
        return (best, {}) + (({},) if return_info else ())
    folds = foldmethod(Xs, ys, nfolds, rng=rng) if callable(foldmethod) else list(foldmethod)
    trials = sort_trials(make_grid(rng, optimiser.sampling, pinfo.lb, pinfo.ub, pinfo.is_disc, maxiters), pinfo.fields)
    keys = [pinfo.safe_paramlist(t) for t in trials]
    todo = list(dict.fromkeys(keys))               # candidates repeated after rounding hit the cache
    jobs = []
    for key in todo:
        opts = opts0.set(**dict(zip(pinfo.fields, key)))
        for tr_i, _ in folds[:nfolds]:
            jobs.append((Xs[tr_i], ys[tr_i], opts))
    t0 = time.time()
    fits = fit_batch(jobs, device=device, **({} if custom_encoding is None else {"custom_encoding": custom_encoding}))
    X_vals = [Xs[va] for _ in todo for _, va in folds[:nfolds]]
    y_vals = [ys[va] for _ in todo for _, va in folds[:nfolds]]
    ok = [k for k, f in enumerate(fits) if f.error is None]
    losses = [float("inf")] * len(fits)
    nb = 0
    if isinstance(objective, ImputationLoss):
        for k in ok:
            losses[k] = float(np.mean(_imputation_loss(fits[k].mps, X_vals[k], y_vals[k], windows, method, device=device)))
    else:
        preds, nb = classify_many([fits[k].mps for k in ok], [X_vals[k] for k in ok], device=device)
        for k, p in zip(ok, preds):
            losses[k] = float(np.mean(_classification_loss(objective, y_vals[k], p)))
    cache = {}
    for c, key in enumerate(todo):
        cache[key] = float(np.mean(losses[c * nfolds:(c + 1) * nfolds]))
        if verbosity >= 1:
            print(f"iter {c + 1}, t={time.time() - t0:.2f}: {dict(zip(pinfo.fields, key))} Mean CV Loss: {cache[key]}")
    best_key, best_loss = None, float("inf")
    for key in keys:                               # the first strict minimum in trial order
        if cache[key] < best_loss:
            best_key, best_loss = key, cache[key]
    if best_key is None:                           # every candidate diverged: the reference's trials[-1] is not reproduced
        raise RuntimeError("every candidate of tune() diverged (all losses are inf)")
    best = dict(zip(pinfo.fields, best_key))
    info = {"fits": len(fits), "batched_fits": sum(1 for f in fits if f.batched and f.error is None),
            "fallback_fits": sum(1 for f in fits if not f.batched), "failed_fits": len(fits) - len(ok), "batched_scores": nb}
    return (best, cache) + ((info,) if return_info else ())


# ---- evaluate (evaluate.jl:136-306) -------------------------------------------------------------------------------------------
def _jsonable(x):
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    return x


def evaluate(Xs, ys, nfolds, tuning_parameters, tuning_optimiser=MPSRandomSearch(), objective=None, verbosity=1, opts0=None,
             tuning_opts0=None, n_cvfolds=5, fold_inds=None, logspace_eta=False, rng=1, tuning_rng=None,
             foldmethod=make_stratified_cvfolds, tuning_foldmethod=make_stratified_cvfolds, eval_pms=None, eval_windows=None,
             tuning_pms=None, tuning_windows=None, tuning_maxiters=250, write=False, writedir="evals", simname=None,
             overwrite=False, method="median", device=0, custom_encoding=None):
    """evaluate (evaluate.jl:136-306): the outer resampling loop.  For every outer fold ``tune`` runs on its training part with
    ``n_cvfolds`` inner folds, then a model with the best options is trained on the whole training part and scored on the test
    part.  The final fits of all outer folds form ONE ``fit_batch``.  Returns one dict per fold of ``fold_inds`` (0-based) with
    the reference's keys: fold, objective, train_inds, test_inds, optimiser, tuning_windows, tuning_pms, eval_windows, eval_pms,
    time, opts, cache, loss.  ``write``: every fold is stored as ``<writedir>/<simname>_tmp/f<fold>.json`` (+ ``.npz``: the
    trained model, save_trained_mps's format) and a fold found there is loaded instead of being refitted (``overwrite`` refits).
    Folds and grids follow NumPy seeds, not Julia's streams.  ``custom_encoding``: the Encoding behind ``encoding="Custom"``."""
    objective = ImputationLoss() if objective is None else objective
    opts0 = default_opts0(objective) if opts0 is None else safe_options(opts0)
    tuning_opts0 = opts0 if tuning_opts0 is None else safe_options(tuning_opts0)
    Xs, ys = np.asarray(Xs, dtype=np.float64), np.asarray(ys)
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    fold_inds = list(range(nfolds)) if fold_inds is None else list(fold_inds)
    tuning_rng = list(range(1, nfolds + 1)) if tuning_rng is None else list(tuning_rng)
    if tuning_pms is None and tuning_windows is None:
        tuning_pms, tuning_windows = eval_pms, eval_windows
    if isinstance(objective, ImputationLoss):
        eval_windows = make_windows(eval_windows, eval_pms, Xs, rng)
    folds = foldmethod(Xs, ys, nfolds, rng=rng) if callable(foldmethod) else list(foldmethod)
    simname = simname or f"{objective}_{tuning_optimiser.sampling}_f={nfolds}_cv={n_cvfolds}_iters={tuning_maxiters}"
    tmpdir = os.path.join(writedir, simname + "_tmp")
    if write:
        os.makedirs(tmpdir, exist_ok=True)
    results, pending = {}, []
    for fold in fold_inds:
        fname = os.path.join(tmpdir, f"f{fold}.json")
        if write and os.path.isfile(fname) and not overwrite:
            verbosity > -1 and print(f"Fold {fold} already exists, skipping...")
            with open(fname) as fh:
                res = json.load(fh)
            res["opts"] = MPSOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in res["opts"].items()})
            res["cache"] = {tuple(k): v for k, v in res["cache"]}
            res["train_inds"], res["test_inds"] = np.asarray(res["train_inds"]), np.asarray(res["test_inds"])
            results[fold] = res
            continue
        verbosity > -1 and print(f"Beginning fold {fold}:")
        tbeg = time.time()
        tr_i, te_i = folds[fold]
        irng = tuning_rng[fold] if isinstance(tuning_rng[fold], np.random.Generator) else np.random.default_rng(tuning_rng[fold])
        tw = make_windows(tuning_windows, tuning_pms, Xs, irng) if isinstance(objective, ImputationLoss) else None
        best, cache = tune(Xs[tr_i], ys[tr_i], n_cvfolds, tuning_parameters, tuning_optimiser, objective=objective, opts0=tuning_opts0,
                           windows=tw, logspace_eta=logspace_eta, maxiters=tuning_maxiters, rng=irng, foldmethod=tuning_foldmethod,
                           verbosity=verbosity - 1, method=method, device=device,
                           **({} if custom_encoding is None else {"custom_encoding": custom_encoding}))
        opts = best if isinstance(best, MPSOptions) else opts0.set(**best)
        pending.append((fold, tbeg, opts, cache))
    finals = fit_batch([(Xs[folds[f][0]], ys[folds[f][0]], o) for f, _, o, _ in pending], device=device,
                       **({} if custom_encoding is None else {"custom_encoding": custom_encoding}))
    for (fold, tbeg, opts, cache), fit in zip(pending, finals):
        tr_i, te_i = folds[fold]
        if fit.error is not None:
            raise fit.error
        res = {"fold": fold, "objective": repr(objective), "train_inds": np.asarray(tr_i), "test_inds": np.asarray(te_i),
               "optimiser": repr(tuning_optimiser), "tuning_windows": tuning_windows, "tuning_pms": tuning_pms,
               "eval_windows": eval_windows, "eval_pms": eval_pms, "time": None, "opts": opts, "cache": cache,
               "loss": eval_loss(objective, fit.mps, Xs[te_i], ys[te_i], eval_windows, method=method, device=device)}
        res["time"] = time.time() - tbeg
        if write:
            d = dict(res)
            d["opts"] = opts.asdict()
            d["cache"] = [[list(k), v] for k, v in cache.items()]
            with open(os.path.join(tmpdir, f"f{fold}.json"), "w") as fh:
                json.dump(_jsonable(d), fh)
            save_trained_mps(os.path.join(tmpdir, f"f{fold}.npz"), fit.mps)
            verbosity > -1 and print(f"saved fold at {os.path.join(tmpdir, f'f{fold}.json')}")
        results[fold] = res
    out = [results[f] for f in fold_inds]
    if write:
        with open(os.path.join(writedir, simname + ".json"), "w") as fh:
            d = [dict(r, opts=r["opts"].asdict(), cache=[[list(k), v] for k, v in r["cache"].items()]) for r in out]
            json.dump(_jsonable(d), fh)
    return out
