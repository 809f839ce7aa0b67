"""The reference's summaries (src/summary.jl:225-456): ``get_training_summary``, ``sweep_summary`` and ``print_opts``.

The tables are plain text (the reference prints them with PrettyTables; its colours and highlighters are not reproduced).  The class
overlap matrix and the per-class norms come from the device (``overlaps.model_overlaps``), the overlaps of the series with the model
from the engine's classification path; ``training_stats`` is the arithmetic on the predictions and needs no device.
"""
from __future__ import annotations

import sys
from dataclasses import fields
from typing import Optional

import numpy as np

from .encodings import EncodedTimeSeriesSet
from .engine import SweepEngine
from .options import engine_options, safe_options
from .overlaps import model_overlaps
from .training import TrainedMPS, classify_states


def _table(io, title, header, row_labels, cells):
    """A boxed text table: ``cells`` are strings, every column as wide as its widest entry, the title centred over it."""
    rows = [[""] + list(header)] + [[r] + list(c) for r, c in zip(row_labels, cells)]
    width = [max(len(row[j]) for row in rows) for j in range(len(rows[0]))]
    rule = "+" + "+".join("-" * (w + 2) for w in width) + "+"
    if title:
        print(title.center(len(rule)), file=io)
    print(rule, file=io)
    for row in rows:
        print("|" + "|".join(" " + x.center(w) + " " for x, w in zip(row, width)) + "|", file=io)
        print(rule, file=io)


def training_stats(true_train, pred_train, true_test, pred_test, C):
    """The statistics of ``get_training_summary`` from class indices in 0..C-1.  ``confmat`` (C, C), integer, is [true][pred] of the test
    set (MLBase.confusmat).  The reference takes the multiclass metrics from MLJBase; they are defined here as the macro average - the
    plain mean over the classes - of the per-class formulas on the confusion matrix, with TP = confmat[c, c], FP and FN the rest of
    column and row c, TN the rest of the matrix:
        precision TP / (TP + FP), recall TP / (TP + FN), specificity TN / (TN + FP), f1_score 2 TP / (2 TP + FP + FN),
    and ``test_balanced_acc`` is the mean per-class recall.  A 0/0 stays NaN and makes the average NaN: a class that is never predicted
    has no precision."""
    true_train, pred_train = np.asarray(true_train, dtype=np.int64), np.asarray(pred_train, dtype=np.int64)
    true_test, pred_test = np.asarray(true_test, dtype=np.int64), np.asarray(pred_test, dtype=np.int64)
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (true_test, pred_test), 1)
    tp = np.diag(conf).astype(np.float64)
    fp, fn = conf.sum(axis=0) - tp, conf.sum(axis=1) - tp
    tn = conf.sum() - tp - fp - fn
    with np.errstate(divide="ignore", invalid="ignore"):
        precision, recall, specificity, f1 = tp / (tp + fp), tp / (tp + fn), tn / (tn + fp), 2 * tp / (2 * tp + fp + fn)
        train_acc = np.float64(np.sum(true_train == pred_train)) / np.float64(len(true_train))
        test_acc = np.float64(np.sum(true_test == pred_test)) / np.float64(len(true_test))
    return {"train_acc": float(train_acc), "test_acc": float(test_acc), "test_balanced_acc": float(np.mean(recall)),
            "precision": float(np.mean(precision)), "recall": float(np.mean(recall)), "specificity": float(np.mean(specificity)),
            "f1_score": float(np.mean(f1)), "confmat": conf}


def normalised_predictions(yhat, log_norm):
    """argmax_c |yhat_c| / ||psi_c||, the first maximum on ties: classify_overlap on the normalised class states of expand_label_index
    (src/summary.jl:182-202, src/utils.jl:356-370).  A class whose state is zero never wins."""
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.abs(np.asarray(yhat)) / np.exp(np.asarray(log_norm))[None, :]
    return np.argmax(np.where(np.isnan(score), -np.inf, score), axis=1)


def get_training_summary(mps: TrainedMPS, test, print_stats: bool = False, io=None, engine: Optional[SweepEngine] = None, device: int = 0,
                         y_test=None):
    """get_training_summary([io], mps, test_states; print_stats) (src/summary.jl:225-370): prints the overlap matrix of the class
    states (%5.3e) and the confusion matrix of the test set, with ``print_stats`` also the scalar statistics, and returns the dict
    ``train_acc, test_acc, test_balanced_acc, precision, recall, specificity, f1_score, confmat`` plus, as an extension, ``overlapmat``.

    ``test``: an EncodedTimeSeriesSet, or a raw matrix, which goes through ``classify_states`` (the model's own preprocessing); a raw
    matrix carries no labels, so ``y_test`` gives them (the original label values; without it every series counts as the first class).
    Predictions are argmax_c |yhat_c| / ||psi_c|| with the first maximum on ties: the reference normalises every class state
    (expand_label_index), so they can differ from ``classify``, which uses the states as stored.  yhat comes from the engine's
    classification path, the norms and the overlap matrix from ``model_overlaps``.  The metrics are the macro averages documented in
    ``training_stats`` (the reference's come from MLJBase)."""
    io = sys.stdout if io is None else io
    opts = safe_options(mps.opts)
    labels = np.unique(mps.train_data.labels)
    states = classify_states(mps, test)
    if isinstance(test, EncodedTimeSeriesSet):
        true_test = np.asarray(states.label_index, dtype=np.int64)
    elif y_test is not None:
        true_test = np.searchsorted(labels, np.asarray(y_test))
    else:
        true_test = np.zeros(len(states), dtype=np.int64)
    Cn = int(mps.mps[-1].shape[3])
    own = engine is None
    eng = engine or SweepEngine(device)
    try:
        ov = model_overlaps([mps], engine=eng)
        eng.set_options(**engine_options(opts))
        eng.set_dataset(0, mps.train_data.phi, mps.train_data.label_index, Cn)
        eng.set_dataset(1, states.phi, np.zeros(len(states), dtype=np.int32), Cn)
        eng.set_mps(mps.mps)
        _, yh_train = eng.classify(0, return_overlaps=True)
        _, yh_test = eng.classify(1, return_overlaps=True)
    finally:
        if own:
            eng.close()
    pred_train, pred_test = normalised_predictions(yh_train, ov.log_norm[0]), normalised_predictions(yh_test, ov.log_norm[0])
    stats = training_stats(mps.train_data.label_index, pred_train, true_test, pred_test, Cn)
    stats["overlapmat"] = ov.fidelity
    names = [str(n) for n in labels.tolist()]
    print(file=io)
    _table(io, "Overlap Matrix", [f"|ψ{n}⟩" for n in names], [f"⟨ψ{n}|" for n in names], [["%5.3e" % v for v in row] for row in ov.fidelity])
    _table(io, "Confusion Matrix", [f"Pred. |{n}⟩" for n in names], [f"True |{n}⟩" for n in names], [[str(int(v)) for v in row] for row in stats["confmat"]])
    if print_stats:
        keys = [k for k in stats if k not in ("confmat", "overlapmat")]
        _table(io, "", keys, [""], [[repr(stats[k]) for k in keys]])
    return stats


def sweep_summary(info, io=None):
    """sweep_summary([io], info) (src/summary.jl:380-430) of the training information ``fitMPS`` returns: rows Train Accuracy, Test Accuracy,
    Train KL Div., Test KL Div., Time taken (the test rows only when ``info`` has them); columns Initial, After Sweep 1..n, After Norm,
    Mean - the mean of the After Sweep entries only (:389).  Prints the table and returns its matrix (rows, nsweeps + 3)."""
    io = sys.stdout if io is None else io
    nsweeps = len(info["time_taken"]) - 2
    rows = [("Train Accuracy", "train_acc"), ("Test Accuracy", "test_acc"), ("Train KL Div.", "train_KL_div"), ("Test KL Div.", "test_KL_div"),
            ("Time taken", "time_taken")]
    rows = [(name, key) for name, key in rows if key in info]
    header = ["Initial"] + [f"After Sweep {n}" for n in range(1, nsweeps + 1)] + ["After Norm", "Mean"]
    data = np.zeros((len(rows), nsweeps + 3))
    for i, (_, key) in enumerate(rows):
        v = np.asarray(info[key], dtype=np.float64)
        data[i, :-1] = v
        data[i, -1] = np.mean(v[1:-1]) if nsweeps > 0 else np.nan
    _table(io, "", header, [name for name, _ in rows], [["%.6g" % x for x in row] for row in data])
    return data


def print_opts(opts, long: bool = False, io=None):
    """print_opts([io], opts; long) (src/summary.jl:438-456): the options in a one-row table - chi_max, d, eta, nsweeps, encoding,
    sigmoid_transform and loss_grad, or with ``long`` every field."""
    io = sys.stdout if io is None else io
    opts = safe_options(opts)
    params = [f.name for f in fields(opts)] if long else ["chi_max", "d", "eta", "nsweeps", "encoding", "sigmoid_transform", "loss_grad"]
    _table(io, "", params, [""], [[str(getattr(opts, k)) for k in params]])
