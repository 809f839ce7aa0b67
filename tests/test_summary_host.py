"""The host side of the summaries (mpstime.jl_amd/summary.py) without a device: the statistics of get_training_summary on a
hand-written example, sweep_summary and print_opts on a fabricated training record."""
import io

import numpy as np

import mpstime_jl_amd as mt
from mpstime_jl_amd.summary import normalised_predictions


def test_training_stats_three_classes():
    #          true: 0 0 0 0 1 1 1 2 2 2      pred: class 2 is never predicted
    true_test = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    pred_test = [0, 0, 0, 1, 1, 1, 0, 0, 1, 1]
    s = mt.training_stats([0, 1, 2, 2], [0, 1, 2, 0], true_test, pred_test, 3)
    assert s["confmat"].dtype.kind == "i" and s["confmat"].tolist() == [[3, 1, 0], [1, 2, 0], [1, 2, 0]]       # [true][pred]
    assert s["train_acc"] == 0.75 and s["test_acc"] == 0.5
    # per class: TP 3 2 0, FP 2 3 0, FN 1 1 3, TN 4 4 7
    recall = np.array([3 / 4, 2 / 3, 0.0])
    assert abs(s["recall"] - recall.mean()) <= 1e-15 and s["test_balanced_acc"] == s["recall"]
    assert abs(s["specificity"] - np.mean([4 / 6, 4 / 7, 1.0])) <= 1e-15
    assert abs(s["f1_score"] - np.mean([6 / 9, 4 / 8, 0.0])) <= 1e-15
    assert np.isnan(s["precision"])                                             # 0 / 0 for the class that is never predicted
    # with every class predicted the macro precision is the plain mean
    s2 = mt.training_stats([0], [0], [0, 1, 2, 2], [0, 1, 2, 1], 3)
    assert abs(s2["precision"] - np.mean([1.0, 0.5, 1.0])) <= 1e-15 and s2["confmat"].sum() == 4


def test_normalised_predictions_divide_by_the_norm_and_take_the_first_maximum():
    yhat = np.array([[2.0, -1.0, 0.5], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0 + 1.0j, 0.1, 0.1]])
    log_norm = np.log([4.0, 1.0, 0.25])
    assert normalised_predictions(yhat, log_norm).tolist() == [2, 2, 0, 2]
    assert normalised_predictions(np.abs(yhat), np.zeros(3)).tolist() == [0, 0, 0, 0]
    dead = np.array([[0.5, 0.0, 2.0], [1.0, 0.0, 1.0]])                          # a zero state has zero overlaps: 0 / 0 never wins
    assert normalised_predictions(dead, np.array([0.0, -np.inf, 0.0])).tolist() == [2, 0]


def _info(nsweeps, test):
    n = nsweeps + 2
    info = {"train_loss": list(np.linspace(1.0, 0.1, n)), "train_acc": list(np.linspace(0.5, 0.9, n)), "train_KL_div": list(np.linspace(2.0, 0.5, n)),
            "time_taken": [0.0] + [0.25 * (k + 1) for k in range(nsweeps)] + [float("nan")]}
    if test:
        info.update(test_acc=list(np.linspace(0.4, 0.8, n)), test_KL_div=list(np.linspace(2.5, 0.7, n)), test_loss=list(np.linspace(1.0, 0.2, n)),
                    test_conf=[np.eye(2)] * n)
    return info


def test_sweep_summary():
    out = io.StringIO()
    info = _info(3, True)
    data = mt.sweep_summary(info, io=out)
    assert data.shape == (5, 6)
    for i, key in enumerate(["train_acc", "test_acc", "train_KL_div", "test_KL_div", "time_taken"]):
        assert np.array_equal(data[i, :5], np.asarray(info[key], dtype=float), equal_nan=True)
        assert abs(data[i, 5] - np.mean(info[key][1:-1])) <= 1e-15             # the After Sweep entries only
    assert data[4, 5] == 0.5 and np.isnan(data[4, 4])
    text = out.getvalue()
    for word in ["Train Accuracy", "Test Accuracy", "Train KL Div.", "Test KL Div.", "Time taken", "Initial", "After Sweep 1", "After Sweep 2",
                 "After Sweep 3", "After Norm", "Mean"]:
        assert word in text, word
    assert "After Sweep 4" not in text
    # without a test set the test rows are left out
    out = io.StringIO()
    data = mt.sweep_summary(_info(2, False), io=out)
    assert data.shape == (3, 5) and "Test" not in out.getvalue() and "Train KL Div." in out.getvalue()


def test_print_opts():
    opts = mt.MPSOptions(chi_max=17, d=6, eta=0.125, nsweeps=3, encoding="fourier", sigmoid_transform=False)
    out = io.StringIO()
    assert mt.print_opts(opts, io=out) is None
    text = out.getvalue()
    for word in ["chi_max", "17", "eta", "0.125", "nsweeps", "encoding", "fourier", "sigmoid_transform", "False", "loss_grad", "KLD"]:
        assert word in text, word
    assert "cutoff" not in text and "bbopt" not in text
    out = io.StringIO()
    mt.print_opts(opts, long=True, io=out)
    for name in opts.asdict():
        assert name in out.getvalue(), name
