"""Host side of tune / evaluate (mpstime.jl_amd/tuning.py): folds, grids, parameter mapping, loss arithmetic, windows.  No GPU."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import tuning as tu


def _labels():
    return np.array([0] * 23 + [1] * 31 + [2] * 7)


def test_stratified_folds_partition_and_balance():
    ys = _labels()
    X = np.zeros((len(ys), 3))
    folds = mt.make_stratified_cvfolds(X, ys, 3, rng=5)
    assert len(folds) == 3
    allval = np.sort(np.concatenate([v for _, v in folds]))
    assert np.array_equal(allval, np.arange(len(ys)))                      # the validation parts partition the indices
    for tr, va in folds:
        assert np.array_equal(np.sort(np.concatenate([tr, va])), np.arange(len(ys)))
    for cls in np.unique(ys):
        sizes = [int(np.sum(ys[va] == cls)) for _, va in folds]
        assert max(sizes) - min(sizes) <= 1
    again = mt.make_stratified_cvfolds(X, ys, 3, rng=5)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(folds, again))
    other = mt.make_stratified_cvfolds(X, ys, 3, rng=6)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(folds, other))
    plain = mt.make_stratified_cvfolds(X, ys, 3, rng=5, shuffle=False)
    assert np.array_equal(plain[0][1][:3], [0, 3, 6])


def test_fold_list_is_used_verbatim(monkeypatch):
    ys = _labels()
    X = np.arange(len(ys) * 3, dtype=float).reshape(len(ys), 3)
    mine = [(np.arange(10, 61), np.arange(10)), (np.r_[0:10, 30:61], np.arange(10, 30))]
    jobs_seen, vals_seen = [], []

    def fake_fit_batch(jobs, device=0):
        jobs_seen.extend(jobs)
        return [tu.BatchFit(mps="model", batched=True) for _ in jobs]

    def fake_classify_many(models, X_vals, device=0):
        vals_seen.extend(X_vals)
        return [np.zeros(len(x), dtype=np.int64) for x in X_vals], len(models)

    monkeypatch.setattr(tu, "fit_batch", fake_fit_batch)
    monkeypatch.setattr(tu, "classify_many", fake_classify_many)
    tu.tune(X, ys, 2, {"chi_max": [8]}, mt.MPSRandomSearch("Exhaustive"), objective=mt.MisclassificationRate(), foldmethod=mine, verbosity=0)
    assert len(jobs_seen) == 2
    for (Xtr, ytr, _), xv, (tr, va) in zip(jobs_seen, vals_seen, mine):
        assert np.array_equal(Xtr, X[tr]) and np.array_equal(ytr, ys[tr]) and np.array_equal(xv, X[va])
    # nfolds <= 1: the start values (25 lies outside (8, 10): the lower bound), no folds, no fits; nfolds == 0: opts0 back
    assert tu.tune(X, ys, 1, {"chi_max": (8, 10)}, objective=mt.MisclassificationRate(), foldmethod=mine) == ({"chi_max": 8}, {})
    assert tu.tune(X, ys, 0, {"chi_max": (8, 10)}, objective=mt.MisclassificationRate())[1] == {}
    assert len(jobs_seen) == 2


def test_exhaustive_grid_in_reference_order():
    opts0 = mt.MPSOptions(verbosity=-5)
    p = tu.parse_parameters({"d": (3, 4), "chi_max": (8, 10)}, opts0)
    assert p.fields == ["chi_max", "d"] and p.is_disc == [True, True]       # sorted by name (tuning.jl:481-487)
    raw = tu.make_grid(None, "Exhaustive", p.lb, p.ub, p.is_disc, 250)
    assert raw == [[8, 3], [9, 3], [10, 3], [8, 4], [9, 4], [10, 4]]         # Iterators.product: first parameter fastest
    trials = tu.sort_trials(raw, p.fields)
    # stable, descending in chi_max * d: 40, 36, 32, 30, 27, 24
    assert trials == [[10, 4], [9, 4], [8, 4], [10, 3], [9, 3], [8, 3]]
    assert [p.safe_paramlist(t) for t in trials][0] == (10, 4)
    # ties (2 * 2 = 1 * 4) keep the product order: [2, 2] was made before [1, 4]
    q = tu.parse_parameters({"d": (2, 4), "chi_max": [4, 8]}, opts0)        # chi_max as a value list: the raw entries are indices
    t2 = tu.sort_trials(tu.make_grid(None, "Exhaustive", q.lb, q.ub, q.is_disc, 250), q.fields)
    assert t2 == [[2, 4], [2, 3], [2, 2], [1, 4], [1, 3], [1, 2]]
    with pytest.raises(ValueError, match="discrete"):
        r = tu.parse_parameters({"eta": (0.01, 0.1)}, opts0)
        tu.make_grid(None, "Exhaustive", r.lb, r.ub, r.is_disc, 4)


def test_latin_hypercube_and_uniform_random():
    rng = np.random.default_rng(3)
    n = 7
    g = tu.make_grid(rng, "LatinHypercube", [0.0, 1], [1.0, 3], [False, True], n)
    assert len(g) == n
    strata = sorted(min(int(x[0] * n), n - 1) for x in g)
    assert strata == list(range(n))                                         # each of the n strata once
    counts = np.bincount([x[1] for x in g], minlength=4)[1:]
    assert counts.max() - counts.min() <= 1 and counts.sum() == n
    u = tu.make_grid(np.random.default_rng(4), "UniformRandom", [1, 1], [3, 2], [True, True], 6)
    assert len(u) == 6 and len({tuple(x) for x in u}) == 6                  # 6 distinct points of a 3 x 2 grid: rerolled
    with pytest.raises(ValueError):
        mt.MPSRandomSearch("Sobol")
    assert mt.MPSRandomSearch(":Exhaustive").sampling == "Exhaustive"


def test_parameter_formats_rounding_and_logspace():
    opts0 = mt.MPSOptions(verbosity=-5, eta=0.05, chi_max=20)
    p = tu.parse_parameters({"eta": (1e-3, 1e-1), "chi_max": [30, 10, 20], "d": (2, 2, 8)}, opts0, logspace_eta=True)
    assert p.fields == ["chi_max", "d", "eta"]
    assert p.value_map[0] == [10, 20, 30] and p.value_map[1] == [2, 4, 6, 8] and p.value_map[2] == []
    assert (p.lb[0], p.ub[0]) == (1, 3) and (p.lb[1], p.ub[1]) == (1, 4)
    assert np.allclose([p.lb[2], p.ub[2]], [-3.0, -1.0]) and p.is_disc == [True, True, False]
    assert p.safe_paramlist([2, 3, -2.0]) == (20, 6, pytest.approx(0.01))
    # integer parameters are rounded: two raw trials, one candidate
    q = tu.parse_parameters({"chi_max": (8, 12)}, opts0)
    assert q.safe_paramlist([9.4]) == q.safe_paramlist([8.6]) == (9,)
    assert isinstance(q.safe_paramlist([9.4])[0], int)
    # start value outside the bounds: the lower bound
    assert q.x0 == [8]
    with pytest.raises(ValueError, match="only numeric types"):
        tu.parse_parameters({"encoding": ["Legendre", "Fourier"]}, opts0)
    with pytest.raises(ValueError, match="only numeric types"):
        tu.parse_parameters({"exit_early": [0, 1]}, opts0)
    with pytest.raises(ValueError, match="duplicates"):
        tu.parse_parameters([("eta", (0.01, 0.1)), ("eta", (0.02, 0.2))], opts0)
    with pytest.raises(ValueError, match="logspace_eta"):
        tu.parse_parameters({"eta": [0.01, 0.1]}, opts0, logspace_eta=True)
    with pytest.raises(ValueError, match="positive"):
        tu.parse_parameters({"eta": (0.0, 0.1)}, opts0, logspace_eta=True)
    with pytest.raises(ValueError, match="Unknown parameter format"):
        tu.parse_parameters({"eta": (0.1,)}, opts0)


def test_repeated_candidates_hit_the_cache(monkeypatch):
    """two trials that round to the same options are fitted once"""
    ys = _labels()
    X = np.random.default_rng(0).normal(size=(len(ys), 6))
    calls = []

    def fake_fit_batch(jobs, device=0):
        calls.append(len(jobs))
        return [tu.BatchFit(mps=("model", j[2].chi_max), batched=True) for j in jobs]

    def fake_classify_many(models, X_vals, device=0):
        return [np.zeros(len(x), dtype=np.int64) for x in X_vals], len(models)

    monkeypatch.setattr(tu, "fit_batch", fake_fit_batch)
    monkeypatch.setattr(tu, "classify_many", fake_classify_many)
    monkeypatch.setattr(tu, "make_grid", lambda *a, **k: [[8.2], [8.4], [9.7]])
    best, cache, info = tu.tune(X, ys, 3, {"chi_max": (8, 12)}, mt.MPSRandomSearch("UniformRandom"), objective=mt.MisclassificationRate(),
                                maxiters=3, verbosity=0, return_info=True)
    assert calls == [2 * 3] and set(cache) == {(8,), (10,)}                 # 8.2 and 8.4 are one candidate
    assert best == {"chi_max": 10}                                          # equal losses: the first in trial order (10 sorts first)
    assert info["fits"] == 6 and info["fallback_fits"] == 0
    with pytest.raises(NotImplementedError):
        tu.tune(X, ys, 3, {"chi_max": (8, 12)}, optimiser="LBFGS", objective=mt.MisclassificationRate())
    o = mt.MPSOptions(verbosity=-5)
    assert tu.tune(X, ys, 3, {}, opts0=o, objective=mt.MisclassificationRate()) == (o, {})
    assert tu.tune(X, ys, 3, {"chi_max": (8, 12)}, opts0=o, objective=mt.MisclassificationRate(), maxiters=0) == (o, {})


def test_loss_arithmetic():
    y = np.array([0, 0, 0, 1, 1, 2])
    pred = np.array([0, 0, 1, 1, 3, 2])
    assert tu.misclassification_rate(y, pred) == [pytest.approx(2 / 6)]
    # recalls: class 0 2/3, class 1 1/2, class 2 1, class 3 (predictions only) 0 -> mean over FOUR classes
    eps = np.finfo(float).eps
    want = 1.0 - (2 / (3 + eps) + 1 / (2 + eps) + 1 / (1 + eps) + 0.0 / (0 + eps)) / 4
    got = tu.balanced_misclassification_rate(y, pred)
    assert len(got) == 1 and got[0] == pytest.approx(want, abs=1e-15)
    assert tu.balanced_misclassification_rate(y, y) == [pytest.approx(0.0, abs=1e-15)]
    assert repr(mt.BalancedMisclassificationRate()) == "BalancedMisclassificationRate()"
    assert isinstance(mt.MisclassificationRate(), mt.ClassificationLoss) and not isinstance(mt.ImputationLoss(), mt.ClassificationLoss)


def test_make_windows():
    X = np.zeros((4, 20))
    with pytest.raises(ValueError, match="both"):
        mt.make_windows([np.arange(3)], [0.2], X)
    with pytest.raises(ValueError, match="either"):
        mt.make_windows(None, None, X)
    w = [np.arange(3), np.arange(5, 9)]
    assert mt.make_windows(w, None, X) == w
    assert [list(x) for x in mt.make_windows({"b": [np.arange(2)], "a": [np.arange(4, 6)]}, None, X)] == [[4, 5], [0, 1]]
    ws = mt.make_windows(None, [0.25, 0.5], X, np.random.default_rng(1))
    assert [len(x) for x in ws] == [5, 10] and all(np.all(np.diff(x) == 1) for x in ws)
    again = mt.make_windows(None, [0.25, 0.5], X, np.random.default_rng(1))
    assert all(np.array_equal(a, b) for a, b in zip(ws, again))
