"""Hyperparameter tuning on batched device fits: ragged batches (mpst_sweep_batch with unequal class counts), batched one-launch
scoring (mpst_classify_batch), fit_batch / eval_loss / tune / evaluate (mpstime.jl_amd/tuning.py; the reference's
src/Training/hyperparameters/)."""
import os

import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(__file__), "golden", "ref_ecg200_trained_mps.npz")


def _ntiles(ds):
    return int(sum((int(c) + 15) // 16 for c in ds.class_distribution))


def _ragged_problems(K):
    """K seeded problems with ragged labels whose sizes differ by one or two; the last one is a tile block shorter."""
    sizes = [250 + (k * 7) % 3 for k in range(K)]
    sizes[-1] = 232
    probs = [make_problem(sizes[k], 12, 4, 4, 2, seed=70 + k, balanced=False) for k in range(K)]
    counts = [tuple(int(c) for c in p[0].class_distribution) for p in probs]
    assert len(set(counts)) > 1 and len({_ntiles(p[0]) for p in probs}) > 1       # a property of the inputs
    return probs


def _fresh(prob, K, eta, cutoff, chi=12, test=None):
    e = mt.SweepEngine(0)
    e.set_batch_hint(K)
    e.set_options(chi_max=chi, eta=eta, cutoff=cutoff)
    ds, W = prob
    e.set_dataset(0, ds.phi, ds.label_index, 2)
    if test is not None:
        e.set_dataset(1, test.phi, test.label_index, 2)
    e.set_mps(W)
    e.build_caches()
    return e


def _same_state(a, b):
    for ta, tb in zip(a.get_mps(), b.get_mps()):
        assert np.array_equal(ta, tb)
    assert a.eval(0)[:3] == b.eval(0)[:3]


def _check_scores(res, engines, tests):
    """classify_batch against classify / eval of every engine and against the oracle's contraction"""
    for r, e, te in zip(res, engines, tests):
        pred, yh = e.classify(1, return_overlaps=True)
        assert np.array_equal(r["pred"], pred)
        yo = R.contract_mps(e.get_mps(), te.phi)
        err = np.max(np.abs(r["yhat"] - yo)) / np.abs(yo).max()
        print(f"classify_batch: N = {len(pred)}, overlap error {err:.3e} of the largest overlap")
        assert err < 1e-11
        mse, kld, acc, conf = e.eval(1)
        print(f"  mse {r['mse']!r} / {mse!r}, kld {r['kld']!r} / {kld!r}, acc {r['acc']!r} / {acc!r}")
        assert abs(r["mse"] - mse) <= 1e-10 * abs(mse)
        assert abs(r["kld"] - kld) <= 1e-10 * abs(kld)
        assert abs(r["acc"] - acc) <= 1e-10 * abs(acc) or r["acc"] == acc
        assert np.array_equal(r["conf"], conf)


@pytest.mark.parametrize("K", [5, 12])
def test_ragged_batch_is_bit_identical_and_scored_in_one_launch(K):
    """Fits that differ in their series and class counts advance in one launch chain with the bits of separate sweeps; the batch is
    then scored on validation sets of unequal size by classify_batch, and a sweep after the scoring continues as one without."""
    probs = _ragged_problems(K)
    tests = [make_problem(37 + 5 * k, 12, 4, 4, 2, seed=170 + k, balanced=False)[0] for k in range(K)]
    etas = [[0.05, 0.02, 0.05, 0.1][k % 4] for k in range(K)]
    cuts = [1e-2 if k % 3 == 1 else 1e-10 for k in range(K)]       # a coarse cutoff: those fits keep smaller bonds
    solo = [_fresh(probs[k], K, etas[k], cuts[k], test=tests[k]) for k in range(K)]
    bat = [_fresh(probs[k], K, etas[k], cuts[k], test=tests[k]) for k in range(K)]
    try:
        for sweep in range(3):
            for e in solo:
                e.sweep()
            st = mt.sweep_batch(bat)
            assert len(st) == K and all(s["eig_fallbacks"] == 0 for s in st)
            for a, b in zip(solo, bat):
                _same_state(a, b)
        profiles = {tuple(e.get_chi()[0].tolist()) for e in bat}
        print("bond dimension profiles:", len(profiles))
        assert len(profiles) > 1
        res = mt.classify_batch(bat, 1, return_overlaps=True)
        _check_scores(res, solo, tests)
        # the scored batch goes on exactly like the fits that were not scored
        for e in solo:
            e.sweep()
        mt.sweep_batch(bat)
        for a, b in zip(solo, bat):
            _same_state(a, b)
        other = _fresh(probs[0], K, 0.05, 1e-10, chi=8)
        try:
            with pytest.raises(mt.MPSTError, match="differs in shape"):
                mt.sweep_batch([bat[0], other])
        finally:
            other.close()
    finally:
        for e in solo + bat:
            e.close()


def test_ragged_batch_multi_is_bit_identical():
    K = 6
    probs = _ragged_problems(K)
    solo = [_fresh(probs[k], K, 0.05, 1e-10) for k in range(K)]
    bat = [_fresh(probs[k], K, 0.05, 1e-10) for k in range(K)]
    try:
        for sweep in range(3):
            for e in solo:
                e.sweep()
            mt.sweep_batch_multi(bat, groups=[0, 1, 0, 1, 0, 1])
            for a, b in zip(solo, bat):
                _same_state(a, b)
    finally:
        for e in solo + bat:
            e.close()


def test_classify_batch_on_the_reference_mps():
    """K = 3 copies of the reference's own trained MPS (d = 5, chi = 25) on row subsets of its data"""
    z = np.load(FIX)
    T = z["pstates"].shape[1]
    W = [z[f"W_{j}"] for j in range(T)]
    cd = z["class_distribution"]
    lab = np.repeat(np.arange(len(cd)), cd)
    subsets = [np.arange(len(lab)), np.arange(0, len(lab), 2), np.arange(3, len(lab) - 10)]
    engines = []
    try:
        for rows in subsets:
            e = mt.SweepEngine(0)
            e.set_options(chi_max=int(z["chi_max"]))
            e.set_dataset(0, z["pstates"][:1], lab[:1], len(cd))
            e.set_dataset(1, z["pstates"][rows], lab[rows], len(cd))
            e.set_mps(W)
            engines.append(e)
        res = mt.classify_batch(engines, 1, return_overlaps=True)
        sets = [R.EncodedSet(z["pstates"][rows], lab[rows], np.bincount(lab[rows])) for rows in subsets]
        _check_scores(res, engines, sets)
        assert np.array_equal(res[0]["pred"], lab) and res[0]["acc"] == 1.0
    finally:
        for e in engines:
            e.close()


# ---- host layer: fit_batch, tune, eval_loss, evaluate ---------------------------------------------------------------------------
from mpstime_jl_amd import tuning as tu      # noqa: E402


def _sine_data(n0=61, n1=59, T=24, seed=11, easy=False):
    """two classes of trendy sines (different periods and slopes), sizes that are no multiples of 3; ``easy``: slopes apart and
    little noise - such data is fitted exactly within two sweeps (checked on the CPU oracle)"""
    rng = np.random.default_rng(seed)
    s0, s1, sg = ((-3.0, -1.0), (1.0, 3.0), 0.05) if easy else ((-2.0, 0.0), (0.0, 2.0), 0.1)
    X0, _ = mt.trendy_sine(T, n0, period=(8.0, 12.0), slope=s0, sigma=sg, rng=rng)
    X1, _ = mt.trendy_sine(T, n1, period=(16.0, 24.0), slope=s1, sigma=sg, rng=rng)
    X = np.vstack([X0, X1])
    y = np.r_[np.zeros(n0, dtype=np.int64), np.ones(n1, dtype=np.int64)]
    perm = rng.permutation(len(y))
    return X[perm], y[perm]


def _opts(**kw):
    base = dict(verbosity=-5, log_level=-1, d=4, chi_max=10, nsweeps=2, eta=0.05, sigmoid_transform=True)
    base.update(kw)
    return mt.MPSOptions(**base)


def test_fit_batch_equals_fitMPS():
    """Six jobs: two shapes, ragged counts, one that reaches exit_early, one with fewer sweeps"""
    X, y = _sine_data(easy=True)
    folds = mt.make_stratified_cvfolds(X, y, 3, rng=2)
    jobs = [(X[folds[0][0]], y[folds[0][0]], _opts()),
            (X[folds[1][0]], y[folds[1][0]], _opts(eta=0.02)),
            (X[folds[2][0]], y[folds[2][0]], _opts(nsweeps=1)),
            (X[folds[0][0]], y[folds[0][0]], _opts(chi_max=8)),
            (X[folds[1][0]], y[folds[1][0]], _opts(chi_max=8, nsweeps=6, exit_early=True, log_level=3)),
            (X[:100], y[:100], _opts(chi_max=8, eta=0.1))]
    assert len({len(j[0]) for j in jobs}) > 1
    res = mt.fit_batch(jobs)
    assert all(r.batched and r.error is None for r in res)
    for (Xt, yt, o), r in zip(jobs, res):
        m, info, _ = mt.fitMPS(Xt, yt, opts=o, batch_hint=tu.BATCH_HINT)
        assert len(m.mps) == len(r.mps.mps)
        for a, b in zip(m.mps, r.mps.mps):
            assert np.array_equal(a, b)
        assert info["train_acc"] == r.info["train_acc"] and info["train_KL_div"][:-1] == r.info["train_KL_div"][:-1]
    ee = res[4].info["train_acc"]
    print("exit_early job: accuracies", ee)
    assert ee[-2] == 1.0 and len(ee) < 6 + 2                               # it stopped before its sixth sweep


def _plain_loop(X, y, folds, opts_list, objective):
    """the parent's capability: one fitMPS and one eval_loss at a time"""
    out = []
    for o in opts_list:
        ls = []
        for tr, va in folds:
            m, _, _ = mt.fitMPS(X[tr], y[tr], opts=o, batch_hint=tu.BATCH_HINT)
            ls.append(float(np.mean(mt.eval_loss(objective, m, X[va], y[va]))))
        out.append(float(np.mean(ls)))
    return out


def test_tune_equals_a_plain_loop():
    X, y = _sine_data()
    folds = mt.make_stratified_cvfolds(X, y, 3, rng=4)
    assert len({len(tr) for tr, _ in folds}) > 1 or len({tuple(np.bincount(y[tr])) for tr, _ in folds}) > 1      # ragged folds
    obj = mt.MisclassificationRate()
    opts0 = _opts()
    # the chosen data trains without a decomposition failure on the CPU oracle as well: "no fallback" is a property of the inputs
    enc = mt.model_encoding(opts0.encoding)
    tr0 = folds[0][0]
    Xs_, _, _, _ = mt.transform_data(X[tr0], np.zeros((0, X.shape[1])), opts0, enc.range)
    ds0 = mt.encode_dataset(X[tr0], Xs_, y[tr0], enc, opts0.d, {0: 0, 1: 1})
    Wo = [t.copy() for t in mt.generate_startingMPS(opts0.chi_init, X.shape[1], opts0.d, 2, opts0.init_rng)]
    R.sweep(Wo, R.EncodedSet(ds0.phi, ds0.label_index, ds0.class_distribution), R.SweepOptions(nsweeps=2, chi_max=10, eta=0.05))
    assert all(np.all(np.isfinite(t)) for t in Wo)

    best, cache, info = mt.tune(X, y, 3, {"chi_max": (8, 10)}, mt.MPSRandomSearch("Exhaustive"), objective=obj, opts0=opts0,
                                foldmethod=folds, verbosity=0, return_info=True)
    assert info["fits"] == 9 and info["batched_fits"] == 9 and info["fallback_fits"] == 0 and info["failed_fits"] == 0
    assert info["batched_scores"] == 9
    keys = [(10,), (9,), (8,)]                                             # the reference's trial order: slow candidates first
    assert list(cache) == keys
    want = _plain_loop(X, y, folds, [opts0.set(chi_max=k[0]) for k in keys], obj)
    for k, w in zip(keys, want):
        print(f"tune: chi_max = {k[0]}: loss {cache[k]!r}, plain loop {w!r}")
        assert abs(cache[k] - w) <= 1e-12
    assert best == {"chi_max": keys[int(np.argmin(want))][0]}              # argmin: the first minimum, as the strict '<' scan

    best2, cache2, info2 = mt.tune(X, y, 3, {"eta": (1e-3, 1e-1)}, mt.MPSRandomSearch("LatinHypercube"), objective=mt.BalancedMisclassificationRate(),
                                   opts0=opts0, foldmethod=folds, logspace_eta=True, maxiters=4, rng=7, verbosity=0, return_info=True)
    assert len(cache2) == 4 and info2["fallback_fits"] == 0 and info2["batched_fits"] == 12
    keys2 = list(cache2)                                                   # the grid, read back from the cache
    want2 = _plain_loop(X, y, folds, [opts0.set(eta=k[0]) for k in keys2], mt.BalancedMisclassificationRate())
    for k, w in zip(keys2, want2):
        print(f"tune: eta = {k[0]!r}: loss {cache2[k]!r}, plain loop {w!r}")
        assert abs(cache2[k] - w) <= 1e-12
    assert best2 == {"eta": keys2[int(np.argmin(want2))][0]}


def test_eval_loss_imputation_equals_instance_loop():
    X, y = _sine_data(n0=40, n1=37)
    m, _, _ = mt.fitMPS(X[:60], y[:60], opts=_opts(sigmoid_transform=False, nsweeps=2))
    Xv, yv = X[60:], y[60:]
    windows = [np.arange(4, 10), np.arange(15, 22)]
    got = mt.eval_loss(mt.ImputationLoss(), m, Xv, yv, windows)
    imp = mt.init_imputation_problem(m, Xv, yv, verbosity=-5)
    want = []
    for w in windows:
        maes = []
        for cls in np.unique(yv):
            for inst in range(int(np.sum(yv == cls))):
                maes.append(mt.MPS_impute(imp, cls, inst, w, "median", NN_baseline=False)[3][0]["MAE"])
        want.append(float(np.mean(maes)))
    print("ImputationLoss:", got, "instance loop:", want)
    assert len(got) == 2 and all(abs(g - w) <= 1e-12 for g, w in zip(got, want))


def test_evaluate_smoke(tmp_path):
    X, y = _sine_data(n0=31, n1=29)
    kw = dict(objective=mt.MisclassificationRate(), opts0=_opts(nsweeps=1), n_cvfolds=2, tuning_maxiters=2, verbosity=-1, rng=3,
              write=True, writedir=str(tmp_path), simname="smoke")
    res = mt.evaluate(X, y, 2, {"chi_max": [6, 8]}, mt.MPSRandomSearch("Exhaustive"), **kw)
    assert len(res) == 2
    want = {"fold", "objective", "train_inds", "test_inds", "optimiser", "tuning_windows", "tuning_pms", "eval_windows", "eval_pms", "time",
            "opts", "cache", "loss"}
    for r in res:
        assert set(r) == want and len(r["loss"]) == 1 and 0.0 <= r["loss"][0] <= 1.0 and len(r["cache"]) == 2
        assert np.array_equal(np.sort(np.r_[r["train_inds"], r["test_inds"]]), np.arange(len(y)))
        assert r["opts"].chi_max in (6, 8)
    assert np.array_equal(np.sort(np.r_[res[0]["test_inds"], res[1]["test_inds"]]), np.arange(len(y)))
    # a second call resumes from the stored folds: nothing is fitted
    calls = []
    real = tu.fit_batch
    tu.fit_batch = lambda jobs, device=0: (calls.append(len(jobs)), real(jobs, device))[1]
    try:
        again = mt.evaluate(X, y, 2, {"chi_max": [6, 8]}, mt.MPSRandomSearch("Exhaustive"), **kw)
    finally:
        tu.fit_batch = real
    assert sum(calls) == 0
    for a, b in zip(res, again):
        assert a["loss"] == b["loss"] and a["cache"] == b["cache"] and a["opts"] == b["opts"]
    m = mt.load_trained_mps(str(tmp_path / "smoke_tmp" / "f0.npz"))
    assert m.opts == res[0]["opts"]
