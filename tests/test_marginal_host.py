"""Marginal likelihoods, host side: the NumPy restatement (tests/marginal_ref.py) against a dense contraction and against an
unscaled long-double product, and the argument checks of log_marginals / classify(..., missing_mask=) - no GPU."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from tests import marginal_ref as MR


MASKS = {"none": [], "all": [0, 1, 2, 3, 4], "both_ends": [0, 4], "interior": [1, 2], "label": None}


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("label_site", [4, 2], ids=["label_last", "label_middle"])
def test_restatement_against_the_dense_contraction(cx, label_site):
    T, d, C = 5, 3, 3
    rng = np.random.default_rng(5 + label_site + (10 if cx else 0))
    W = MR.gaussian_chain(T, d, 4, C, label_site, cx, rng)
    names = list(MASKS)
    phi = MR.random_states(len(names), T, d, cx, rng)
    miss = np.zeros((len(names), T), dtype=bool)
    for i, n in enumerate(names):
        miss[i, [label_site] if MASKS[n] is None else MASKS[n]] = True
    got = MR.log_marginals_ref(W, phi, miss)
    worst = 0.0
    for i in range(len(names)):
        for c in range(C):
            worst = max(worst, abs(got[i, c] - MR.dense_log_marginal(W, phi[i], miss[i], c)))
    print(f"largest |ln l (recursion) - ln l (dense)| = {worst:.3e}")
    assert worst <= 1e-12
    # NULL mask == nothing missing; masked states are never read
    assert np.array_equal(MR.log_marginals_ref(W, phi[:1], None), got[:1])
    poisoned = phi.copy()
    poisoned[miss] = np.nan
    assert np.array_equal(MR.log_marginals_ref(W, poisoned, miss), got)


def test_restatement_log_bookkeeping_against_a_long_double_product():
    """T = 1000, d = 4, chi = 8: ln l is below -800, where an unscaled fp64 product has underflowed (ln of the smallest fp64
    denormal is -744.4); np.longdouble's exponent range keeps the unscaled product in range.  Bound: every site contributes about
    d chi eps = 4e-15 to ln l in either form, 1000 sites 4e-12 at most if every error had the same sign; 1e-10 as on the device."""
    assert np.finfo(np.longdouble).minexp < -16000, "np.longdouble must have the x87 exponent range for this check"
    from oracle import ref_numpy as R
    T, d, chi, C = 1000, 4, 8, 2
    rng = np.random.default_rng(77)
    W = MR.normalised_chain(T, d, chi, C, rng)          # (R.random_mps carries its R factors along and overflows near T = 400)
    x = rng.uniform(-1, 1, (2, T))
    phi = R.legendre_encode(x, d)
    miss = np.zeros((2, T), dtype=bool)
    miss[1, rng.choice(T, 300, replace=False)] = True
    got = MR.log_marginals_ref(W, phi, miss)
    assert np.all(np.isfinite(got)) and got[0].max() < -800.0, got
    for i in range(2):
        for c in range(C):
            want = MR.naive_log_marginal(W, phi[i], miss[i], c)
            assert np.isfinite(want)
            assert abs(got[i, c] - want) <= 1e-10, (i, c, got[i, c], want)


# ---- argument checks, before an engine exists ------------------------------------------------------------------------------------
class _NoEngine:
    def __init__(self, *a, **k):
        raise AssertionError("an engine was constructed before the arguments were checked")


def _trained(T=6, N=8):
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (N, T))
    y = np.arange(N) % 2
    opts = mt.MPSOptions(d=3, chi_max=4, verbosity=-1)
    td = mt.EncodedTimeSeriesSet(np.zeros((N, T, 3)), y, y.astype(np.int32), X, np.array([N // 2, N // 2]))
    W = MR.gaussian_chain(T, 3, 4, 2, T - 1, False, rng)
    return mt.TrainedMPS(W, opts, td), X


@pytest.fixture
def no_engine(monkeypatch):
    from mpstime_jl_amd import marginal, training
    monkeypatch.setattr(marginal, "SweepEngine", _NoEngine)
    monkeypatch.setattr(training, "SweepEngine", _NoEngine)


def test_mask_shape_mismatch_raises_before_an_engine_exists(no_engine):
    trained, X = _trained()
    for bad in (np.zeros((X.shape[0], X.shape[1] + 1), dtype=bool), np.zeros((X.shape[0] - 1, X.shape[1]), dtype=bool),
                np.zeros(X.shape[1], dtype=bool)):
        with pytest.raises(ValueError, match="missing_mask has shape"):
            mt.log_marginals(trained, X, bad)
        with pytest.raises(ValueError, match="missing_mask has shape"):
            mt.classify(trained, X, missing_mask=bad)
        with pytest.raises(ValueError, match="missing_mask has shape"):
            mt.class_posteriors(trained, X, bad)
    enc = mt.EncodedTimeSeriesSet(np.zeros((4, X.shape[1], 3)), np.zeros(4), np.zeros(4, dtype=np.int32), X[:4], np.array([4]))
    with pytest.raises(ValueError, match="missing_mask has shape"):
        mt.log_marginals(trained, enc, np.zeros((5, X.shape[1]), dtype=bool))


def test_non_finite_value_at_an_unmasked_position_raises_before_an_engine_exists(no_engine):
    trained, X = _trained()
    mask = np.zeros(X.shape, dtype=bool)
    mask[0, 1] = True
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[2, 3] = bad
        with pytest.raises(ValueError, match="unmasked"):
            mt.log_marginals(trained, Xb, mask)
        with pytest.raises(ValueError, match="unmasked"):
            mt.classify(trained, Xb, missing_mask=mask)
    enc = mt.EncodedTimeSeriesSet(np.full((X.shape[0], X.shape[1], 3), np.nan), np.zeros(X.shape[0]), np.zeros(X.shape[0], dtype=np.int32), X,
                                  np.array([X.shape[0]]))
    with pytest.raises(ValueError, match="unmasked"):
        mt.log_marginals(trained, enc, mask)


def test_values_at_masked_positions_may_be_anything(monkeypatch):
    """NaN under the mask passes the checks and never reaches the encoder: the states equal those of any other filler."""
    from mpstime_jl_amd import marginal
    trained, X = _trained()
    mask = np.zeros(X.shape, dtype=bool)
    mask[0, 1] = mask[3, :] = True
    Xn = X.copy()
    Xn[mask] = np.nan
    Xz = X.copy()
    Xz[mask] = 123.0
    pa, ma = marginal.marginal_states(trained, Xn, mask)
    pb, mb = marginal.marginal_states(trained, Xz, mask)
    assert np.all(np.isfinite(pa)) and np.array_equal(pa, pb) and np.array_equal(ma, mask) and np.array_equal(mb, mask)
    # imputation's own pre-processing on the same rows gives the same scaled series
    from mpstime_jl_amd import imputation as IM
    from mpstime_jl_amd.encodings import fit_encoding_from_training_data
    td = trained.train_data
    encoder = fit_encoding_from_training_data(mt.safe_options(trained.opts), td.original_data, td.labels)[2]
    Xf = np.where(mask, 0.0, X)
    imp = IM.ImputationProblem(trained.mps, td.original_data, td.labels, Xf, np.zeros(len(X)), mt.safe_options(trained.opts), None, {}, encoder)
    scaled = IM._scaled_instances(imp, np.arange(len(X)), mask)[4]
    assert np.array_equal(pa, encoder(scaled))
