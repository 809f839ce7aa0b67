"""Entanglement analysis on the device (mpst_entanglement / mpst_see_variation through mpstime_jl_amd.analysis) against the
NumPy restatement of the reference's analysis module (tests/analysis_ref.py).

Tolerance: where the restatement's smallest RDM eigenvalue lies within 1e-13 of zero, whether rho_correct clamps it (adding
about 2.7e-7 per clamped eigenvalue) depends on the sign of rounding noise, which two correct implementations need not share;
there the comparison allows d * 3e-7 (analysis_ref.tolerance)."""
import os

import numpy as np
import pytest

import mpstime_jl_amd as mt
from tests import analysis_ref as A
from tests.test_analysis_ref import gauge, random_model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
JLD = os.path.join(HERE, "golden", "ref_test_dataset.jld2")


@pytest.fixture(scope="module")
def engine():
    eng = mt.SweepEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ecg():
    return mt.load_trained_mps(JLD)


def _model(W, X=None, opts=None):
    """A TrainedMPS around raw site tensors (training data only feeds see_variation's normalisation)."""
    T = len(W)
    X = np.random.default_rng(0).uniform(-1, 1, (8, T)) if X is None else X
    y = np.zeros(len(X), dtype=np.int64)
    td = mt.EncodedTimeSeriesSet(np.zeros((len(X), T, W[0].shape[1])), y, y.astype(np.int32), X, np.array([len(X)]))
    return mt.TrainedMPS(W, opts or mt.MPSOptions(d=W[0].shape[1], verbosity=-1), td)


def _encoded(tm, X):
    opts = mt.options.safe_options(tm.opts)
    enc = mt.model_encoding(opts.encoding)
    _, norms = mt.transform_train_data(tm.train_data.original_data, opts, enc.range)
    scaled, _ = mt.transform_test_data(X, norms, opts, enc.range)
    return enc.encode(scaled, opts.d)


def _check_spectra(tm, engine, atol=1e-10):
    d = tm.mps[0].shape[1]
    bee, see = mt.bipartite_spectrum(tm, engine=engine), mt.single_site_spectrum(tm, engine=engine)
    mins = []
    rb, rs = A.bipartite_spectrum(tm.mps), A.single_site_spectrum(tm.mps, mins)
    for c in range(len(rb)):
        np.testing.assert_allclose(bee[c], rb[c], atol=atol, rtol=0)
        assert bee[c][-1] == bee[c][-2] or len(bee[c]) == 1
        err = np.abs(see[c] - rs[c])
        assert np.all(err <= A.tolerance(mins[c], d, atol)), err.max()
    return bee, see


def _check_variation(tm, X, cls, engine, see_row0, atol=1e-9):
    d = tm.mps[0].shape[1]
    T = len(tm.mps)
    out = mt.see_variation(tm, X, cls, engine=engine)
    assert out.shape == (len(X), T, T)
    ref, mins = A.see_variation_encoded(A.expand_label_index(tm.mps)[cls], _encoded(tm, X), return_mins=True)
    err = np.abs(out - ref)
    assert np.all(err <= A.tolerance(mins, d, atol)), float(np.nanmax(err))
    assert np.array_equal(out[:, 0, :], np.broadcast_to(see_row0, (len(X), T)))       # row 0 is single_site_spectrum, bit for bit
    lo = np.tril_indices(T, -1)
    assert np.all(out[:, lo[0], lo[1]] == 0.0)
    return out


def test_reference_ecg200_model(ecg, engine):
    """The reference's own trained ECG200 model (T=96, d=5, chi=25, C=2): BEE / SEE of both classes to 1e-10, see_variation
    on 16 of its series for both classes to 1e-9."""
    _, see = _check_spectra(ecg, engine)
    X = ecg.train_data.original_data[::6][:16]
    for cls in range(2):
        _check_variation(ecg, X, cls, engine, see[cls])


def test_fitted_model_headline_shape(engine):
    """A fitMPS-trained model at (T=100, chi=32, d=4)."""
    rng = np.random.default_rng(7)
    X1, _ = mt.trendy_sine(100, 24, period=(12.0, 15.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(100, 24, period=(16.0, 19.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.repeat([0, 1], 24)
    tm, _, _ = mt.fitMPS(X, y, opts=mt.MPSOptions(d=4, chi_max=32, nsweeps=1, eta=0.05, verbosity=-1))
    assert max(t.shape[2] for t in tm.mps) == 32
    _, see = _check_spectra(tm, engine)
    _check_variation(tm, X[[0, 30, 47]], 1, engine, see[1])


@pytest.mark.parametrize("T,d,chi,C,label", [(8, 8, 128, 2, 7), (2, 4, 4, 3, 1), (9, 3, 20, 2, 4)])
def test_shapes(T, d, chi, C, label, engine):
    """chi = 128 with d = 8, T = 2, and the label site mid-chain."""
    W = random_model(T, d, chi, C, label, seed=T + d)
    tm = _model(W)
    _, see = _check_spectra(tm, engine)
    X = np.random.default_rng(3).uniform(-1, 1, (2, T))
    _check_variation(tm, X, C - 1, engine, see[C - 1])


def test_gauge_perturbed_model_gives_the_same_output(engine):
    """G, G^-1 with cond(G) ~ 1e4 on every bond: the canonicalisation must not care (1e-9)."""
    W = random_model(12, 3, 27, 2, 6, seed=11)
    Wg = gauge(W, 1e4, seed=12)
    tm, tg = _model(W), _model(Wg)
    X = np.random.default_rng(4).uniform(-1, 1, (3, 12))
    for f in (mt.bipartite_spectrum, mt.single_site_spectrum):
        for a, b in zip(f(tm, engine=engine), f(tg, engine=engine)):
            np.testing.assert_allclose(a, b, atol=1e-9, rtol=0)
    _, mins = A.see_variation_encoded(A.expand_label_index(W)[0], _encoded(tm, X), return_mins=True)
    err = np.abs(mt.see_variation(tm, X, 0, engine=engine) - mt.see_variation(tg, X, 0, engine=engine))
    assert np.all(err <= A.tolerance(mins, 3, 1e-9))


def test_batch_not_a_multiple_of_the_tile_and_repeatable(ecg, engine):
    """37 series (no multiple of anything the kernels deal out); two calls give the same bits; log bases."""
    X = ecg.train_data.original_data[:37]
    a = mt.see_variation(ecg, X, 1, engine=engine)
    b = mt.see_variation(ecg, X, 1, engine=engine)
    assert np.array_equal(a, b)
    one = mt.see_variation(ecg, X[36:37], 1, engine=engine)
    np.testing.assert_allclose(one[0], a[36], atol=1e-12, rtol=0)
    e, e2, e10 = (mt.bipartite_spectrum(ecg, logfn=f, engine=engine) for f in ("log", np.log2, "log10"))
    np.testing.assert_allclose(e2[0], e[0] / np.log(2), rtol=1e-14)
    np.testing.assert_allclose(e10[1], e[1] / np.log(10), rtol=1e-14)


def test_complex_model_is_refused(engine):
    W = [t.astype(np.complex128) for t in random_model(4, 2, 4, 2, seed=1)]
    with pytest.raises(ValueError, match="complex"):
        mt.single_site_spectrum(_model(W), engine=engine)
    # and the ABI refuses it too
    import ctypes as C
    from mpstime_jl_amd import analysis
    m = analysis._Model(_model(random_model(4, 2, 4, 2, seed=1)))
    m.struct.dtype = 1
    rc = engine.lib.mpst_entanglement(engine.ctx, C.byref(m.struct), None, None)
    assert rc == mt._lib.MPST_ERR_UNSUPPORTED
