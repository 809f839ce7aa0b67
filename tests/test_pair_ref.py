"""The two host forms of the pair analysis against each other (tests/pair_ref.py): the recursion the device runs (``transfer``)
against the dense state (``brute_force``), the closed-form answers of a GHZ chain and a product state, and ``position_operator``
against the Jacobi matrix of the Legendre recurrence.  No GPU.

The two forms agreed to 2.1e-14 at worst on the five models below when they were first tried; the bound here is 1e-12."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from tests import pair_ref as P

LN2 = float(np.log(2.0))

# (chi, d, label site)
MODELS = [((1, 2, 4, 4, 3, 2, 1), 2, None), ((1, 3, 7, 7, 5, 3, 1), 3, 2), ((1, 5, 3, 1), 2, 0), ((1, 4, 9, 9, 9, 4, 2, 1), 2, 3),
          ((1, 1, 1, 1), 3, None)]


def sym_obs(d, seed, T=None):
    rng = np.random.default_rng(seed)
    O = rng.standard_normal((d, d) if T is None else (T, d, d))
    return 0.5 * (O + np.swapaxes(O, -1, -2))


def trained(W, X=None, opts=None):
    """A TrainedMPS around raw site tensors (the training data only feeds the encoder's fit)."""
    T = len(W)
    X = np.random.default_rng(0).uniform(-1, 1, (8, T)) if X is None else X
    y = np.zeros(len(X), dtype=np.int64)
    td = mt.EncodedTimeSeriesSet(np.zeros((len(X), T, W[0].shape[1])), y, y.astype(np.int32), X, np.array([len(X)]))
    return mt.TrainedMPS(W, opts or mt.MPSOptions(d=W[0].shape[1], verbosity=-1), td)


@pytest.mark.parametrize("chi,d,label", MODELS)
def test_transfer_equals_brute_force(chi, d, label):
    W = P.chain_model(chi, d, 2, label, seed=len(chi) + d)
    O = sym_obs(d, 5, T=len(chi) - 1)
    a, b = P.brute_force(W, O), P.transfer(W, O)
    worst = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
    print(f"transfer vs brute_force, chi={chi} d={d}: {worst:.2e}")
    assert worst <= 1e-12
    mi = a[0]
    assert np.array_equal(mi, mi.transpose(0, 2, 1)) and np.array_equal(a[2], a[2].transpose(0, 2, 1))


@pytest.mark.parametrize("form", [P.brute_force, P.transfer])
def test_ghz_chain(form):
    """T = 5, d = 2, O = diag(1, -1): every I(i:j) is ln 2, every S_i is ln 2 (0.6931471805599454), every covariance 1, mean 0."""
    mi, mean, cov = form(P.ghz_model(5), np.diag([1.0, -1.0]))
    np.testing.assert_allclose(mi, LN2, atol=1e-12, rtol=0)
    np.testing.assert_allclose(cov, 1.0, atol=1e-12, rtol=0)
    np.testing.assert_allclose(mean, 0.0, atol=1e-12, rtol=0)


@pytest.mark.parametrize("form", [P.brute_force, P.transfer])
def test_product_state(form):
    """All bonds 1: |I| <= 1e-12 (4e-15 seen) and |cov| <= 1e-12 off the diagonal."""
    W = P.chain_model((1, 1, 1, 1), 3, 2, seed=9)
    mi, mean, cov = form(W, sym_obs(3, 2))
    off = ~np.eye(3, dtype=bool)
    print("product state: max |I|", np.abs(mi[:, off]).max(), "max |cov|", np.abs(cov[:, off]).max())
    assert np.abs(mi[:, off]).max() <= 1e-12 and np.abs(cov[:, off]).max() <= 1e-12
    assert np.abs(np.diagonal(mi, axis1=1, axis2=2)).max() <= 1e-12          # a product state's sites are pure


def test_no_observable_gives_no_moments():
    mi, mean, cov = P.transfer(P.chain_model((1, 2, 2, 1), 2, 2))
    assert mean is None and cov is None and mi.shape == (2, 3, 3)


def test_position_operator_is_the_legendre_jacobi_matrix():
    """The default encoding is the orthonormal Legendre basis sqrt((2k+1)/2) P_k on [-1, 1], whose position operator is the Jacobi
    matrix of the three-term recurrence: zero diagonal, X[k, k+1] = (k+1) / sqrt((2k+1)(2k+3)).  The bound is the grid's own
    quadrature error, measured here: the composite trapezoid's error falls as h^2, so the result on 2001 points differs from the
    exact integral by a third of its distance to the result on 1001 points; that whole distance is the bound.  For d = 6 the bound
    was 6.5e-5 and the error 2.2e-5 when this was written."""
    d, T = 6, 4
    W = trained(P.chain_model((1, 2, 2, 2, 1), d, 2))
    X = mt.position_operator(W)
    assert X.shape == (T, d, d)
    J = np.zeros((d, d))
    for k in range(d - 1):
        J[k, k + 1] = J[k + 1, k] = (k + 1) / np.sqrt((2 * k + 1) * (2 * k + 3))
    bound = float(np.abs(mt.position_operator(W, npoints=1001) - X).max())
    err = float(np.abs(X - J).max())
    print(f"position_operator: quadrature bound {bound:.3e}, error {err:.3e}")
    assert 0.0 < bound < 1e-4
    assert err <= bound
    assert np.array_equal(X, X.transpose(0, 2, 1))
    for t in range(1, T):
        assert np.array_equal(X[t], X[0])


def test_position_operator_refuses_a_complex_encoding():
    W = trained(P.chain_model((1, 2, 2, 1), 4, 2), opts=mt.MPSOptions(d=4, encoding="Fourier", verbosity=-1))
    with pytest.raises(ValueError, match="complex encoding"):
        mt.position_operator(W)
