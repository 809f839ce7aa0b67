"""The NumPy restatement of the reference's analysis module (tests/analysis_ref.py) against brute force on tiny models, its
gauge invariance and the reference's quirks; and the argument checks of the package's analysis API, which run before the
device is touched."""
import os
import types

import numpy as np
import pytest

import mpstime_jl_amd as mt
from tests import analysis_ref as A


def random_model(T, d, chi, C, label=None, seed=0):
    rng = np.random.default_rng(seed)
    label = T - 1 if label is None else label
    dims = [1] + [min(chi, d ** min(j, T - j)) for j in range(1, T)] + [1]
    W = []
    for j in range(T):
        shape = (dims[j], d, dims[j + 1]) + ((C,) if j == label else ())
        W.append(rng.standard_normal(shape))
    return W


def full_state(W, c):
    """psi of class c, normalised: (d,) * T."""
    ls = A.label_site(W)
    psi = np.ones((1, 1))
    for j, a in enumerate(W):
        a = a[..., c] if j == ls else a
        psi = np.einsum("xl,lsr->xsr", psi, a).reshape(-1, a.shape[2])
    psi = psi[:, 0]
    return psi / np.linalg.norm(psi)


def vn(p, logfn=np.log):
    return float(sum(-x * logfn(x) for x in p if x > 1e-12))


def brute_bee(psi, T, d):
    out = np.zeros(T)
    for i in range(T - 1):
        s = np.linalg.svd(psi.reshape(d ** (i + 1), -1), compute_uv=False)
        out[i] = vn(s * s)
    out[T - 1] = out[T - 2] if T > 1 else 0.0
    return out


def brute_see(psi, T, d):
    out = np.zeros(T)
    for i in range(T):
        m = psi.reshape(d ** i, d, -1)
        rho = np.einsum("asb,atb->st", m, m)
        out[i] = A.entropy_of(A.rho_correct(rho))
    return out


def brute_variation(psi, phi, T, d):
    out = np.zeros((T, T))
    out[0] = brute_see(psi, T, d)
    for k in range(1, T):
        m = psi.reshape((d,) * T)
        for i in range(k):
            m = np.tensordot(phi[i], m, axes=(0, 0))
        m = m.reshape(-1)
        m = m / np.linalg.norm(m)
        out[k, k:] = brute_see(m, T - k, d)
    return out


def gauge(W, cond, seed):
    """G_j, G_j^-1 on every bond, cond(G_j) ~ cond."""
    rng = np.random.default_rng(seed)
    W = [a.copy() for a in W]
    for j in range(len(W) - 1):
        n = W[j].shape[2]
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        G = U @ np.diag(np.logspace(0, np.log10(cond), n)) @ V.T
        W[j] = np.einsum("lsr...,rq->lsq...", W[j], G)
        W[j + 1] = np.einsum("pr,rsq...->psq...", np.linalg.inv(G), W[j + 1])
    return W


SHAPES = [(2, 2, 2, 2, 1), (5, 2, 4, 2, 4), (6, 3, 9, 2, 2), (8, 2, 16, 3, 0), (4, 3, 9, 1, 3)]


@pytest.mark.parametrize("T,d,chi,C,label", SHAPES)
def test_restatement_agrees_with_brute_force(T, d, chi, C, label):
    W = random_model(T, d, chi, C, label, seed=T * 10 + d)
    mins = []
    bee, see = A.bipartite_spectrum(W), A.single_site_spectrum(W, mins)
    rng = np.random.default_rng(1)
    phi = rng.standard_normal((2, T, d))
    for c in range(C):
        psi = full_state(W, c)
        np.testing.assert_allclose(bee[c], brute_bee(psi, T, d), atol=1e-12, rtol=0)
        assert np.all(np.abs(see[c] - brute_see(psi, T, d)) <= A.tolerance(mins[c], d, 1e-12))
        var, vm = A.see_variation_encoded(A.expand_label_index(W)[c], phi, return_mins=True)
        for i in range(2):
            assert np.all(np.abs(var[i] - brute_variation(psi, phi[i], T, d)) <= A.tolerance(vm[i], d, 1e-12))
        assert np.array_equal(var[0, 0], see[c])
        assert np.all(var[:, np.tril_indices(T, -1)[0], np.tril_indices(T, -1)[1]] == 0.0)


def test_restatement_is_gauge_invariant():
    T, d, chi, C = 7, 3, 8, 2
    W = random_model(T, d, chi, C, 3, seed=5)
    Wg = gauge(W, 1e4, seed=6)
    phi = np.random.default_rng(2).standard_normal((2, T, d))
    # the gauged model itself differs from the original by about cond * eps per bond (G^-1 is rounded)
    for a, b in zip(A.bipartite_spectrum(W), A.bipartite_spectrum(Wg)):
        np.testing.assert_allclose(a, b, atol=1e-9, rtol=0)
    mins = []
    for a, b, m in zip(A.single_site_spectrum(W, mins), A.single_site_spectrum(Wg), mins):
        assert np.all(np.abs(a - b) <= A.tolerance(m, d, 1e-9))
    for c in range(C):
        v, vm = A.see_variation_encoded(A.expand_label_index(W)[c], phi, return_mins=True)
        assert np.all(np.abs(v - A.see_variation_encoded(A.expand_label_index(Wg)[c], phi)) <= A.tolerance(vm, d, 1e-9))


def test_last_entry_repeats_the_last_bond_and_logfn_bases():
    W = random_model(6, 2, 4, 2, seed=9)
    for b in A.bipartite_spectrum(W):
        assert b[-1] == pytest.approx(b[-2], abs=1e-13)          # the same bond, cut by a second SVD
    for a, b in zip(A.bipartite_spectrum(W, np.log), A.bipartite_spectrum(W, np.log2)):
        np.testing.assert_allclose(a / np.log(2), b, rtol=1e-13)
    with pytest.raises(ValueError):
        A.bipartite_spectrum(W, np.exp)


def test_schmidt_weights_below_1e_12_are_cut():
    p = np.array([1 - 1e-13, 1e-13])
    W = [np.diag(np.sqrt(p)).reshape(1, 2, 2), np.eye(2).reshape(2, 2, 1, 1)]
    bee = A.bipartite_spectrum(W)[0]
    assert bee[0] == pytest.approx(1e-13, rel=1e-2) and bee[1] == pytest.approx(bee[0], rel=1e-2)
    assert -p[1] * np.log(p[1]) > 2e-12                          # the weight below the cut would have added this


def test_rho_correct_branches():
    rho = np.diag([0.6, 0.4])
    assert A.rho_correct(rho) is rho                                    # no negative eigenvalue: untouched
    clamped = A.rho_correct(np.diag([1.0, -1e-10]))                     # within sqrt(eps): clamped to sqrt(eps)
    np.testing.assert_allclose(np.linalg.eigvalsh(clamped), [A.EIGTOL, 1.0], rtol=1e-12)
    with pytest.raises(A.DomainError):
        A.rho_correct(np.diag([1.0, -1e-6]))                            # outside the tolerance
    with pytest.raises(A.DomainError):
        A.rho_correct(np.diag([1.05, -1e-10]))                          # trace off by more than 0.01 after clamping
    assert A.entropy_of(np.diag([1.0, 0.0])) == 0.0                     # an exact zero contributes 0 (the reference: NaN)


def _fake(W):
    return types.SimpleNamespace(mps=W, opts=mt.MPSOptions(verbosity=-1), train_data=None)


def test_api_argument_checks_need_no_device():
    W = random_model(5, 2, 4, 2, seed=1)
    with pytest.raises(ValueError, match="logfn"):
        mt.bipartite_spectrum(_fake(W), logfn="ln")
    with pytest.raises(ValueError, match="logfn"):
        mt.bipartite_spectrum(_fake(W), logfn=np.exp)
    Wc = [a.astype(np.complex128) for a in W]
    for call in (lambda: mt.bipartite_spectrum(_fake(Wc)), lambda: mt.single_site_spectrum(_fake(Wc)),
                 lambda: mt.see_variation(_fake(Wc), np.zeros((1, 5)))):
        with pytest.raises(ValueError, match="complex"):
            call()
    with pytest.raises(ValueError, match="class"):
        mt.see_variation(_fake(W), np.zeros((1, 5)), cls=2)
    with pytest.raises(ValueError, match="class"):
        mt.see_variation(_fake(W), np.zeros((1, 5)), cls=-1)
    with pytest.raises(ValueError, match="measure_series"):
        mt.see_variation(_fake(W), np.zeros((2, 6)))
    assert issubclass(mt.DomainError, mt.MPSTError) and issubclass(mt.DomainError, ValueError)


GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_ecg200_analysis.npz")


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="tests/golden/make_analysis_goldens.jl has not been run (needs Julia)")
def test_restatement_against_reference_outputs():
    """The reference's own bipartite_spectrum / single_site_spectrum / see_variation of its trained ECG200 model."""
    g = np.load(GOLDEN)
    tm = mt.load_trained_mps(os.path.join(os.path.dirname(__file__), "golden", "ref_test_dataset.jld2"))
    d = tm.mps[0].shape[1]
    mins = []
    bee, see = A.bipartite_spectrum(tm.mps), A.single_site_spectrum(tm.mps, mins)
    X = tm.train_data.original_data[g["rows"]]
    opts = mt.options.safe_options(tm.opts)
    enc = mt.model_encoding(opts.encoding)
    _, norms = mt.transform_train_data(tm.train_data.original_data, opts, enc.range)
    phi = enc.encode(mt.transform_test_data(X, norms, opts, enc.range)[0], opts.d)
    for c in range(len(bee)):
        np.testing.assert_allclose(bee[c], g[f"bee_{c}"], atol=1e-10, rtol=0)
        assert np.all(np.abs(see[c] - g[f"see_{c}"]) <= A.tolerance(mins[c], d, 1e-10))
        var, vm = A.see_variation_encoded(A.expand_label_index(tm.mps)[c], phi, return_mins=True)
        assert np.all(np.abs(var - g[f"var_{c}"]) <= A.tolerance(vm, d, 1e-9))
