"""The NumPy restatement of the marginal site conditionals (tests/margcond_ref.py) pinned to independent forms, without a GPU: the
dense d^T amplitude tensor, the marginal likelihoods of tests/marginal_ref.py, the leave-one-out conditionals of
tests/site_cond_ref.py, and its own unscaled form."""
import numpy as np
import pytest

from tests import margcond_ref as M
from tests import site_cond_ref as S
from tests.marginal_ref import class_slice, log_marginals_ref

CASES = [(5, 3, 4, 2, 6, None), (7, 2, 5, 2, 6, 3), (1, 3, 1, 2, 3, None), (4, 4, 6, 3, 7, 0)]     # (T, d, chi, C, N, label site)


def _case(case, cx):
    T, d, chi, C, N, ls = case
    return M.make_case(T, d, chi, C, N, seed=100 + T + (50 if cx else 0), cx=cx, label_site=ls, ngrid=41)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-d%d-chi%d" % c[:3])
def test_rho_matches_the_dense_amplitude_tensor(case, cx):
    W, phi, lab, miss, x_in, xs, gp, _ = _case(case, cx)
    for i in range(len(lab)):
        cm = class_slice(W, int(lab[i]))
        L, R = M.density_walks(cm, phi[i], miss[i], scaled=False)
        for t in range(len(cm)):
            r = M.rho_site(L[t], cm[t], R[t])
            ref = M.dense_rho(cm, phi[i], miss[i], t)
            assert np.abs(r - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), (i, t)
            assert np.abs(r - np.conj(r.T)).max() <= 1e-13 * np.abs(r).max()


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-d%d-chi%d" % c[:3])
def test_trace_of_rho_is_the_marginal_likelihood_without_the_site(case, cx):
    """ln tr rho_t - ln l(K_i) = ln l(K_i \\ {t}) - ln l(K_i)"""
    W, phi, lab, miss, x_in, xs, gp, _ = _case(case, cx)
    N, T = miss.shape
    safe = np.where(np.isnan(phi), 0.0, phi)
    lK = log_marginals_ref(W, safe, miss)
    for t in range(T):
        mt = miss.copy()
        mt[:, t] = True
        lKt = log_marginals_ref(W, safe, mt)
        for i in range(N):
            cm = class_slice(W, int(lab[i]))
            L, R = M.density_walks(cm, phi[i], miss[i], scaled=False)
            tr = np.trace(M.rho_site(L[t], cm[t], R[t])).real
            c = int(lab[i])
            assert abs((np.log(tr) - lK[i, c]) - (lKt[i, c] - lK[i, c])) <= 1e-12 * max(1.0, abs(lKt[i, c])), (i, t)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_nothing_missing_is_the_leave_one_out_conditional(cx):
    W, phi, lab, x, xs, gp = S.make_case(6, 3, 5, 2, 4, seed=9, cx=cx, label_site=2, ngrid=41)
    miss = np.zeros(x.shape, dtype=bool)
    levels = (0.1, 0.9)
    ref = M.marginal_conditionals_ref(W, phi, lab, miss, x, xs, gp, levels, scaled=False)
    for i in range(len(lab)):
        a = S.amplitudes(class_slice(W, int(lab[i])), phi[i])
        for t in range(x.shape[1]):
            r = ref.rho[i, t]
            outer = np.outer(a[t], np.conj(a[t]))
            k = np.vdot(outer, r) / np.vdot(outer, outer)        # a_t carries the scales of its rows
            assert np.abs(r - k * outer).max() <= 1e-12 * np.abs(r).max()
    sc = S.scaled_site_conditionals(W, phi, lab, x, xs, gp, levels)
    assert np.abs(ref.sc.F - sc.F).max() <= 1e-12
    assert np.abs(ref.sc.nll - sc.nll).max() <= 1e-10
    assert np.abs(ref.sc.pit - sc.pit).max() <= 1e-12
    ok = ~ref.excused
    assert np.array_equal(ref.sc.median[ok], sc.median[ok]) and np.array_equal(ref.sc.quantiles[ok], sc.quantiles[ok])


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_scaled_form_agrees_with_the_unscaled_one(cx):
    W, phi, lab, miss, x_in, xs, gp, _ = M.make_case(9, 3, 6, 2, 6, seed=21 + cx, cx=cx, label_site=4, ngrid=41)
    a = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gp, (0.25,), scaled=True)
    b = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gp, (0.25,), scaled=False)
    assert np.abs(a.sc.F - b.sc.F).max() <= 1e-12
    assert np.array_equal(np.isnan(a.sc.nll), np.isnan(b.sc.nll))
    assert np.nanmax(np.abs(a.sc.nll - b.sc.nll)) <= 1e-10
    assert np.abs(a.mean - b.mean).max() <= 1e-12


def test_scaled_form_holds_a_thousand_sites():
    W, phi, lab, miss, x_in, xs, gp, _ = M.make_case(1000, 4, 8, 2, 2, seed=5, long_chain=True, ngrid=21)
    ref = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gp)
    assert np.all(np.isfinite(ref.sc.F)) and np.all(np.isfinite(ref.mean))
    assert np.array_equal(np.isnan(ref.sc.nll), np.isnan(x_in))


def test_nan_pattern_and_untouched_states():
    W, phi, lab, miss, x_in, xs, gp, x = M.make_case(9, 4, 7, 2, 19, seed=3, ngrid=41)
    ref = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gp)
    held = miss & np.isfinite(x_in)
    assert held.any() and (miss & ~held).any() and np.isnan(phi[miss & ~held]).all()
    assert np.array_equal(np.isnan(ref.sc.nll), miss & ~held) and np.array_equal(np.isnan(ref.sc.pit), miss & ~held)
    assert np.all(np.isfinite(ref.sc.median)) and np.all(np.isfinite(ref.mean))
