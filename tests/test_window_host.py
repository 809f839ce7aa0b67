"""Host side of the window conditionals: the two forms of the NumPy restatement tests/window_ref.py against each other and against the
dense amplitude tensor, the three facts of the definition, and the argument checks of the Python layer that must raise before any
engine exists.

The masked difference costs one full chain per window through ``marginal_ref._step``'s unoptimised einsum: on the shapes with
chi = 72 and on the long chains it runs for a subset of the (series, start) pairs - first, last and label-site starts included - and
for every pair elsewhere."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests import site_cond_ref as S
from tests import window_ref as WR
from tests.marginal_ref import class_slice, dense_log_marginal, gaussian_chain, label_site_of, normalised_chain, random_states

FORMS_TOL = 1e-10
FACTS_TOL = 1e-12

# the pairs of the masked form where all of them would take minutes
SUBSETS = {
    "big-real": [(0, 0), (0, 3), (1, 4), (1, 7)],
    "big-complex": [(0, 2), (1, 5)],
    "long-200": [(0, 0), (0, 100), (1, 196), (1, 199)],
    "long-1000": [(0, 0), (1, 500), (1, 997), (0, 999)],
}


@pytest.mark.parametrize("name", list(WR.SHAPES))
def test_the_two_forms_agree(name):
    W, phi, lab, mw = WR.make_case(name)
    N, T = phi.shape[:2]
    pairs = SUBSETS.get(name)
    loc = WR.window_nll_local(W, phi, lab, mw, pairs)
    msk = WR.window_nll_masked(W, phi, lab, mw, pairs)
    have = ~np.isnan(msk)
    want = ~WR.expected_nan(N, T, mw)
    if pairs is not None:
        sel = np.zeros((N, T, mw), dtype=bool)
        for i, t in pairs:
            sel[i, t] = True
        want = want & sel
    assert np.array_equal(have, want) and np.array_equal(~np.isnan(loc), want)
    worst = float(np.abs(loc[want] - msk[want]).max())
    print(f"{name}: largest |window-local - masked difference| = {worst:.3e} over {int(want.sum())} windows (bound {FORMS_TOL:g})")
    assert worst < FORMS_TOL


def test_worst_case_of_the_definition_on_a_normalised_chain():
    """(T, d, chi, C, N) = (9, 4, 7, 2, 5) on normalised_chain: the shape at which the two forms were furthest apart (4.2e-12)"""
    rng = np.random.default_rng(9472)
    W = normalised_chain(9, 4, 7, 2, rng)
    phi = random_states(5, 9, 4, False, rng)
    lab = (np.arange(5) % 2).astype(np.int32)
    loc, msk = WR.window_nll_local(W, phi, lab, 9), WR.window_nll_masked(W, phi, lab, 9)
    ok = ~WR.expected_nan(5, 9, 9)
    worst = float(np.abs(loc[ok] - msk[ok]).max())
    print(f"largest |window-local - masked difference| = {worst:.3e}")
    assert worst < FORMS_TOL


@pytest.mark.parametrize("cx,label_site", [(False, 6), (False, 0), (True, 3)], ids=["real-last", "real-first", "complex-mid"])
def test_both_forms_against_the_dense_amplitude_tensor(cx, label_site):
    """T = 7, d = 3: ln l from the full d^T tensor, every window of every series"""
    rng = np.random.default_rng(70 + label_site)
    T, d, C, N, mw = 7, 3, 2, 3, 7
    W = gaussian_chain(T, d, 5, C, label_site, cx, rng)
    phi = random_states(N, T, d, cx, rng)
    lab = np.array([0, 1, 1], dtype=np.int32)
    loc, msk = WR.window_nll_local(W, phi, lab, mw), WR.window_nll_masked(W, phi, lab, mw)
    worst = 0.0
    for i in range(N):
        full = dense_log_marginal(W, phi[i], np.zeros(T, dtype=bool), int(lab[i]))
        for t in range(T):
            for w in range(1, T - t + 1):
                m = np.zeros(T, dtype=bool)
                m[t:t + w] = True
                want = dense_log_marginal(W, phi[i], m, int(lab[i])) - full
                worst = max(worst, abs(loc[i, t, w - 1] - want), abs(msk[i, t, w - 1] - want))
    print(f"largest |form - dense| = {worst:.3e}")
    assert worst < FORMS_TOL


@pytest.mark.parametrize("name", ["ragged-tile", "second-tile", "complex-mid", "bond-17"])
def test_the_three_facts_of_the_definition(name):
    W, phi, lab, _ = WR.make_case(name)
    N, T = phi.shape[:2]
    nll = WR.window_nll_local(W, phi, lab, T)
    ok = ~WR.expected_nan(N, T, T)
    # unit-norm states: nll >= 0 and non-decreasing in the width (Cauchy-Schwarz)
    assert np.all(nll[ok] >= -FACTS_TOL)
    for w in range(1, T):
        both = ok[:, :, w]
        assert np.all(nll[:, :, w][both] >= nll[:, :, w - 1][both] - FACTS_TOL)
    # the whole chain: ln ||W_c||^2 - ln |yhat_c|^2
    yhat = R.contract_mps(W, phi)
    for i in range(N):
        cm = class_slice(W, int(lab[i]))
        psi = cm[0][0]
        for t in cm[1:]:
            psi = np.tensordot(psi, t, axes=([psi.ndim - 1], [0]))
        want = np.log(np.sum(np.abs(psi) ** 2)) - np.log(abs(yhat[i, lab[i]]) ** 2)
        assert abs(nll[i, 0, T - 1] - want) < FACTS_TOL * max(1.0, abs(want)), (i, nll[i, 0, T - 1], want)
        # width 1: -ln(|conj(phi_t) . a_t|^2 / sum_s |a_t[s]|^2)
        a = S.amplitudes(cm, phi[i])
        for t in range(T):
            w1 = -np.log(abs(np.conj(phi[i, t]) @ a[t]) ** 2 / np.sum(np.abs(a[t]) ** 2))
            assert abs(nll[i, t, 0] - w1) < FACTS_TOL * max(1.0, abs(w1)), (i, t, nll[i, t, 0], w1)


def test_label_site_is_where_the_shapes_say():
    for name, s in WR.SHAPES.items():
        if s["T"] <= 12:
            W = WR.make_case(name)[0]
            assert label_site_of(W) == s.get("label_site", s["T"] - 1)


class _NoEngine:
    def __init__(self, *a, **k):
        raise AssertionError("an engine was constructed before the arguments were checked")


def _fake_problem(X):
    return mt.ImputationProblem([], X, np.zeros(len(X)), X, np.zeros(len(X)), None, None, {0: 0})


def test_python_layer_checks_its_arguments_before_an_engine_exists(monkeypatch):
    from mpstime_jl_amd import conditionals
    monkeypatch.setattr(conditionals, "SweepEngine", _NoEngine)
    X = np.zeros((3, 4))
    X[1, 2] = np.nan
    with pytest.raises(ValueError, match="log_marginals.*impute_dataset"):
        mt.window_conditionals(_fake_problem(X), 2, rows=[0, 1])
    with pytest.raises(ValueError, match="log_marginals.*impute_dataset"):
        mt.window_anomaly_scores(_fake_problem(X), 2)
    good = _fake_problem(np.zeros((3, 4)))
    for bad in (0, 5, -1, 1.5):
        with pytest.raises(ValueError, match="max_width"):
            mt.window_conditionals(good, bad)
        with pytest.raises(ValueError, match="width"):
            mt.window_anomaly_scores(good, bad)
    with pytest.raises(ValueError, match="reduce"):
        mt.window_anomaly_scores(good, 2, reduce="sum")
