"""Host side of the leave-one-out site conditionals: the NumPy restatement tests/site_cond_ref.py against the oracle's median imputer
with one missing site and against tests/impute_dist_ref.py, the numerator identity, the properties of the interpolated PIT, and the
argument checks of the Python layer that must raise before any engine exists."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import impute_numpy as I
from oracle import ref_numpy as R
from tests import impute_dist_ref as D
from tests import site_cond_ref as S
from tests.marginal_ref import class_slice

LEVELS = (0.05, 0.5, 0.95)
# (T, d, chi, C, complex)
SHAPES = [(6, 3, 4, 2, False), (9, 4, 7, 2, False), (7, 2, 3, 3, False), (7, 4, 5, 2, True)]
IDS = ["6-3-4-2", "9-4-7-2", "7-2-3-3", "7-4-5-2-fourier"]


def _case(T, d, chi, C, cx):
    return S.make_case(T, d, chi, C, 4, seed=1000 + 17 * T + 5 * d + chi + C, cx=cx, label_site=T // 2)


@pytest.mark.parametrize("T,d,chi,C,cx", SHAPES, ids=IDS)
def test_restatement_against_the_median_imputer_with_one_missing_site(T, d, chi, C, cx):
    """Medians, WMADs and levels identical to impute(..., [t], "median") and impute_dist_ref with levels; normalised cdf within 1e-12 (the
    bound of tests/test_impute_dist_host.py); the scaled form of the definition gives the same selections and the same cdf."""
    W, phi, lab, x, xs, gphi = _case(T, d, chi, C, cx)
    ref = S.site_conditionals_ref(W, phi, lab, x, xs, gphi, LEVELS)
    vec = S.scaled_site_conditionals(W, phi, lab, x, xs, gphi, LEVELS)
    assert ref.margins_ok() and vec.margins_ok()
    worst = worst_vec = 0.0
    for i in range(x.shape[0]):
        cm = class_slice(W, int(lab[i]))
        for t in range(T):
            xo, eo = I.impute(cm, phi[i], [t], xs, gphi, "median")
            assert xo[0] == ref.median[i, t] and eo[0] == ref.err[i, t]
            med, wm, cdfs, lidx, _ = D.impute_med_and_cdfs(cm, phi[i], [t], xs, gphi, "forwards", LEVELS)
            assert med[0] == ref.median[i, t] and wm[0] == ref.err[i, t]
            assert np.array_equal(lidx[0], ref.lev_idx[i, t]) and ref.lev_idx[i, t, 1] == ref.med_idx[i, t]
            worst = max(worst, float(np.abs(cdfs[0] - ref.F[i, t]).max()))
    worst_vec = float(np.abs(vec.F - ref.F).max())
    print(f"largest |F - impute_dist_ref| = {worst:.3e}, |F(scaled walk) - F| = {worst_vec:.3e}, "
          f"|nll(scaled walk) - nll| = {np.abs(vec.nll - ref.nll).max():.3e}")
    assert worst < 1e-12 and worst_vec < 1e-12
    assert np.array_equal(vec.med_idx, ref.med_idx) and np.array_equal(vec.err, ref.err) and np.array_equal(vec.lev_idx, ref.lev_idx)
    assert np.abs(vec.nll - ref.nll).max() < 1e-10 and np.abs(vec.pit - ref.pit).max() < 1e-12


@pytest.mark.parametrize("T,d,chi,C,cx", SHAPES, ids=IDS)
def test_numerator_is_the_squared_overlap_at_every_site(T, d, chi, C, cx):
    """|conj(phi_t) . a_t|^2 with the scales undone is one number for all t: |yhat_c|^2 of the oracle's contraction (1e-12 relative)."""
    W, phi, lab, x, xs, gphi = _case(T, d, chi, C, cx)
    yhat = R.contract_mps(W, phi)
    for i in range(x.shape[0]):
        a, ls = S.amplitudes(class_slice(W, int(lab[i])), phi[i], return_scales=True)
        want = abs(yhat[i, lab[i]]) ** 2
        got = np.array([abs(np.conj(phi[i, t]) @ a[t]) ** 2 * np.exp(2.0 * ls[t]) for t in range(T)])
        assert np.abs(got / want - 1.0).max() < 1e-12, (i, got, want)


def test_pit_properties():
    W, phi, lab, x, xs, gphi = _case(6, 3, 4, 2, False)
    ref = S.site_conditionals_ref(W, phi, lab, x, xs, gphi)
    F = ref.F[1, 2]
    assert all(S.pit_at(xs, F, xs[k]) == F[k] for k in range(len(xs)))                 # at a grid value: F_k
    assert S.pit_at(xs, F, -1.5) == 0.0 and S.pit_at(xs, F, xs[0]) == 0.0
    assert S.pit_at(xs, F, 1.5) == 1.0 and S.pit_at(xs, F, xs[-1]) == 1.0
    xx = np.sort(np.random.default_rng(5).uniform(-1.2, 1.2, 500))
    pp = np.array([S.pit_at(xs, F, v) for v in xx])
    assert np.all(np.diff(pp) >= 0.0) and pp.min() == 0.0 and pp.max() == 1.0      # non-decreasing in x
    assert np.all((ref.pit > 0.0) & (ref.pit < 1.0))


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
        mt.site_conditionals(_fake_problem(X), rows=[0, 1])
    with pytest.raises(ValueError, match="log_marginals.*impute_dataset"):
        mt.anomaly_scores(_fake_problem(X))
    X[1, 2] = np.inf
    with pytest.raises(ValueError):
        mt.site_conditionals(_fake_problem(X))
    with pytest.raises(ValueError, match="reduce"):
        mt.anomaly_scores(_fake_problem(np.zeros((3, 4))), reduce="sum")
    for bad in ((0.0,), (1.0,), (0.5, 1.5), tuple(np.linspace(0.05, 0.95, 17))):
        with pytest.raises(ValueError):
            mt.site_conditionals(_fake_problem(np.zeros((3, 4))), quantiles=bad)
        with pytest.raises(ValueError):
            conditionals.site_conditionals_model(None, [], np.zeros((1, 1, 1)), [0], np.zeros((1, 1)), np.zeros(2), np.zeros((2, 1)), levels=bad)
