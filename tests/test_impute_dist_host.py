"""Host side of the distribution outputs (get_cdfs, quantile bands): the NumPy restatement tests/impute_dist_ref.py against the
independent brute-force conditional densities, and the argument checks that must raise before any engine exists."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import impute_numpy as I
from tests import impute_dist_ref as D


def _chain(T, d, chi, cx, rng):
    dims = [1] + [min(chi, d ** min(j, T - j)) for j in range(1, T)] + [1]
    W = []
    for j in range(T):
        t = rng.normal(size=(dims[j], d, dims[j + 1]))
        if cx:
            t = t + 1j * rng.normal(size=t.shape)
        W.append(t)
    W[-1] = W[-1] / I.mps_norm3(W)
    return W


@pytest.mark.parametrize("order", ["forwards", "backwards"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("T,d,chi,sites", [(6, 3, 4, (1, 2, 4)), (5, 2, 3, (0, 3, 4)), (6, 3, 4, (0, 1, 2, 3, 4, 5)), (4, 2, 2, (2,))])
def test_restatement_against_the_brute_force_conditionals(T, d, chi, sites, cx, order):
    """cdf at every missing site == normalised cumulative trapezoid of brute_force_conditional(fixed = states of the medians chosen so
    far), 1e-12: both sides are fp64 sums of at most 201 terms of a [0, 1]-scaled quantity (201-point grid)."""
    rng = np.random.default_rng(17 * T + 5 * d + chi + len(sites) + (100 if cx else 0))
    W = _chain(T, d, chi, cx, rng)
    enc_m = mt.model_encoding("Fourier" if cx else "Legendre_No_Norm")
    xs = np.linspace(-1.0, 1.0, 201)
    grid_phi = np.asarray(enc_m.encode(xs, d))
    enc = np.asarray(enc_m.encode(rng.uniform(-0.9, 0.9, T), d))
    levels = (0.05, 0.5, 0.95)
    med, wm, cdfs, lidx, states = D.impute_med_and_cdfs(W, enc, sites, xs, grid_phi, order, levels)
    known = np.ones(T, dtype=bool)
    known[list(sites)] = False
    fixed = {}
    worst = 0.0
    ranks = range(len(sites)) if order == "forwards" else range(len(sites) - 1, -1, -1)
    for r in ranks:
        p = I.brute_force_conditional(W, enc, known, sites[r], fixed, grid_phi)
        c = I.cumul_trapz_even(xs, p)
        c = c / c[-1]
        worst = max(worst, float(np.abs(c - cdfs[r]).max()))
        assert np.abs(c - cdfs[r]).max() < 1e-12, (r, np.abs(c - cdfs[r]).max())
        assert med[r] == xs[int(np.argmin(np.abs(cdfs[r] - 0.5)))]
        for l, q in enumerate(levels):
            assert lidx[r, l] == int(np.argmin(np.abs(cdfs[r] - q)))
        assert np.array_equal(lidx[r, 1], int(np.argmin(np.abs(cdfs[r] - 0.5))))
        fixed[sites[r]] = states[r]
    # the plain median imputer of the oracle takes the same path
    xo, eo = I.impute(W, enc, sites, xs, grid_phi, "median", order, True)
    assert np.array_equal(xo, med) and np.array_equal(eo, wm)
    print(f"largest |cdf - brute force| = {worst:.3e}")


class _NoEngine:
    def __init__(self, *a, **k):
        raise AssertionError("an engine was constructed before the arguments were checked")


def _fake_problem():
    X = np.zeros((2, 4))
    return mt.ImputationProblem([], X, np.zeros(2), X, np.zeros(2), None, None, {0: 0})


@pytest.mark.parametrize("bad", [(0.0,), (1.0,), (0.5, 1.5), (-0.1,), tuple(np.linspace(0.05, 0.95, 17))],
                         ids=["zero", "one", "above", "below", "seventeen"])
def test_bad_levels_raise_before_an_engine_exists(monkeypatch, bad):
    from mpstime_jl_amd import imputation, engine
    monkeypatch.setattr(imputation, "SweepEngine", _NoEngine)
    with pytest.raises(ValueError):
        mt.impute_dataset(_fake_problem(), np.ones((2, 4), dtype=bool), "median", quantiles=bad)
    with pytest.raises(ValueError):
        engine.SweepEngine._dist_args(np.ones((2, 4), dtype=np.uint8), 201, 0, bad, 0, None)
    with pytest.raises(ValueError):
        engine.check_levels(bad)


@pytest.mark.parametrize("method", ["mode", "mean", "ITS"])
def test_quantiles_need_the_median(monkeypatch, method):
    from mpstime_jl_amd import imputation
    monkeypatch.setattr(imputation, "SweepEngine", _NoEngine)
    with pytest.raises(ValueError):
        mt.impute_dataset(_fake_problem(), np.ones((2, 4), dtype=bool), method, quantiles=(0.05, 0.95))


def test_get_cdfs_only_supports_the_median(monkeypatch):
    from mpstime_jl_amd import imputation
    monkeypatch.setattr(imputation, "SweepEngine", _NoEngine)
    with pytest.raises(ValueError, match="get_cdfs only supports method=:median"):
        mt.get_cdfs(_fake_problem(), 0, 0, [1, 2], method="mode")


def test_cdf_index_formula():
    from mpstime_jl_amd.engine import cdf_indices, cdf_points
    for n in (2, 3, 8, 201, 2001, 20001):
        for s in (1, 2, 7, 16, n, n + 5):
            k = cdf_indices(n, s)
            assert len(k) == cdf_points(n, s) == (n - 2) // s + 2
            assert k[0] == 0 and k[-1] == n - 1 and np.all(np.diff(k) > 0)
            assert np.array_equal(k[:-1], np.arange(len(k) - 1) * s)
