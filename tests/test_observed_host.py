"""The NumPy restatement of the observed conditionals (tests/observed_ref.py) pinned to independent forms, and the host half of the
Python layer (mpstime_jl_amd/observations.py: validation, the transform of intervals and noise sds), without a GPU."""
import types

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import observations as ob
from tests import margcond_ref as M
from tests import observed_ref as O
from tests.marginal_ref import class_slice, gaussian_chain


def _tiny(cx, seed=11):
    """T = 4, d = 3, chi = 3, all five kinds mixed: rows 0 .. 4 hold every kind at every site once"""
    T, d, N = 4, 3, 5
    inp = O.make_case(T, d, 3, 2, N, seed, cx=cx, label_site=1, ngrid=65)
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    rng = np.random.default_rng(seed)
    kind = ((np.arange(N)[:, None] + np.arange(T)[None, :]) % 5).astype(np.uint8)
    # rebuild the parameters for the new kinds from the case's generator: a fresh case with these kinds
    x = rng.uniform(-0.9, 0.9, (N, T))
    enc = mt.model_encoding("Fourier" if cx else "Legendre_No_Norm")
    phi = np.asarray(enc.encode(x.ravel(), d)).reshape(N, T, d)
    dx = xs[1] - xs[0]
    g, iv = kind == O.GAUSS, kind == O.INTERVAL
    a = np.where(g, x + 0.05, np.where(iv, x - 0.2, 0.0))
    b = np.where(g, 6 * dx, np.where(iv, x + 0.3, 0.0))
    E_user = O.random_operators(N, T, d, cx, rng)
    return W, phi, lab, kind, a, b, E_user, x, xs, gp


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_the_restatement_is_the_dense_amplitude_tensor(cx):
    W, phi, lab, kind, a, b, E_user, x, xs, gp = _tiny(cx)
    assert all(set(kind[:, t]) == {0, 1, 2, 3, 4} for t in range(kind.shape[1]))
    ref = O.observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x, xs, gp, scaled=False)
    for i in range(len(lab)):
        cm = class_slice(W, int(lab[i]))
        logev, rho = O.dense_evidence(cm, list(ref.E[i]))
        assert abs(logev - ref.logev[i]) <= 1e-12 * max(1.0, abs(logev)), (i, logev, ref.logev[i])
        for t in range(kind.shape[1]):
            scale = np.abs(rho[t]).max()
            assert np.abs(rho[t] - ref.rho[i, t]).max() <= 1e-13 * scale, (i, t)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_exact_and_missing_kinds_are_the_marginal_conditionals(cx):
    W, phi, lab, miss, x_in, xs, gp, x = M.make_case(9, 4, 7, 2, 7, 23, cx=cx, label_site=4, ngrid=65)
    kind = miss.astype(np.uint8)
    z = np.zeros(x_in.shape)
    ref = O.observed_conditionals_ref(W, phi, lab, kind, z, z, None, x_in, xs, gp, O.LEVELS)
    mc = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gp, O.LEVELS)
    assert np.array_equal(ref.rho, mc.rho)
    for f in ("nll", "pit", "median", "err", "quantiles"):
        assert np.array_equal(getattr(ref.pred, f), getattr(mc.sc, f), equal_nan=True), f
    assert np.array_equal(ref.pred_mean, mc.mean)
    # the posterior group: the predictive one at a missing site, NaN at an exact one
    assert np.array_equal(ref.post.median[miss], ref.pred.median[miss]) and np.all(np.isnan(ref.post.median[~miss]))
    assert np.array_equal(ref.post_mean[miss], ref.pred_mean[miss]) and np.all(np.isnan(ref.post_mean[~miss]))


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_scaled_form_agrees_with_the_unscaled_one(cx):
    W, phi, lab, kind, a, b, E_user, x, xs, gp = _tiny(cx)
    s = O.observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x, xs, gp, (0.25,), scaled=True)
    u = O.observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x, xs, gp, (0.25,), scaled=False)
    assert np.abs(s.logev - u.logev).max() <= 1e-12
    with np.errstate(invalid="ignore"):
        assert np.nanmax(np.abs(s.pred.nll - u.pred.nll)) <= 1e-12 and np.array_equal(np.isnan(s.pred.nll), np.isnan(u.pred.nll))
    assert np.abs(s.pred.F - u.pred.F).max() <= 1e-13
    ok = ~np.isnan(u.post.median)
    assert np.abs(s.post.F - u.post.F)[ok].max() <= 1e-13 and np.abs(s.post_mean - u.post_mean)[ok].max() <= 1e-13


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_an_operator_site_with_the_quadrature_of_a_gauss_site_acts_as_that_site(cx):
    W, phi, lab, kind, a, b, E_user, x, xs, gp = _tiny(cx)
    ref = O.observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x, xs, gp, O.LEVELS)
    g = kind == O.GAUSS
    kind2, E2 = np.where(g, O.OPERATOR, kind).astype(np.uint8), E_user.copy()
    E2[g] = ref.E[g]
    alt = O.observed_conditionals_ref(W, phi, lab, kind2, a, b, E2, x, xs, gp, O.LEVELS)
    assert np.array_equal(alt.rho, ref.rho) and np.array_equal(alt.logev, ref.logev)
    assert np.array_equal(alt.pred.nll, ref.pred.nll, equal_nan=True) and np.array_equal(alt.pred.median, ref.pred.median)
    assert np.array_equal(alt.post.median[~g], ref.post.median[~g], equal_nan=True) and np.all(np.isnan(alt.post.median[g]))


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_a_row_of_missing_sites_gives_the_norm_of_its_class(cx):
    rng = np.random.default_rng(5)
    T, d, C = 6, 3, 3
    W = gaussian_chain(T, d, 5, C, 2, cx, rng)
    xs = np.linspace(-1.0, 1.0, 33)
    gp = np.asarray(mt.model_encoding("Fourier" if cx else "Legendre_No_Norm").encode(xs, d))
    kind = np.full((C, T), O.MISSING, dtype=np.uint8)
    z = np.zeros((C, T))
    ref = O.observed_conditionals_ref(W, np.full((C, T, d), np.nan), np.arange(C), kind, z, z, None, np.full((C, T), np.nan), xs, gp)
    for c in range(C):
        psi = class_slice(W, c)[0][0]
        for w in class_slice(W, c)[1:]:
            psi = np.tensordot(psi, w, axes=([psi.ndim - 1], [0]))
        assert abs(ref.logev[c] - np.log(np.sum(np.abs(psi) ** 2))) <= 1e-12


long_reference, long_logev_distance = O.long_reference, O.long_logev_distance


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_logev_of_a_thousand_sites_against_the_longdouble_walk(cx):
    """Found: real 1.2e-12, complex 3.0e-13 (logev near -700 and -870: a few ulps of the sum).  The GPU test allows the device four
    times this, or 1e-10 if that is larger."""
    dist = long_logev_distance(cx)
    ref = long_reference(cx)
    print(f"T = 1000 {'complex' if cx else 'real'}: logev = {ref.logev}, |restatement - longdouble| = {dist:.3e}")
    assert np.all(np.isfinite(ref.logev))
    assert dist <= 1e-10                # 1000 logs of traces, each within an ulp of a number of size one: 1000 * 2^-53 * a few


@pytest.mark.parametrize("spec", O.gpu_cases(), ids=lambda s: f"{'-'.join(map(str, s[0]))}-{'cx' if s[1] else 're'}-{s[2]}-{s[3]}{'-persite' if s[4] else ''}")
def test_the_committed_seeds_excuse_at_most_one_pair_in_a_hundred(spec):
    shape, cx, label, ngrid, per_site = spec
    if shape == O.LONG:
        ref = long_reference(cx)
    else:
        W, phi, lab, kind, a, b, E_user, x_in, xs, gp = O.case(*shape, cx, label, ngrid, per_site)
        ref = O.observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x_in, xs, gp, O.LEVELS)
    print(f"excused {int(ref.excused.sum())} of {ref.excused.size}")
    assert ref.excused.mean() <= 0.01


def test_the_kinds_of_a_case_hold_every_pattern():
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = O.case(9, 4, 7, 2, 19)
    dx = xs[1] - xs[0]
    for k in range(5):
        assert np.all(kind[k] == k)
    assert (kind[5] == O.GAUSS).sum() == 1 and (kind[5] == O.EXACT).sum() == kind.shape[1] - 1
    assert all(len(set(row)) >= 3 for row in kind[6:])
    g, iv = kind == O.GAUSS, kind == O.INTERVAL
    assert np.all(b[g] >= 2 * dx * (1 - 1e-12)) and np.all(b[g] <= 40 * dx * (1 + 1e-12))
    assert np.all(a[iv] <= b[iv]) and np.all(a[iv] >= xs[0]) and np.all(b[iv] <= xs[-1])
    wid = (b - a)[iv]
    assert wid.min() <= dx * (1 + 1e-9) and wid.max() >= 0.5 * (xs[-1] - xs[0])       # from one grid spacing to (most of) the whole grid
    valued = (kind == O.EXACT) | ((kind == O.MISSING) & np.isfinite(x_in))
    assert np.all(np.isnan(phi[~valued])) and np.all(np.isfinite(phi[valued])) and np.all(np.isnan(E_user[kind != O.OPERATOR]))


# ---- the host half of the Python layer ----
def _problem(sigmoid):
    rng = np.random.default_rng(3)
    T, d = 6, 3
    Xtr = np.cumsum(rng.standard_normal((40, T)), axis=1)
    ytr = np.arange(40) % 2
    opts = mt.MPSOptions(encoding="Legendre_No_Norm", d=d, chi_max=4, nsweeps=1, verbosity=-1, sigmoid_transform=sigmoid)
    trained = types.SimpleNamespace(opts=opts, mps=gaussian_chain(T, d, 4, 2, T - 1, False, rng), custom_encoding=None,
                                    train_data=types.SimpleNamespace(original_data=Xtr, labels=ytr))
    Xte = np.cumsum(rng.standard_normal((5, T)), axis=1)
    return mt.init_imputation_problem(trained, Xte, np.arange(5) % 2, dx=0.01, verbosity=0)


def test_constructors_and_validation():
    x = np.array([[0.0, 1.0, np.nan, 2.0]])
    m = mt.gaussian_noise(x, [0.5, 0.0, 0.5, 0.1])
    assert m.kind.tolist() == [[ob.GAUSS, ob.EXACT, ob.MISSING, ob.GAUSS]] and m.b[0, 3] == 0.1
    assert mt.gaussian_noise(x, 0.3, missing_mask=[[True, False, False, False]]).kind.tolist() == [[1, 2, 1, 2]]
    m = mt.interval_observations([[0.0, 1.0, -np.inf, -np.inf]], [[1.0, 1.0, 2.0, np.inf]])
    assert m.kind.tolist() == [[ob.INTERVAL, ob.EXACT, ob.INTERVAL, ob.MISSING]]
    for bad in (lambda: mt.gaussian_noise(x, -1.0), lambda: mt.gaussian_noise(x, np.nan), lambda: mt.interval_observations([[1.0]], [[0.0]]),
                lambda: mt.interval_observations([[np.nan]], [[0.0]]), lambda: mt.ObservationModel([[5]], [[0.0]], [[0.0]]),
                lambda: mt.ObservationModel([[ob.GAUSS]], [[0.0]], [[0.0]]), lambda: mt.ObservationModel([[ob.OPERATOR]], [[0.0]], [[0.0]]),
                lambda: mt.ObservationModel([[ob.EXACT]], [[np.nan]], [[0.0]]), lambda: mt.ObservationModel([[0, 1]], [[0.0]], [[0.0]]),
                lambda: mt.ObservationModel([[ob.OPERATOR]], [[0.0]], [[0.0]], np.zeros((1, 1, 2, 3)))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("sigmoid", [False, True], ids=["affine", "sigmoid"])
def test_intervals_and_sds_go_through_the_test_transform(sigmoid):
    from mpstime_jl_amd.conditionals import _true_values
    from mpstime_jl_amd.imputation import _scaled_instances
    imp = _problem(sigmoid)
    X = imp.X_test
    N, T = X.shape
    kind = np.full((N, T), ob.GAUSS, dtype=np.uint8)
    kind[:, 1], kind[:, 2], kind[:, 3] = ob.INTERVAL, ob.EXACT, ob.MISSING
    sd = 0.3
    a = np.where(kind == ob.INTERVAL, X - 0.4, X)
    b = np.where(kind == ob.INTERVAL, X + 0.7, sd)
    b[0, 1], a[1, 1] = np.inf, -np.inf
    e = ob.encode_observations(imp, mt.ObservationModel(kind, a, b))
    valued = (kind == ob.GAUSS) | (kind == ob.EXACT)
    enc, norms, raw, _, scaled, oob = _scaled_instances(imp, np.arange(N), ~valued)
    xr = imp.x_guess_range.xvals
    assert np.array_equal(e.model.a[valued], scaled[valued]) and np.array_equal(e.x[kind == ob.EXACT], scaled[kind == ob.EXACT])
    assert np.all(np.isnan(e.x[kind != ob.EXACT]))
    # interval ends: the monotone transform of the row, exactly, then the clip to the grid
    lo = np.clip(_true_values(imp, enc, norms, np.where(np.isfinite(a), a, 0.0), oob), xr[0], xr[-1])
    hi = np.clip(_true_values(imp, enc, norms, np.where(np.isfinite(b), b, 0.0), oob), xr[0], xr[-1])
    iv = kind == ob.INTERVAL
    fin_a, fin_b = iv & np.isfinite(a), iv & np.isfinite(b)
    assert np.array_equal(e.model.a[fin_a], lo[fin_a]) and np.array_equal(e.model.b[fin_b], hi[fin_b])
    assert e.model.a[1, 1] == xr[0] and e.model.b[0, 1] == xr[-1] and np.all(e.model.a[iv] <= e.model.b[iv])
    # the sd: the slope of the transform at the observed value - a central difference of the transform itself
    g = kind == ob.GAUSS
    h = 1e-6
    num = (_true_values(imp, enc, norms, X + h, oob) - _true_values(imp, enc, norms, X - h, oob)) / (2 * h)
    assert np.abs(e.model.b[g] / sd - num[g]).max() <= 1e-6 * np.abs(num[g]).max()
    if not sigmoid:                     # an affine transform: the same factor at every site of a row
        assert np.abs(e.model.b[g].reshape(N, -1) / e.model.b[g].reshape(N, -1)[:, :1] - 1).max() <= 1e-14
    # domain="encoded": as they are
    ee = ob.encode_observations(imp, e.model, domain="encoded")
    assert np.array_equal(ee.model.a, e.model.a) and np.array_equal(ee.model.b, e.model.b)
    # an sd below the grid spacing is refused, with the advice
    with pytest.raises(ValueError, match="pass the value as exact"):
        ob.encode_observations(imp, mt.gaussian_noise(X, 1e-6))
    with pytest.raises(ValueError, match="shape"):
        ob.encode_observations(imp, mt.gaussian_noise(X[:2], 0.3))
    with pytest.raises(ValueError, match="domain"):
        ob.encode_observations(imp, mt.gaussian_noise(X, 0.3), domain="other")
