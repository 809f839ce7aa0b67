"""The Sahand-Legendre encodings on the host ("Sahand-Legendre encodings"): the density estimate, the fit and the encode
step of mpstime_jl_amd.encodings against tests/kde_ref.py - the loop-by-loop restatement -, the density against the exact Gaussian
sum, the bandwidth rule's branches, the properties the fit is built to have, and the path a custom encoding takes from the fit to
the imputation grid."""
import math

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import encodings as E
from tests import kde_ref as KR

EPS = np.finfo(np.float64).eps
REL = 1e-12                 # package against kde_ref, relative to each array's largest entry: the two differ in the order of summation only


def _bimodal(rng, shape):
    pick = rng.random(shape) < 0.45
    return np.clip(np.where(pick, rng.normal(-0.45, 0.18, shape), rng.normal(0.4, 0.22, shape)), -1.0, 1.0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def td_fit():
    """a time-dependent fit (T = 3, d = 4, 50 series) by the package and by kde_ref, shared and left unchanged"""
    rng = np.random.default_rng(101)
    X = _bimodal(rng, (50, 3))
    opts = mt.MPSOptions(encoding="Custom", d=4)
    args = E.init_sahand_legendre_time_dependent(X, None, opts=opts)
    return X, opts, args, KR.fit_time_dependent(X, 4)


def test_time_dependent_fit_and_encode_against_the_restatement(td_fit):
    X, opts, (kdes, minxs, scales, cvecs), ref = td_fit
    assert len(kdes) == 3 and all(k.npoints == 2048 and k.coef.shape == (2050,) for k in kdes)
    assert _rel([k.coef for k in kdes], [r[0]["coef"] for r in ref]) <= REL
    for name in ("lo", "step", "h"):
        assert _rel([getattr(k, name) for k in kdes], [r[0][name] for r in ref]) <= REL
    assert _rel(minxs, [r[1] for r in ref]) <= REL and _rel(scales, [r[2] for r in ref]) <= REL
    assert _rel(cvecs, [r[3] for r in ref]) <= REL
    rng = np.random.default_rng(102)
    Xq = rng.uniform(-1.0, 1.0, (9, 3))
    Xq[0], Xq[1] = -1.0, 1.0
    enc = mt.sahand_legendre(True)
    encoder = E.FittedEncoder(enc, 4, [kdes, minxs, scales, cvecs])
    got = encoder(Xq)
    assert got.shape == (9, 3, 4) and _rel(got, KR.encode_matrix(Xq, 4, ref)) <= REL
    # any shape of values, the site as the third argument
    one = E.sahand_legendre_encode(Xq[:, 1].reshape(3, 3), 4, 1, kdes, minxs, scales, cvecs)
    assert one.shape == (3, 3, 4) and np.array_equal(one.reshape(9, 4), got[:, 1])


def test_time_independent_fit_is_finite_and_is_the_one_column_fit():
    rng = np.random.default_rng(103)
    X = _bimodal(rng, (30, 5))
    opts = mt.MPSOptions(encoding="Custom", d=4)
    kd, minx, scale, cv = E.init_sahand_legendre(X, None, opts=opts)
    assert np.all(np.isfinite(cv)) and np.isfinite(minx) and minx > 0 and np.isfinite(scale) and scale > 0 and np.any(cv[3] != 0)
    kds, mn, sc, cvs = E.init_sahand_legendre_time_dependent(X.reshape(-1, 1), None, opts=opts, max_samples=max(200, X.shape[1]))
    assert np.array_equal(kd.coef, kds[0].coef) and (kd.lo, kd.step, kd.h) == (kds[0].lo, kds[0].step, kds[0].h)
    assert minx == mn[0] and scale == sc[0] and np.array_equal(cv, cvs[0])
    rk, rminx, rscale, rcv = KR.fit_time_independent(X, 4)
    assert _rel(kd.coef, rk["coef"]) <= REL and _rel(cv, rcv) <= REL and abs(minx - rminx) <= REL * rminx and abs(scale - rscale) <= REL * rscale
    enc = mt.sahand_legendre(False)
    assert not enc.istimedependent and enc.isdatadriven and enc.name == "Sahand-Legendre Time Independent"
    encoder = E.FittedEncoder(enc, 4, [kd, minx, scale, cv])
    Xq = rng.uniform(-1.0, 1.0, (4, 5))
    assert _rel(encoder(Xq), KR.encode_matrix(Xq, 4, (rk, rminx, rscale, rcv))) <= REL
    assert encoder.table(Xq[0], 5).shape == (5, 4)


@pytest.mark.parametrize("n", [12, 500, 4096])
def test_density_against_the_exact_gaussian_sum(n):
    """kde_pdf stays within twice the linear-binning bound delta^2 / (8 h^3 sqrt(2 pi)) of sum_i N(x - x_i; h) / n: the bound of
    binning the samples onto the grid, doubled to leave room for the interpolant's higher-order error."""
    rng = np.random.default_rng(n)
    xs = _bimodal(rng, n)
    k = E.kde(xs)
    q = np.linspace(-1.0, 1.0, 401)
    exact = np.exp(-0.5 * ((q[:, None] - xs[None, :]) / k.h) ** 2).sum(axis=1) / (n * k.h * math.sqrt(2.0 * math.pi))
    bound = 2.0 * k.step ** 2 / (8.0 * k.h ** 3 * math.sqrt(2.0 * math.pi))
    err = np.abs(E.kde_pdf(k, q) - exact).max()
    print(f"n = {n}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert E.kde_pdf(k, np.array([k.lo - 1e-9, k.hi + 1e-9])).tolist() == [0.0, 0.0]


def test_bandwidth_branches():
    n = 40
    assert E.kde(np.full(n, 0.3)).h == 0.9 * n ** (-0.2)                    # constant column: std = 0 and IQR = 0 -> w = 1
    xs = np.array([0.2] * 30 + [-0.7, 0.9, 0.5, -0.1])                      # IQR = 0, std > 0 -> w = std
    assert np.quantile(xs, 0.75) == np.quantile(xs, 0.25)
    assert abs(E.kde(xs).h - 0.9 * np.std(xs, ddof=1) * len(xs) ** (-0.2)) <= 4 * EPS
    assert E.kde(np.array([0.4])).h == 0.9                                  # n = 1
    assert E.kde(xs, bandwidth=0.05).h == 0.05
    rng = np.random.default_rng(5)
    ys = rng.normal(0.0, 0.3, 200)                                          # the regular branch: min(std, IQR / 1.34)
    q75, q25 = np.quantile(ys, [0.75, 0.25])
    assert abs(E.kde(ys).h - 0.9 * min(np.std(ys, ddof=1), (q75 - q25) / 1.34) * 200 ** (-0.2)) <= 4 * EPS
    for v in (xs, ys, np.array([0.4])):
        assert abs(E.kde(v).h - KR.bandwidth(v)) <= 4 * EPS
    k = E.kde(ys)
    assert k.lo == ys.min() - 4 * k.h and abs(k.hi - (ys.max() + 4 * k.h)) <= 1e-12 and k.step == (ys.max() + 4 * k.h - k.lo) / 2047


@pytest.mark.parametrize("d", [2, 4, 8])
def test_fit_properties(d):
    """With G = c M c^T under the trapezoid weights of the fit's own samples: G[n][n] = 1 for n >= 1 (every row is normalised by
    c^T M c) and G[0][0] = 1 / scale (f0 is divided by its squared norm, not by the norm).  The bound is the rounding of the d^2
    products and of the trapezoid sums behind M, relative to sum |c_i| M|x|_ij |c_j| - the same sum without its cancellation."""
    rng = np.random.default_rng(200 + d)
    X = np.clip(_bimodal(rng, (80, 3)) + 0.2, -1.0, 1.0)
    assert np.all(X.mean(axis=0) > 0.1)                                     # a nonzero mean keeps M[1][0] away from 0: the n = 1 row is finite
    opts = mt.MPSOptions(encoding="Custom", d=d)
    kdes, minxs, scales, cvecs = E.init_sahand_legendre_time_dependent(X, None, opts=opts)
    S = 200
    xs = np.linspace(-1.0, 1.0, S)
    assert np.all(np.isfinite(cvecs))
    for t in range(3):
        f0 = np.sqrt(np.maximum(E.kde_pdf(kdes[t], xs), 0.0))
        minx, scale = E.remove_zeros(xs, f0)
        assert minx == minxs[t] and scale == scales[t] and minx > 0
        w = np.full(S, xs[1] - xs[0])
        w[[0, -1]] *= 0.5
        pw = xs[None, :] ** np.arange(2 * d - 1)[:, None]
        mom, mabs = (pw * f0 ** 2 * w).sum(axis=1), (np.abs(pw) * f0 ** 2 * w).sum(axis=1)
        idx = np.add.outer(np.arange(d), np.arange(d))
        c = cvecs[t]
        G = c @ mom[idx] @ c.T
        tol = 4 * (d * d + 16) * EPS * np.diag(np.abs(c) @ mabs[idx] @ np.abs(c).T)
        assert abs(G[0, 0] - 1.0 / scale) <= tol[0] and np.all(c[0, 1:] == 0) and c[0, 0] == 1.0
        for n in range(1, d):
            assert abs(G[n, n] - 1.0) <= tol[n], (t, n, G[n, n] - 1.0, tol[n])
            assert np.all(c[n, n + 1:] == 0)
        one = E.sahand_legendre_coeffs(xs, f0, d)                           # the one-row call: the same solves outside the batch
        assert one.shape == (d, d) and np.allclose(one[:2], c[:2], rtol=1e-13, atol=0.0)


def test_sites_without_data_or_without_a_wavefunction_encode_to_zero():
    rng = np.random.default_rng(7)
    X = _bimodal(rng, (40, 4))
    X[:, 1] = 1.5                                                           # no value inside (-1, 1)
    X[:, 2] = 0.12345                                                       # with h = 1e-7 the density's grid misses every sample point
    opts = mt.MPSOptions(encoding="Custom", d=3)
    enc = mt.sahand_legendre(True)
    kdes, minxs, scales, cvecs = args = E.init_sahand_legendre_time_dependent(X, None, opts=opts, bandwidth=1e-7)
    assert not cvecs[1].any() and not cvecs[2].any() and minxs[2] == 0.0 and cvecs[0].any() and cvecs[3].any()
    encoder = E.FittedEncoder(enc, 3, args)
    Xq = rng.uniform(-1.0, 1.0, (6, 4))
    phi = encoder(Xq)
    assert np.all(phi[:, 1] == 0.0) and np.all(phi[:, 2] == 0.0) and np.all(np.isfinite(phi)) and np.any(phi[:, 0] != 0)
    ref = KR.fit_time_dependent(X, 3, bw=1e-7)
    assert ref[1][0] is None and ref[2][1] == 0.0
    assert _rel(phi, KR.encode_matrix(Xq, 3, ref)) <= REL
    tab = encoder.kde
    assert tab["per_site"] == 1 and tab["coef"].shape == (4, 2050) and tab["cvecs"].shape == (4, 3, 3) and not tab["coef"][1].any()


def test_a_value_outside_the_grid_encodes_at_the_floor():
    rng = np.random.default_rng(8)
    X = rng.uniform(0.2, 0.6, (60, 2))
    opts = mt.MPSOptions(encoding="Custom", d=3)
    kdes, minxs, scales, cvecs = E.init_sahand_legendre_time_dependent(X, None, opts=opts)
    assert kdes[0].lo > -0.9 and kdes[0].hi < 0.95
    for x in (-0.9, 0.95):
        got = E.sahand_legendre_encode(np.array([x]), 3, 0, kdes, minxs, scales, cvecs)[0]
        want = np.array([sum(cvecs[0][n, i] * x ** i for i in range(3)) for n in range(3)]) * minxs[0] / scales[0]
        assert np.all(got != 0) and np.abs(got - want).max() <= 8 * EPS * np.abs(want).max()


def test_a_nan_value_encodes_to_nan_on_the_host_as_on_the_device():
    rng = np.random.default_rng(11)
    opts = mt.MPSOptions(encoding="Custom", d=3)
    args = E.init_sahand_legendre_time_dependent(_bimodal(rng, (30, 2)), None, opts=opts)
    phi = E.sahand_legendre_encode(np.array([0.1, np.nan, -0.3]), 3, 0, *args)
    assert np.all(np.isnan(phi[1])) and np.all(np.isfinite(phi[[0, 2]]))
    assert np.isnan(E.kde_pdf(args[0][0], np.array([np.nan]))[0])


def test_names_symbols_and_the_pinned_errors():
    for td, name in ((True, "Sahand-Legendre Time Dependent"), (False, "Sahand-Legendre Time Independent")):
        enc = mt.sahand_legendre(time_dependent=td)
        assert enc.name == name and enc.range == (-1.0, 1.0) and not enc.iscomplex and enc.isdatadriven and enc.istimedependent == td
        sym = mt.symbolic_encoding(enc)
        assert sym == name.replace(" ", "_").replace("-", "_")
        canon, iscomplex, rng, data_driven = mt.options.encoding_info(sym)                   # the symbol is one the options know
        assert canon == ("SLTD" if td else "Sahand_Legendre") and not iscomplex and rng == enc.range and data_driven
        assert mt.model_encoding(enc) is enc                                                 # an Encoding comes back unchanged
        assert E.opts_encoding(mt.MPSOptions(encoding="Custom", d=4), enc) is enc
        assert E.encoding_from_name(name).name == name and mt.symbolic_encoding(E.encoding_from_name(name)) == sym
    assert mt.sahand_legendre().istimedependent
    for name in ("SLTD", "sahand_legendre", "hist_split_sltd"):
        with pytest.raises(NotImplementedError):
            mt.model_encoding(name)
    with pytest.raises(NotImplementedError, match="sahand_legendre"):
        mt.model_encoding("SLTD")


def test_fit_encode_and_imputation_grid_end_to_end_on_the_host(tmp_path):
    """T = 6, d = 3, 40 series, 2 classes: the path fitMPS takes on the host up to the sweep, then what init_imputation_problem
    derives again from the model's raw training data - the custom encoding travels inside the TrainedMPS."""
    rng = np.random.default_rng(9)
    T, d = 6, 3
    X, _ = mt.trendy_sine(T, 60, period=(4.0, 9.0), slope=[-1.0, 1.5], sigma=0.2, rng=rng)
    y = np.arange(60) % 2
    Xtr, ytr, Xte, yte = X[:40], y[:40], X[40:], y[40:]
    enc = mt.sahand_legendre(time_dependent=True)
    opts = mt.MPSOptions(encoding="Custom", d=d, chi_max=4, nsweeps=1, verbosity=-1)
    W, Xtr_, ytr_, Xte_, yte_, opts, enc_, class_keys = mt.training._fit_inputs(Xtr, ytr, Xte, yte, opts, enc)
    assert enc_ is enc
    tr, te = mt.training._encode_fit(Xtr_, ytr_, Xte_, yte_, opts, enc, class_keys)
    assert tr.phi.shape == (40, T, d) and te.phi.shape == (20, T, d) and np.all(np.isfinite(tr.phi)) and np.all(np.isfinite(te.phi))
    # the restatement on the same transformed data
    Xtr_s, Xte_s, norms, oob = E.transform_data(Xtr, Xte, opts, enc.range)
    ref = KR.fit_time_dependent(Xtr_s, d)
    assert _rel(tr.phi, KR.encode_matrix(Xtr_s[np.argsort(ytr, kind="stable")], d, ref)) <= REL
    assert _rel(te.phi, KR.encode_matrix(Xte_s[np.argsort(yte, kind="stable")], d, ref)) <= REL
    trained = mt.TrainedMPS(W, opts, tr, enc)
    imp = mt.init_imputation_problem(trained, Xte, yte, dx=1e-3, verbosity=0)
    xr = imp.x_guess_range
    assert len(xr.xvals) == 2001 and xr.xvals_enc.shape == (T, 2001, d) and imp.custom_encoding is enc
    for t in range(T):
        want = np.array([KR.encode_value(float(x), d, ref[t]) for x in xr.xvals])
        assert _rel(xr.xvals_enc[t], want) <= REL, t
    assert mt.init_imputation_problem(trained, Xte, yte, verbosity=0).x_guess_range.xvals_enc.shape == (T, 20001, d)      # dx = 1e-4
    # fit_encoding_from_training_data with the custom encoding; without it the options alone cannot name it
    _, _, encoder = E.fit_encoding_from_training_data(opts, Xtr, ytr, enc)
    assert np.array_equal(encoder(Xtr_s[np.argsort(ytr, kind="stable")]), tr.phi)
    with pytest.raises(ValueError, match="custom"):
        E.fit_encoding_from_training_data(opts, Xtr, ytr)
    with pytest.raises(NotImplementedError, match="closed-form bases only"):
        mt.impute_dataset(imp, np.ones(Xte.shape, dtype=bool), "mean")
    # save and load: the name is stored, the constructor rebuilds the encoding
    path = str(tmp_path / "model.npz")
    mt.save_trained_mps(path, trained)
    back = mt.load_trained_mps(path)
    assert back == trained and back.custom_encoding.name == enc.name and back.custom_encoding.init is enc.init
    imp2 = mt.init_imputation_problem(back, Xte, yte, dx=1e-3, verbosity=0)
    assert np.array_equal(imp2.x_guess_range.xvals_enc, xr.xvals_enc)
    # the encoding is part of the model's identity; one handed over must carry the stored name
    other = mt.TrainedMPS(trained.mps, opts, tr, mt.sahand_legendre(False))
    assert other != trained and mt.TrainedMPS(trained.mps, opts, tr, None) != trained
    assert mt.load_trained_mps(path, custom_encoding=enc).custom_encoding is enc
    with pytest.raises(ValueError, match="Time Dependent"):
        mt.load_trained_mps(path, custom_encoding=mt.sahand_legendre(False))
    # a file without a name - as saved before names were stored - and a name no constructor builds load with the field empty
    z = dict(np.load(path))
    del z["custom_encoding_name"]
    old = str(tmp_path / "old.npz")
    np.savez_compressed(old, **z)
    assert mt.load_trained_mps(old).custom_encoding is None and mt.load_trained_mps(old, custom_encoding=enc).custom_encoding is enc
    mine = E.function_basis(lambda x, d: np.ones(d), False, (-1.0, 1.0), name="Mine")
    np.savez_compressed(old, custom_encoding_name="Mine", **z)
    assert mt.load_trained_mps(old).custom_encoding is None and mt.load_trained_mps(old, custom_encoding=mine).custom_encoding is mine

