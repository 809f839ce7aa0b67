"""The projected bases on the host ("Projected bases"): the fit and the encoders of mpstime_jl_amd.encodings against
tests/proj_ref.py - the loop-by-loop restatement -, the reference's quirk that stays, the degenerate sites, names and pinned errors,
and the path a projected encoding takes from the fit to the imputation grid and through save / load."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import encodings as E
from tests import proj_ref as PR

EPS = np.finfo(np.float64).eps
GAP = 1e-9                  # the selection is compared only where the restatement's own cut is this clear, relative to the largest |c|^2


def _bimodal(rng, N, T):
    """two Gaussian modes plus a shift that differs from site to site"""
    pick = rng.random((N, T)) < 0.45
    X = np.where(pick, rng.normal(-0.45, 0.18, (N, T)), rng.normal(0.4, 0.22, (N, T)))
    return np.clip(X + np.linspace(-0.25, 0.25, T), -1.0, 1.0)


def _opts(d, cx=False, **kw):
    return mt.MPSOptions(encoding="Custom", d=d, dtype="ComplexF64" if cx else "Float64", **kw)


def _cut_is_clear(abs2, d, pair_ties=False):
    """The condition on the inputs: at every site the d-th and the (d + 1)-th largest |c|^2 of the restatement lie at least GAP of the
    largest apart.  Fourier: a pair +f / -f is an exact tie by definition and is resolved by position, not by size; where the cut falls
    inside such a pair the gaps to the members next to the pair count instead."""
    gaps = []
    for site in abs2:
        order = PR.select(site, len(site))
        v = [site[p - 1] for p in order]
        lo, hi = d - 1, d
        if pair_ties and v[lo] == v[hi]:
            assert PR.fourier_freqs(len(site))[order[lo] - 1] == -PR.fourier_freqs(len(site))[order[hi] - 1] > 0
            gaps.append(min(v[lo - 1] - v[lo], v[hi] - v[hi + 1]) / v[0])
        else:
            gaps.append((v[lo] - v[hi]) / v[0])
    print(f"smallest relative gap at the cut: {min(gaps):.3e}")
    return min(gaps) >= GAP


SHAPES = [(40, 6, 3), (64, 5, 4), (30, 4, 6)]


@pytest.fixture(scope="module")
def fits():
    """the restatement's fits of the three shapes, both families: computed once, shared and left unchanged"""
    out = {}
    for N, T, d in SHAPES:
        X = _bimodal(np.random.default_rng(100 * N + d), N, T)
        out[N, T, d] = (X, PR.fit(X, d, "legendre"), PR.fit(X, d, "fourier"))
    return out


@pytest.mark.parametrize("N,T,d", SHAPES)
def test_legendre_fit_against_the_restatement(fits, N, T, d):
    X, (ds, abs2), _ = fits[N, T, d]
    assert _cut_is_clear(abs2, d)
    (got,) = E.project_legendre(X, None, opts=_opts(d))
    assert got.shape == (T, d) and np.issubdtype(got.dtype, np.integer) and got.tolist() == ds
    assert got.min() >= 1 and got.max() <= 7 * d
    assert np.array_equal(mt.legendre(norm=True, project=True).init(X, None, opts=_opts(d))[0], got)
    for t in range(T):                                                     # the one-vector forms of the reference, site by site
        xs, wf = E.construct_kerneldensity_wavefunction(X[:, t][(X[:, t] >= -1) & (X[:, t] <= 1)], (-1.0, 1.0), max_samples=max(200, 2 * N))
        assert len(xs) == max(200, 2 * N) and np.all(wf >= 0)
        assert E.series_expand(E._legendre_table(xs, 7 * d).T, xs, wf, d).tolist() == ds[t]
        assert E.series_expand([lambda x, k=k: E._legendre_table(x, k + 1)[..., k] for k in range(7 * d)], xs, wf, d).tolist() == ds[t]


@pytest.mark.parametrize("N,T,d", SHAPES)
def test_fourier_fit_against_the_restatement_and_its_ties(fits, N, T, d):
    X, _, (ds, abs2) = fits[N, T, d]
    assert _cut_is_clear(abs2, d, pair_ties=True)
    (got,) = E.project_fourier(X, None, opts=_opts(d, cx=True))
    assert got.shape == (T, d) and got.tolist() == ds and got.min() >= 1 and got.max() <= 10 * d
    freqs = E.projected_fourier_freqs(got, d)
    assert np.array_equal(freqs, np.asarray(PR.fourier_freqs(10 * d))[got - 1])
    for t in range(T):
        f = freqs[t].tolist()
        for j, v in enumerate(f):                                          # -f never stands before +f: the exact tie goes to +f
            if v < 0:
                assert v == -f[j - 1] and j > 0, (t, f)
        if d % 2 == 0:                                                     # f = 0 and whole pairs leave one +f without its partner
            assert f[-1] > 0 and -f[-1] not in f, (t, f)


@pytest.mark.parametrize("norm", [False, True])
def test_legendre_encoder_against_the_restatement(fits, norm):
    X, (ds, _), _ = fits[64, 5, 4]
    rng = np.random.default_rng(3)
    Xq = rng.uniform(-1.0, 1.0, (11, 5))
    Xq[0], Xq[1] = -1.0, 1.0
    enc = mt.legendre(norm=norm, project=True)
    encoder = E.FittedEncoder(enc, 4, [np.asarray(ds)])
    got = encoder(Xq)
    e_ref, want = PR.float64_loss(Xq, ds, "legendre", 4, norm)
    print(f"largest |package - restatement| {np.abs(got - want).max():.3e}, e_ref {e_ref:.3e}")
    assert got.shape == (11, 5, 4) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 4 * e_ref + 16 * EPS * max(1.0, np.abs(want).max())
    one = enc.encode(Xq[:, 2].reshape(1, 11), 4, 2, np.asarray(ds))         # any shape of values, the site as the third argument
    assert one.shape == (1, 11, 4) and np.array_equal(one[0], got[:, 2])
    tab = encoder.orders
    assert tab["basis"] == ("Legendre_Norm" if norm else "Legendre_No_Norm") and tab["orders"].dtype == np.int32
    assert np.array_equal(tab["orders"], np.asarray(ds)) and tab["inv_norm"].shape == (5,)
    m = np.asarray(ds).max(axis=1)
    assert np.allclose(tab["inv_norm"], 1.0 / np.sqrt(np.sqrt((2 * m + 1) / 2) * m) if norm else 1.0, rtol=4 * EPS, atol=0)
    assert encoder.kde is None and encoder.bins is None


def test_fourier_encoder_against_the_restatement(fits):
    X, _, (ds, _) = fits[30, 4, 6]
    rng = np.random.default_rng(4)
    Xq = rng.uniform(-1.0, 1.0, (9, 4))
    Xq[0], Xq[1] = -1.0, 1.0
    enc = mt.fourier(project=True)
    encoder = E.FittedEncoder(enc, 6, [np.asarray(ds)])
    got = encoder(Xq)
    e_ref, want = PR.float64_loss(Xq, ds, "fourier", 6)
    print(f"largest |package - restatement| {np.abs(got - want).max():.3e}, e_ref {e_ref:.3e}")
    assert got.shape == (9, 4, 6) and got.dtype == np.complex128
    assert np.abs(got - want).max() <= 4 * e_ref + 16 * EPS
    assert np.abs(np.abs(got) - 1 / np.sqrt(6)).max() <= 4 * EPS
    tab = encoder.orders
    assert tab["basis"] == "Fourier" and np.array_equal(tab["orders"], np.asarray(PR.fourier_freqs(60))[np.asarray(ds) - 1])
    assert np.abs(tab["orders"]).max() <= 5 * 6 and np.all(tab["inv_norm"] == 1.0)


def test_the_order_used_is_one_above_the_order_selected():
    """The reference's quirk, pinned: positions [1, 3, 5] - the terms of order 0, 2, 4 - encode P_1, P_3, P_5, never the constant."""
    ds = np.array([[1, 3, 5], [2, 1, 4]])
    x = np.array([-1.0, -0.3, 0.0, 0.77, 1.0])
    got = E.projected_legendre_encode_no_norm(x, 3, 0, ds)
    table = E.legendre_encode_no_norm(x, 6)                                 # the closed-form basis: column k = order k
    assert np.array_equal(got, table[:, [1, 3, 5]])
    assert not np.any(np.all(got == table[:, [0]], axis=0))                 # no column is the constant sqrt(1/2)
    assert np.array_equal(E.projected_legendre_encode_no_norm(x, 3, 1, ds), table[:, [2, 1, 4]])
    normed = E.projected_legendre_encode(x, 3, 0, ds)                       # norm: m = 5, one scalar for the site
    assert np.allclose(normed, table[:, [1, 3, 5]] / np.sqrt(np.sqrt(11 / 2) * 5), rtol=4 * EPS, atol=0)
    assert E.FittedEncoder(mt.legendre(project=True), 3, [ds]).orders["orders"].tolist() == ds.tolist()


def test_a_site_without_values_in_range_and_a_nan_value():
    rng = np.random.default_rng(5)
    X = _bimodal(rng, 30, 3)
    X[:, 1] = 1.5                                                           # no value inside (-1, 1): wf = 0, every |c|^2 = 0
    for enc, d, cx in ((mt.legendre(project=True), 3, False), (mt.legendre(norm=True, project=True), 3, False),
                       (mt.fourier(project=True), 4, True)):
        (ds,) = enc.init(X, None, opts=_opts(d, cx))
        assert ds[1].tolist() == list(range(1, d + 1))
        kind = "fourier" if cx else "legendre"
        assert PR.fit(X[:, 1:2], d, kind)[0] == [list(range(1, d + 1))]
        encoder = E.FittedEncoder(enc, d, [ds])
        Xq = rng.uniform(-1.0, 1.0, (5, 3))
        phi = encoder(Xq)
        assert np.all(np.isfinite(phi)) and np.any(phi[:, 1] != 0)
        Xq[2, 0] = np.nan
        phin = encoder(Xq)
        assert np.all(np.isnan(phin[2, 0])) and np.all(np.isfinite(np.delete(phin.reshape(15, d), 6, axis=0)))
    assert np.all(E.construct_kerneldensity_wavefunction(np.zeros(0), np.linspace(-1, 1, 7)) == 0.0)


def test_names_symbols_and_the_pinned_errors():
    built = ((mt.legendre(project=True), "Projected Legendre", False, E.project_legendre),
             (mt.legendre_no_norm(project=True), "Projected Legendre", False, E.project_legendre),
             (mt.legendre(norm=True, project=True), "Projected Legendre_Norm", False, E.project_legendre),
             (mt.fourier(project=True), "Projected Fourier", True, E.project_fourier))
    for enc, name, cx, init in built:
        assert enc.name == name and enc.range == (-1.0, 1.0) and enc.iscomplex == cx and enc.istimedependent and enc.isdatadriven
        assert enc.init is init
        sym = mt.symbolic_encoding(enc)
        assert sym == name.replace(" ", "_")
        canon, iscomplex, rng, data_driven = mt.options.encoding_info(sym)
        assert canon == sym and iscomplex == cx and rng == enc.range and data_driven
        back = E.encoding_from_name(name)
        assert back == enc and mt.symbolic_encoding(back) == sym
        assert mt.model_encoding(enc) is enc and E.opts_encoding(_opts(4, cx), enc) is enc
        with pytest.raises(NotImplementedError, match="project=True"):      # the symbol stays unbuilt and names the constructor
            mt.model_encoding(sym)
        with pytest.raises(NotImplementedError, match="projected_basis"):
            E.opts_encoding(mt.MPSOptions(encoding=sym, d=4))
        with pytest.raises(ValueError, match="Splitting up a data-driven encoding"):
            mt.encodings.histogram_split(enc)
        with pytest.raises(ValueError, match="Splitting up a data-driven encoding"):
            mt.encodings.uniform_split(enc)
    # project=False: what model_encoding builds today
    assert mt.legendre() == mt.model_encoding("Legendre_No_Norm") == mt.legendre_no_norm()
    assert mt.legendre(norm=True) == mt.model_encoding("Legendre_Norm") and mt.fourier() == mt.model_encoding("Fourier")
    assert mt.legendre().init is None and not mt.fourier().isdatadriven
    assert E.FittedEncoder(mt.legendre(), 4, []).orders is None
    # the option and the symbols keep raising
    with pytest.raises(NotImplementedError, match="projected_basis"):
        E.opts_encoding(mt.MPSOptions(projected_basis=True))
    with pytest.raises(NotImplementedError, match="projected_basis"):
        mt.model_encoding("Fourier", project=True)
    with pytest.raises(NotImplementedError, match="encode_classes_separately"):
        E.fit_encoding(mt.legendre(project=True), np.zeros((4, 3)), np.zeros(4, dtype=int), _opts(3, encode_classes_separately=True))
    # a complex custom encoding needs a complex dtype, and the error says which option to change
    X = np.random.default_rng(2).normal(size=(10, 6))
    with pytest.raises(ValueError, match="dtype"):
        mt.fitMPS(X, np.zeros(10, dtype=int), opts=mt.MPSOptions(encoding="Custom", d=4), custom_encoding=mt.fourier(project=True))
    for spelling in ("Custom", ":Custom", "custom"):
        with pytest.raises(ValueError, match="dtype"):
            mt.fitMPS(X, np.zeros(10, dtype=int), opts=mt.MPSOptions(encoding=spelling, d=4, dtype="Float32"), custom_encoding=mt.fourier(project=True))


@pytest.mark.parametrize("kind", ["legendre", "legendre_norm", "fourier"])
def test_fit_encode_and_imputation_grid_end_to_end_on_the_host(tmp_path, kind):
    """T = 6, d = 3, 40 + 20 series, 2 classes: the path fitMPS takes on the host up to the sweep, then what init_imputation_problem
    derives again from the model's raw training data, and the save / load round trip."""
    rng = np.random.default_rng(9)
    T, d = 6, 3
    X, _ = mt.trendy_sine(T, 60, period=(4.0, 9.0), slope=[-1.0, 1.5], sigma=0.2, rng=rng)
    y = np.arange(60) % 2
    Xtr, ytr, Xte, yte = X[:40], y[:40], X[40:], y[40:]
    cx, norm = kind == "fourier", kind == "legendre_norm"
    enc = mt.fourier(project=True) if cx else mt.legendre(norm=norm, project=True)
    opts = _opts(d, cx, chi_max=4, nsweeps=1, verbosity=-1)
    W, Xtr_, ytr_, Xte_, yte_, opts, enc_, class_keys = mt.training._fit_inputs(Xtr, ytr, Xte, yte, opts, enc)
    assert enc_ is enc and W[0].dtype == (np.complex128 if cx else np.float64)
    tr, te = mt.training._encode_fit(Xtr_, ytr_, Xte_, yte_, opts, enc, class_keys)
    assert tr.phi.shape == (40, T, d) and te.phi.shape == (20, T, d) and np.all(np.isfinite(tr.phi)) and np.all(np.isfinite(te.phi))
    # the restatement on the same transformed data
    Xtr_s, Xte_s, norms, oob = E.transform_data(Xtr, Xte, opts, enc.range)
    fam = "fourier" if cx else "legendre"
    ds, abs2 = PR.fit(Xtr_s, d, fam)
    assert _cut_is_clear(abs2, d, pair_ties=cx)
    for phi, Xs, ys in ((tr.phi, Xtr_s, ytr), (te.phi, Xte_s, yte)):
        Xs = Xs[np.argsort(ys, kind="stable")]
        e_ref, want = PR.float64_loss(Xs, ds, fam, d, norm)
        assert np.abs(phi - want).max() <= 4 * e_ref + 16 * EPS * max(1.0, np.abs(want).max())
    trained = mt.TrainedMPS(W, opts, tr, enc)
    imp = mt.init_imputation_problem(trained, Xte, yte, dx=1e-3, verbosity=0)
    xr = imp.x_guess_range
    assert len(xr.xvals) == 2001 and xr.xvals_enc.shape == (T, 2001, d) and imp.custom_encoding is enc
    _, _, encoder = E.fit_encoding_from_training_data(opts, Xtr, ytr, enc)
    assert encoder.orders["orders"].shape == (T, d) and encoder.args[0].tolist() == ds
    for t in range(T):
        assert np.array_equal(xr.xvals_enc[t], enc.encode(xr.xvals, d, t, *encoder.args)), t
    assert np.array_equal(encoder(Xtr_s[np.argsort(ytr, kind="stable")]), tr.phi)
    with pytest.raises(NotImplementedError, match="closed-form bases only"):
        mt.impute_dataset(imp, np.ones(Xte.shape, dtype=bool), "mean")
    # save and load: the name is stored, the constructor rebuilds the encoding
    path = str(tmp_path / "model.npz")
    mt.save_trained_mps(path, trained)
    back = mt.load_trained_mps(path)
    assert back == trained and back.custom_encoding == enc and back.custom_encoding.init is enc.init
    imp2 = mt.init_imputation_problem(back, Xte, yte, dx=1e-3, verbosity=0)
    assert np.array_equal(imp2.x_guess_range.xvals_enc, xr.xvals_enc)
    with pytest.raises(ValueError, match=enc.name):
        mt.load_trained_mps(path, custom_encoding=mt.sahand_legendre(True))
