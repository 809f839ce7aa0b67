"""The Sahand-Legendre encodings on the device: k_encode_kde against the host encoder element by element (alone and behind the whole
front end), fitMPS with the encoding on both routes, imputation on the trained model against tests/impute_td_ref.py, and the checks
of the C ABI.

The tolerance of an encoded value.  Host and device evaluate the same expressions from the same tables; they differ in the rounding
of the spline (no fused multiply-add on either side, but x^i is pow on the host and a running product on the device) and of the
polynomial sum.  With f0 = max(sqrt(pdf), minx), e_f = 8 eps max(|c_{i-1}|, |c_i|, |c_{i+1}|) / minx - the spline's rounding carried
through the square root, which is at least minx above the floor - the bound per entry is
    (e_f + 32 d eps f0) sum_i |cvecs[n][i]| |x|^i / scale.
Behind the preprocessing the value x itself differs by the device's exp(): the bound grows by FRONT_END = 1e-13 on the state, what
tests/test_gpu_encode.py allows a state behind the same front end."""
import ctypes as C

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import _lib as L
from mpstime_jl_amd import encodings as E
from oracle import impute_numpy as I
from tests import impute_td_ref as TD
from tests.test_gpu_split import _accept

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FRONT_END = 1e-13


def _bimodal(rng, shape, shift=0.15):
    pick = rng.random(shape) < 0.45
    return np.clip(np.where(pick, rng.normal(-0.45, 0.18, shape), rng.normal(0.4, 0.22, shape)) + shift, -1.0, 1.0)


def _fit(X, d, time_dependent=True, **kw):
    enc = mt.sahand_legendre(time_dependent)
    opts = mt.MPSOptions(encoding="Custom", d=d)
    args = enc.init(X, None, opts=opts, **kw)
    return enc, E.FittedEncoder(enc, d, args)


def _tolerance(encoder, X):
    """the bound of the module docstring for every entry of encoder(X), (N, T, d)"""
    tab = encoder.kde
    d, K = encoder.d, tab["npoints"]
    N, T = X.shape
    site = np.arange(T) if tab["per_site"] else np.zeros(T, dtype=np.int64)
    lo, step, minx, scale = (tab[k][site][None, :] for k in ("lo", "step", "minx", "scale"))
    i = np.clip(np.rint((X - lo) / step + 1.0), 1, K).astype(np.int64)
    coef = np.abs(tab["coef"])[site]                                           # (T, K + 2)
    cmax = np.max([np.take_along_axis(coef, (i + o).T, axis=1).T for o in (-1, 0, 1)], axis=0)
    k = [E.UnivariateKDE(tab["lo"][s], tab["step"][s], 0.0, tab["coef"][s]) for s in site]
    f0 = np.stack([np.maximum(np.sqrt(np.maximum(E.kde_pdf(k[t], X[:, t]), 0.0)), tab["minx"][site[t]]) for t in range(T)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_f = np.where(minx > 0, 8 * EPS * cmax / minx, 0.0)
    pabs = np.einsum("tni,bti->btn", np.abs(tab["cvecs"])[site], np.abs(X)[..., None] ** np.arange(d))
    return (e_f + 32 * d * EPS * f0)[..., None] * pabs / scale[..., None]


def _compare(dev, host, tol, zero_sites=()):
    assert dev.shape == host.shape and dev.dtype == np.float64
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(dev))
    excess = np.abs(dev - host) - tol
    print(f"largest |device - host| {np.abs(dev - host).max():.3e}, largest excess over the bound {excess.max():.3e}, "
          f"largest |state| {np.abs(host).max():.3e}")
    assert np.all(excess <= 0)
    for t in zero_sites:
        assert np.all(dev[:, t] == 0.0) and np.all(host[:, t] == 0.0)


@pytest.mark.parametrize("N,T,d,td", [(37, 5, 4, True), (300, 3, 2, True), (33, 4, 12, True), (64, 1, 4, False)],
                         ids=["per_site_d4", "not_a_multiple_of_256_d2", "d12", "one_table_T1"])
def test_device_encoder_against_the_host_encoder(engine_cls, N, T, d, td):
    """encode_values without transforms: host and device see the same x bit for bit.  d = 2 is the n = 1 row alone, d = 12 the worst
    cancellation in the polynomial sum, (300, 3) leaves the last block partly empty, T = 1 with one table for all sites."""
    rng = np.random.default_rng(1000 * N + d)
    enc, encoder = _fit(_bimodal(rng, (80, T)), d, td)
    tab = encoder.kde
    assert tab["per_site"] == int(td) and np.all(np.isfinite(tab["cvecs"])) and np.all(tab["cvecs"][:, d - 1].any(axis=-1))
    X = rng.uniform(-1.0, 1.0, (N, T))
    X[0], X[1] = -1.0, 1.0
    host = encoder(X)
    eng = engine_cls(0)
    try:
        dev, sec = eng.encode_values(X, enc, d=d, kde=encoder)
        dev2, _ = eng.encode_values(X, enc, d=d, kde=tab)                  # the tables themselves
    finally:
        eng.close()
    assert sec > 0 and np.array_equal(dev, dev2)
    _compare(dev, host, _tolerance(encoder, X))


def test_zero_site_and_the_ends_of_the_grid(engine_cls):
    """Site 1 has no value inside the range: zero coefficients, exact zeros from both sides.  Sites 0 and 2 are fitted to values in
    [0.2, 0.6], so their grids end inside (-1, 1): the values lo and hi themselves, the doubles next to them and values well beyond
    are encoded - outside the grid at the floor minx."""
    rng = np.random.default_rng(77)
    Xfit = rng.uniform(0.2, 0.6, (60, 3))
    Xfit[:, 1] = 1.5
    enc, encoder = _fit(Xfit, 3)
    tab = encoder.kde
    assert not tab["cvecs"][1].any() and tab["cvecs"][0].any() and tab["cvecs"][2].any()
    X = rng.uniform(-1.0, 1.0, (21, 3))
    for t in (0, 2):
        lo, hi = tab["lo"][t], tab["lo"][t] + (tab["npoints"] - 1) * tab["step"][t]
        assert -1.0 < lo and hi < 1.0
        X[:8, t] = [lo, hi, np.nextafter(lo, -1.0), np.nextafter(hi, 1.0), np.nextafter(lo, 1.0), np.nextafter(hi, -1.0), lo - 0.05, hi + 0.05]
    host = encoder(X)
    eng = engine_cls(0)
    try:
        dev, _ = eng.encode_values(X, enc, d=3, kde=encoder)
    finally:
        eng.close()
    _compare(dev, host, _tolerance(encoder, X), zero_sites=(1,))
    Xn = X.copy()                                                          # a NaN value: NaN from both sides, the other entries untouched
    Xn[9, 0] = np.nan
    eng = engine_cls(0)
    try:
        devn, _ = eng.encode_values(Xn, enc, d=3, kde=encoder)
    finally:
        eng.close()
    keep = np.ones(X.shape, dtype=bool)
    keep[9, 0] = False
    assert np.all(np.isnan(devn[9, 0])) and np.all(np.isnan(encoder(Xn)[9, 0])) and np.array_equal(devn[keep], dev[keep])
    for t in (0, 2):                                                       # outside the grid: exactly the floor, on both sides
        x = X[[2, 3, 6, 7], t]
        floor = np.stack([sum(tab["cvecs"][t][n, i] * x ** i for i in range(3)) for n in range(3)], axis=1) * tab["minx"][t] / tab["scale"][t]
        assert np.abs(dev[[2, 3, 6, 7], t] - floor).max() <= 32 * 3 * EPS * np.abs(floor).max()


def test_the_whole_front_end(engine_cls):
    """Raw data through sigmoid + min-max on the device - norms fitted there - and, for the test set, the out-of-bounds rescale, then
    k_encode_kde: mpst_encode_kde_dataset + get_encoded against transform_data + the host encoder."""
    rng = np.random.default_rng(4)
    N, Nt, T, d = 70, 41, 7, 4
    Xtr = rng.normal(size=(N, T)) + np.linspace(0, 1, T)
    Xte = 1.6 * rng.normal(size=(Nt, T)) + 0.3                             # wider than the training data: out-of-bounds rescales
    enc = mt.sahand_legendre(True)
    opts = mt.MPSOptions(encoding="Custom", d=d)
    Xtr_s, Xte_s, norms, oob = E.transform_data(Xtr, Xte, opts, enc.range)
    assert len(oob) > 0
    _, encoder = E.fit_encoding(enc, Xtr_s, np.zeros(N, dtype=int), opts)
    common = dict(basis=enc, d=d, sigmoid_transform=True, minmax=True, enc_range=enc.range, kde=encoder)
    eng = engine_cls(0)
    try:
        norms_d, _ = eng.encode_dataset(0, Xtr, np.zeros(N, dtype=np.int32), 1, **common)
        tr = eng.get_encoded(0)
        oob_d, _ = eng.encode_dataset(1, Xte, np.zeros(Nt, dtype=np.int32), 1, norms=norms_d, **common)
        te = eng.get_encoded(1)
        te_v, _ = eng.encode_values(Xte, norms=norms_d, rescale_out_of_bounds=True, **common)
    finally:
        eng.close()
    assert [o[0] for o in oob_d] == [o[0] for o in oob]
    assert norms_d.sigmoid == norms.sigmoid and np.allclose(norms_d.minmax, norms.minmax, rtol=0, atol=1e-15)
    for dev, Xs in ((tr, Xtr_s), (te, Xte_s)):
        _compare(dev, encoder(Xs), _tolerance(encoder, Xs) + FRONT_END)
    assert np.array_equal(te, te_v)                                        # mpst_encode_kde_dataset + get_encoded == mpst_encode_kde_values


# ---- fitMPS and imputation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sl_fit():
    """T = 6, d = 3, chi_max = 4, 2 sweeps, 2 classes: host-encoded and device-encoded, shared and left unchanged"""
    rng = np.random.default_rng(23)
    X1, _ = mt.trendy_sine(6, 34, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(6, 34, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(34, dtype=np.int64), np.ones(34, dtype=np.int64)])
    p = rng.permutation(68)
    X, y = X[p], y[p]
    Xtr, ytr, Xte, yte = X[:48], y[:48], X[48:], y[48:]
    enc = mt.sahand_legendre(time_dependent=True)
    opts = mt.MPSOptions(encoding="Custom", d=3, chi_max=4, nsweeps=2, verbosity=-1)
    host = mt.fitMPS(Xtr, ytr, Xte, yte, opts, custom_encoding=enc, device_encode=False)
    dev = mt.fitMPS(Xtr, ytr, Xte, yte, opts, custom_encoding=enc, device_encode=True)
    return Xtr, ytr, Xte, yte, opts, enc, host, dev


def test_fitmps_on_both_routes(sl_fit):
    Xtr, ytr, Xte, yte, opts, enc, (a, info_a, te_a), (b, info_b, te_b) = sl_fit
    assert a.custom_encoding is enc and b.custom_encoding is enc
    _, _, encoder = E.fit_encoding_from_training_data(opts, Xtr, ytr, enc)
    Xtr_s, Xte_s, _, _ = E.transform_data(Xtr, Xte, opts, enc.range)
    for dev, host, Xs, y in ((b.train_data.phi, a.train_data.phi, Xtr_s, ytr), (te_b.phi, te_a.phi, Xte_s, yte)):
        Xs = Xs[np.argsort(y, kind="stable")]
        assert np.array_equal(host, encoder(Xs))
        _compare(dev, host, _tolerance(encoder, Xs) + FRONT_END)
    assert np.array_equal(a.train_data.label_index, b.train_data.label_index)
    assert np.array_equal(a.train_data.original_data, b.train_data.original_data)
    for k in (0, 1):                                                       # before the first sweep and after it; later the trajectories may drift
        la, lb = info_a["train_KL_div"][k], info_b["train_KL_div"][k]
        print(f"training KLD, entry {k}: host-encoded {la:.15g}, device-encoded {lb:.15g}")
        assert np.isfinite(la) and abs(la - lb) <= 1e-9 * abs(la)
    assert np.all(np.isfinite(info_a["train_KL_div"])) and np.all(np.isfinite(info_b["train_KL_div"]))
    pred = mt.classify(a, Xte)                                             # classify re-derives the custom encoding from the model
    assert pred.shape == yte.shape and set(np.unique(pred)) <= {0, 1}


def test_impute_median_against_the_restatement(sl_fit):
    Xtr, ytr, Xte, yte, opts, enc, (trained, _, _), _ = sl_fit
    imp = mt.init_imputation_problem(trained, Xte, yte, dx=1e-3, verbosity=0)
    xr = imp.x_guess_range
    T = Xte.shape[1]
    assert xr.xvals_enc.shape == (T, len(xr.xvals), 3)
    mask = np.zeros(Xte.shape, dtype=bool)
    mask[:, 2:5] = True                                                    # one missing block
    ts, err = mt.impute_dataset(imp, mask, "median")
    assert np.all(np.isfinite(ts)) and np.all(np.isfinite(err[mask])) and np.allclose(ts[~mask], Xte[~mask], rtol=0, atol=1e-9)
    with pytest.raises(NotImplementedError, match="closed-form bases only"):
        mt.impute_dataset(imp, mask, "mean")
    xs_dom, err_dom = mt.impute_dataset(imp, mask, "median", invert_transform=False)
    enc_, norms, raw, full, scaled, oob = mt.imputation._scaled_instances(imp, np.arange(len(Xte)), mask)
    assert enc_ is enc
    phi = imp.encoder(scaled)
    classes = I.expand_label_index(trained.mps)
    lab = [imp.class_map[c] for c in yte.tolist()]
    _accept({"median": (np.where(mask, xs_dom, 0.0), np.where(mask, err_dom, 0.0), "forwards")}, mask.astype(np.uint8), xr.xvals, True,
            lambda i, sites, method: TD.impute(classes[lab[i]], phi[i], sites, xr.xvals, xr.xvals_enc, "median", "forwards", True, None))


def test_fit_batch_and_tune_keep_the_custom_encoding(sl_fit):
    """fit_batch / tune with custom_encoding=: every fold's model carries the encoding, its states are the encoder's fitted to that
    fold's own rows, and the scoring step (classify_many -> classify_states) re-derives it from the model."""
    Xtr, ytr, Xte, yte, opts, enc, _, _ = sl_fit
    o1 = opts.set(nsweeps=1)
    folds = [(np.arange(0, 32), np.arange(32, 48)), (np.arange(16, 48), np.arange(0, 16))]
    out = mt.tuning.fit_batch([(Xtr[tr], ytr[tr], o1, Xtr[va], ytr[va]) for tr, va in folds], custom_encoding=enc)
    for (tr, va), res in zip(folds, out):
        assert res.error is None and res.mps.custom_encoding is enc
        _, _, encoder = E.fit_encoding_from_training_data(o1, Xtr[tr], ytr[tr], enc)
        Xs, _ = E.transform_train_data(Xtr[tr], o1, enc.range)
        assert np.array_equal(res.mps.train_data.phi, encoder(Xs[np.argsort(ytr[tr], kind="stable")]))
    preds, _ = mt.tuning.classify_many([r.mps for r in out], [Xtr[va] for _, va in folds])
    assert all(p.shape == (16,) for p in preds)
    with pytest.raises(ValueError, match="custom"):                        # without it the options alone cannot name the encoding
        mt.tuning.fit_batch([(Xtr[:32], ytr[:32], o1)])
    best, cache = mt.tune(Xtr, ytr, 2, {"eta": [0.01, 0.05]}, objective=mt.MisclassificationRate(), opts0=o1, maxiters=2, verbosity=0,
                          custom_encoding=enc)
    assert set(best) == {"eta"} and len(cache) >= 1 and all(np.isfinite(v) for v in cache.values())


# ---- the C ABI's checks -----------------------------------------------------------------------------------------------------------
def test_kde_abi_errors(engine_cls):
    """Every MPST_ERR_INVALID case of include/mpstime_hip.h; after each, a valid call on the same context succeeds, and a rejected
    data-set call leaves the set that was there."""
    rng = np.random.default_rng(3)
    N, T, d = 6, 2, 3
    Xfit = _bimodal(rng, (40, T))
    Xfit[:, 1] = 1.5                                                       # site 1: zero coefficients
    enc, encoder = _fit(Xfit, d)
    tab = encoder.kde
    X = rng.uniform(-1.0, 1.0, (N, T))
    dp = C.POINTER(C.c_double)
    names = ("lo", "step", "coef", "minx", "scale", "cvecs")
    big = np.zeros((T, 17, 17))                                            # room for the d the call names, whatever it is

    def opts(d_call=d, **over):
        arr = {k: np.array(tab[k], dtype=np.float64, copy=True) for k in names}
        if d_call != d:
            arr["cvecs"] = big.copy()
            arr["cvecs"][:, 0, 0] = 1.0
        for k, v in over.items():
            if k in names and v is not None and not isinstance(v, np.ndarray):
                arr[k][0] = v                                              # a scalar: site 0's entry
        ptr = {k: (None if k in over and over[k] is None else arr[k].ctypes.data_as(dp)) for k in names}
        return L.mpst_kde_opts(over.get("npoints", tab["npoints"]), over.get("per_site", 1), *[ptr[k] for k in names]), arr

    eng = engine_cls(0)
    try:
        out, sec = np.zeros((N, T, 17)), C.c_double()

        def values(kd, d_call=d):
            eo = L.mpst_encode_opts()
            eo.range_a, eo.range_b = 0.0, 1.0
            return eng.lib.mpst_encode_kde_values(eng.ctx, X.ctypes.data_as(dp), N, T, d_call, C.byref(eo), kd, out.ctypes.data_as(C.c_void_p),
                                                  None, C.byref(sec))

        def valid():
            kd, keep = opts()
            assert values(C.byref(kd)) == 0
            assert np.abs(out.ravel()[:N * T * d].reshape(N, T, d) - encoder(X)).max() <= _tolerance(encoder, X).max()

        valid()
        bad = [dict(npoints=2), dict(per_site=2)] + [{k: None} for k in names]
        bad += [{k: v} for k in ("step", "scale", "minx") for v in (0.0, -1.0, np.inf, np.nan)]
        for over in bad:
            kd, keep = opts(**over)
            assert values(C.byref(kd)) == L.MPST_ERR_INVALID, over
            assert eng.lib.mpst_last_error(eng.ctx)
            valid()
        assert values(None) == L.MPST_ERR_INVALID                          # NULL struct
        valid()
        for d_call in (0, 17):
            kd, keep = opts(d_call)
            assert values(C.byref(kd), d_call) == L.MPST_ERR_INVALID, d_call
            valid()
        # a site whose coefficients are all zero may carry anything in its other tables: they are not read
        kd, keep = opts()
        for k in ("step", "scale", "minx", "lo"):
            keep[k][1] = np.nan
        keep["coef"][1] = np.nan
        assert values(C.byref(kd)) == 0 and np.all(out.ravel()[:N * T * d].reshape(N, T, d)[:, 1] == 0.0)
        # the data-set door: a rejected call leaves the context as it was
        lab = np.zeros(N, dtype=np.int32)
        eng.encode_dataset(0, X, lab, 1, basis=enc, d=d, sigmoid_transform=False, minmax=False, enc_range=(0.0, 1.0), kde=encoder)
        before = eng.get_encoded(0)
        assert np.abs(before - encoder(X)).max() <= _tolerance(encoder, X).max()
        with pytest.raises(L.MPSTError) as e:
            eng.encode_dataset(0, X, lab, 1, basis=enc, d=d, sigmoid_transform=False, minmax=False, enc_range=(0.0, 1.0),
                               kde=dict(tab, step=np.array([0.0, 1.0])))
        assert e.value.code == L.MPST_ERR_INVALID
        eo = L.mpst_encode_opts()
        eo.range_a, eo.range_b = 0.0, 1.0
        assert eng.lib.mpst_encode_kde_dataset(eng.ctx, 0, X.ctypes.data_as(dp), lab.ctypes.data_as(C.POINTER(C.c_int32)), N, T, d, 1, C.byref(eo), None,
                                               None, None, C.byref(sec)) == L.MPST_ERR_INVALID
        assert np.array_equal(eng.get_encoded(0), before)
        with pytest.raises(ValueError, match="shape"):                      # the binding checks what the library cannot: the lengths
            eng.encode_values(X, enc, d=d, kde=dict(tab, coef=tab["coef"][:, :-1]))
        with pytest.raises(L.MPSTError) as e:                               # without its tables the encoding has no device route
            eng.encode_values(X, enc, d=d)
        assert e.value.code == L.MPST_ERR_UNSUPPORTED
    finally:
        eng.close()
