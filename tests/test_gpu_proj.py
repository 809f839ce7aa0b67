"""The projected bases on the device: k_encode_proj against the host encoder element by element (alone and behind the whole front
end), fitMPS with the encodings on both routes, imputation on the trained model against tests/impute_td_ref.py, and the checks of
the C ABI.

The tolerance of an encoded value.  Host and device evaluate the same expressions from the same order lists - the Bonnet recursion,
the factor sqrt((2k + 1) / 2), sincospi(f x) - and differ only where a square root, a division or a sine rounds differently.  How
much float64 arithmetic itself loses on a test's inputs is measured, not assumed: e_ref is the largest difference between the
float64 and the longdouble restatement of tests/proj_ref.py over the states of that test.  The bound per entry is
    4 e_ref + 16 eps max(1, |state|):
the device must not be more than a few times further from the truth than float64 arithmetic is by itself.
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
from tests import proj_ref as PR
from tests.test_gpu_split import _accept

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FRONT_END = 1e-13


def _bimodal(rng, N, T):
    pick = rng.random((N, T)) < 0.45
    X = np.where(pick, rng.normal(-0.45, 0.18, (N, T)), rng.normal(0.4, 0.22, (N, T)))
    return np.clip(X + np.linspace(-0.25, 0.25, T), -1.0, 1.0)


def _encoding(kind):
    return mt.fourier(project=True) if kind == "fourier" else mt.legendre(norm=kind == "legendre_norm", project=True)


def _opts(kind, d, **kw):
    return mt.MPSOptions(encoding="Custom", d=d, dtype="ComplexF64" if kind == "fourier" else "Float64", **kw)


def _fit(kind, X, d):
    enc = _encoding(kind)
    return enc, E.FittedEncoder(enc, d, enc.init(X, None, opts=_opts(kind, d)))


def _e_ref(kind, encoder, X):
    """(e_ref, float64 restatement) of the module docstring for the states of X"""
    fam = "fourier" if kind == "fourier" else "legendre"
    return PR.float64_loss(X, encoder.args[0].tolist(), fam, encoder.d, kind == "legendre_norm")


def _compare(dev, host, e_ref, extra=0.0):
    assert dev.shape == host.shape and dev.dtype == host.dtype
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(dev))
    tol = 4 * e_ref + 16 * EPS * np.maximum(1.0, np.abs(host)) + extra
    print(f"largest |device - host| {np.abs(dev - host).max():.3e}, e_ref {e_ref:.3e}, largest |state| {np.abs(host).max():.3e}")
    assert np.all(np.abs(dev - host) <= tol)


def _values(engine_cls, X, enc, encoder, table=None):
    eng = engine_cls(0)
    try:
        dev, sec = eng.encode_values(X, enc, d=encoder.d, orders=encoder)
        dev2, _ = eng.encode_values(X, enc, d=encoder.d, orders=encoder.orders if table is None else table)
    finally:
        eng.close()
    assert sec > 0
    return dev, dev2


@pytest.mark.parametrize("kind,N,T,d", [("legendre", 37, 5, 4), ("legendre_norm", 37, 5, 4), ("legendre", 300, 3, 2), ("legendre_norm", 300, 3, 2),
                                        ("legendre", 33, 4, 16), ("legendre_norm", 33, 4, 16), ("fourier", 37, 5, 4), ("fourier", 64, 1, 5)])
def test_device_encoder_against_the_host_encoder(engine_cls, kind, N, T, d):
    """encode_values without transforms: host and device see the same x bit for bit.  (300, 3) leaves the last block partly empty
    and lets a wave straddle two sites; d = 16 is the limit, and there the last member of every site's selection is replaced by
    position 112 = 7 * 16, the largest the fit can return: the recursion runs to order 112.  Rows 0 and 1 are -1 and +1."""
    rng = np.random.default_rng(1000 * N + d)
    enc, encoder = _fit(kind, _bimodal(rng, 80, T), d)
    if d == 16:
        encoder.args[0][:, -1] = 7 * 16
        assert encoder.orders["orders"].max() == 112
    X = rng.uniform(-1.0, 1.0, (N, T))
    X[0], X[1] = -1.0, 1.0
    host = encoder(X)
    dev, dev2 = _values(engine_cls, X, enc, encoder)
    assert np.array_equal(dev, dev2)                                       # orders=encoder and orders=dict: identical bits
    e_ref, want = _e_ref(kind, encoder, X)
    assert np.abs(host - want).max() <= 4 * e_ref + 16 * EPS * max(1.0, np.abs(want).max())
    _compare(dev, host, e_ref)


def test_a_hand_made_order_list_and_a_nan_value(engine_cls):
    """Repeated and descending orders, order 0 (which no fit selects) and a one-order site; then a NaN value: NaN from both sides,
    every other entry untouched."""
    ds = np.array([[5, 3, 3, 1], [2, 2, 2, 2], [7, 6, 5, 4], [1, 28, 1, 28]])
    enc = mt.legendre(norm=True, project=True)
    encoder = E.FittedEncoder(enc, 4, [ds])
    rng = np.random.default_rng(12)
    X = rng.uniform(-1.0, 1.0, (70, 4))
    X[0], X[1] = -1.0, 1.0
    host = encoder(X)
    assert np.array_equal(host[:, 0, 1], host[:, 0, 2]) and np.array_equal(host[:, 3, 0], host[:, 3, 2])
    table = dict(encoder.orders)
    dev, dev2 = _values(engine_cls, X, enc, encoder, table)
    assert np.array_equal(dev, dev2)
    e_ref, _ = _e_ref("legendre_norm", encoder, X)
    _compare(dev, host, e_ref)
    assert np.array_equal(dev[:, 0, 1], dev[:, 0, 2]) and np.array_equal(dev[:, 1, 0], dev[:, 1, 3])
    zero = dict(table, orders=np.array([[0, 3, 0, 1]] * 4, dtype=np.int32), basis="Legendre_No_Norm")
    eng = engine_cls(0)
    try:
        dev0, _ = eng.encode_values(X, enc, d=4, orders=zero)
        Xn = X.copy()
        Xn[9, 2] = np.nan
        devn, _ = eng.encode_values(Xn, enc, d=4, orders=encoder)
        fdev, _ = eng.encode_values(Xn, mt.fourier(project=True), d=4, orders=dict(basis="Fourier", orders=np.array([[0, 2, -2, 1]] * 4), inv_norm=None))
    finally:
        eng.close()
    want0 = E.legendre_encode_no_norm(X, 4)[..., [0, 3, 0, 1]]
    assert np.abs(dev0 - want0).max() <= 16 * EPS * np.abs(want0).max() and np.abs(dev0[..., 0] - np.sqrt(0.5)).max() <= EPS
    keep = np.ones(X.shape, dtype=bool)
    keep[9, 2] = False
    assert np.all(np.isnan(devn[9, 2])) and np.all(np.isnan(encoder(Xn)[9, 2])) and np.array_equal(devn[keep], dev[keep])
    assert fdev.dtype == np.complex128 and np.all(np.isnan(fdev[9, 2, 1:])) and np.all(np.isfinite(fdev[keep]))


@pytest.mark.parametrize("kind", ["legendre_norm", "fourier"])
def test_the_whole_front_end(engine_cls, kind):
    """Raw data through sigmoid + min-max on the device - norms fitted there - and, for the test set, the out-of-bounds rescale, then
    k_encode_proj: mpst_encode_proj_dataset + get_encoded against transform_data + the host encoder."""
    rng = np.random.default_rng(4)
    N, Nt, T, d = 70, 41, 7, 4
    Xtr = rng.normal(size=(N, T)) + np.linspace(0, 1, T)
    Xte = 1.6 * rng.normal(size=(Nt, T)) + 0.3                             # wider than the training data: out-of-bounds rescales
    enc = _encoding(kind)
    opts = _opts(kind, d)
    Xtr_s, Xte_s, norms, oob = E.transform_data(Xtr, Xte, opts, enc.range)
    assert len(oob) > 0
    _, encoder = E.fit_encoding(enc, Xtr_s, np.zeros(N, dtype=int), opts)
    common = dict(basis=enc, d=d, sigmoid_transform=True, minmax=True, enc_range=enc.range, orders=encoder)
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
        _compare(dev, encoder(Xs), _e_ref(kind, encoder, Xs)[0], FRONT_END)
    assert np.array_equal(te, te_v)                                        # mpst_encode_proj_dataset + get_encoded == mpst_encode_proj_values


# ---- fitMPS and imputation -------------------------------------------------------------------------------------------------------
def _data():
    rng = np.random.default_rng(23)
    X1, _ = mt.trendy_sine(6, 34, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(6, 34, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(34, dtype=np.int64), np.ones(34, dtype=np.int64)])
    p = rng.permutation(68)
    X, y = X[p], y[p]
    return X[:48], y[:48], X[48:], y[48:]


@pytest.fixture(scope="module")
def proj_fits():
    """T = 6, d = 3, chi_max = 4, one sweep, 2 classes: host-encoded and device-encoded, one pair of fits per family, shared by the
    tests below and left unchanged"""
    return {kind: _both_routes(kind) for kind in ("legendre", "fourier")}


@pytest.fixture(scope="module", params=["legendre", "fourier"])
def proj_fit(request, proj_fits):
    return proj_fits[request.param]


@pytest.fixture(scope="module")
def legendre_fit(proj_fits):
    return proj_fits["legendre"]


def _both_routes(kind):
    Xtr, ytr, Xte, yte = _data()
    enc = _encoding(kind)
    opts = _opts(kind, 3, chi_max=4, nsweeps=1, verbosity=-1)
    host = mt.fitMPS(Xtr, ytr, Xte, yte, opts, custom_encoding=enc, device_encode=False)
    dev = mt.fitMPS(Xtr, ytr, Xte, yte, opts, custom_encoding=enc, device_encode=True)
    return kind, Xtr, ytr, Xte, yte, opts, enc, host, dev


def test_fitmps_on_both_routes(proj_fit):
    kind, Xtr, ytr, Xte, yte, opts, enc, (a, info_a, te_a), (b, info_b, te_b) = proj_fit
    assert a.custom_encoding is enc and b.custom_encoding is enc
    assert a.mps[0].dtype == b.mps[0].dtype == (np.complex128 if kind == "fourier" else np.float64)
    _, _, encoder = E.fit_encoding_from_training_data(opts, Xtr, ytr, enc)
    Xtr_s, Xte_s, _, _ = E.transform_data(Xtr, Xte, opts, enc.range)
    for dev, host, Xs, y in ((b.train_data.phi, a.train_data.phi, Xtr_s, ytr), (te_b.phi, te_a.phi, Xte_s, yte)):
        Xs = Xs[np.argsort(y, kind="stable")]
        assert np.array_equal(host, encoder(Xs))
        _compare(dev, host, _e_ref(kind, encoder, Xs)[0], FRONT_END)
    assert np.array_equal(a.train_data.label_index, b.train_data.label_index)
    assert np.array_equal(a.train_data.original_data, b.train_data.original_data)
    assert np.all(np.isfinite(info_a["train_KL_div"])) and np.all(np.isfinite(info_b["train_KL_div"]))
    for k in (0, 1):                                                       # before the sweep and after it
        la, lb = info_a["train_KL_div"][k], info_b["train_KL_div"][k]
        print(f"training KLD, entry {k}: host-encoded {la:.15g}, device-encoded {lb:.15g}")
        assert np.isfinite(la) and abs(la - lb) <= 1e-9 * abs(la)
    pa, pb = mt.classify(a, Xte), mt.classify(b, Xte)                      # classify re-derives the custom encoding from the model
    assert pa.shape == yte.shape and set(np.unique(pa)) <= {0, 1} and np.array_equal(mt.classify(a, Xte), pa)
    assert pb.shape == yte.shape and set(np.unique(pb)) <= {0, 1}
    assert np.array_equal(pa, pb)                                          # the two routes' MODELS give equal labels
    assert np.array_equal(mt.classify(a, te_a), mt.classify(a, te_b))      # equal labels from the two routes' states


def test_impute_median_against_the_restatement(legendre_fit):
    kind, Xtr, ytr, Xte, yte, opts, enc, (trained, _, _), _ = legendre_fit
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


def test_fit_batch_and_tune_keep_the_custom_encoding(legendre_fit):
    kind, Xtr, ytr, Xte, yte, opts, enc, _, _ = legendre_fit
    folds = [(np.arange(0, 32), np.arange(32, 48)), (np.arange(16, 48), np.arange(0, 16))]
    out = mt.tuning.fit_batch([(Xtr[tr], ytr[tr], opts, Xtr[va], ytr[va]) for tr, va in folds], custom_encoding=enc)
    for (tr, va), res in zip(folds, out):
        assert res.error is None and res.mps.custom_encoding is enc
        _, _, encoder = E.fit_encoding_from_training_data(opts, Xtr[tr], ytr[tr], enc)
        Xs, _ = E.transform_train_data(Xtr[tr], opts, enc.range)
        assert np.array_equal(res.mps.train_data.phi, encoder(Xs[np.argsort(ytr[tr], kind="stable")]))
    preds, _ = mt.tuning.classify_many([r.mps for r in out], [Xtr[va] for _, va in folds])
    assert all(p.shape == (16,) for p in preds)
    best, cache = mt.tune(Xtr, ytr, 2, {"eta": [0.01, 0.05]}, objective=mt.MisclassificationRate(), opts0=opts, maxiters=2, verbosity=0,
                          custom_encoding=enc)
    assert set(best) == {"eta"} and len(cache) >= 1 and all(np.isfinite(v) for v in cache.values())


# ---- the C ABI's checks -----------------------------------------------------------------------------------------------------------
def test_proj_abi_errors(engine_cls):
    """Every MPST_ERR_INVALID case of include/mpstime_hip.h; after each, a valid call on the same context succeeds, and a rejected
    data-set call leaves the set that was there.  Every case is rejected on the host before anything is launched."""
    rng = np.random.default_rng(3)
    N, T, d = 6, 2, 3
    ds = np.array([[1, 3, 5], [2, 1, 4]])
    enc = mt.legendre(norm=True, project=True)
    encoder = E.FittedEncoder(enc, d, [ds])
    tab = encoder.orders
    X = rng.uniform(-1.0, 1.0, (N, T))
    host = encoder(X)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    LN, LNN, F = L.BASIS["Legendre_Norm"], L.BASIS["Legendre_No_Norm"], L.BASIS["Fourier"]

    def opts(basis=LN, orders=tab["orders"], inv=tab["inv_norm"], max_order=5, d_call=d):
        o = None if orders is None else np.ascontiguousarray(np.resize(np.asarray(orders, dtype=np.int32), (T, d_call)))
        v = None if inv is None else np.ascontiguousarray(inv, dtype=np.float64)
        pj = L.mpst_proj_opts(basis, None if o is None else o.ctypes.data_as(ip), None if v is None else v.ctypes.data_as(dp), max_order)
        return pj, (o, v)

    eng = engine_cls(0)
    try:
        out, sec = np.zeros((N, T, 2 * 17)), C.c_double()

        def values(pj, d_call=d):
            eo = L.mpst_encode_opts()
            eo.range_a, eo.range_b = 0.0, 1.0
            return eng.lib.mpst_encode_proj_values(eng.ctx, X.ctypes.data_as(dp), N, T, d_call, C.byref(eo), pj, out.ctypes.data_as(C.c_void_p),
                                                   None, C.byref(sec))

        def valid():
            pj, keep = opts()
            assert values(C.byref(pj)) == 0
            assert np.abs(out.ravel()[:N * T * d].reshape(N, T, d) - host).max() <= 16 * EPS * np.abs(host).max()

        valid()
        bad = [dict(orders=[[1, 3, 6], [2, 1, 4]]),                        # an order above max_order
               dict(orders=[[1, -1, 5], [2, 1, 4]]),                       # a negative Legendre order
               dict(max_order=4),                                          # max_order too small for the table
               dict(max_order=-1), dict(max_order=7 * 16 + 1),
               dict(basis=F, orders=[[0, 81, -1], [2, 1, 4]], max_order=81),   # Fourier: above 5 * 16
               dict(basis=F, orders=[[0, 3, -4], [2, 1, 3]], max_order=3),     # Fourier: |f| above max_order
               dict(orders=None),                                          # NULL table
               dict(inv=None),                                             # the normalised basis without its norms
               dict(inv=[0.3, 0.0]), dict(inv=[-1.0, 0.3]), dict(inv=[np.inf, 0.3]), dict(inv=[0.3, np.nan]),
               dict(basis=L.BASIS["Stoudenmire"]), dict(basis=L.BASIS["Uniform"]), dict(basis=-1), dict(basis=6)]
        for over in bad:
            pj, keep = opts(**over)
            assert values(C.byref(pj)) == L.MPST_ERR_INVALID, over
            assert eng.lib.mpst_last_error(eng.ctx)
            valid()
        assert values(None) == L.MPST_ERR_INVALID                          # NULL struct
        valid()
        for d_call in (0, 17):
            pj, keep = opts(basis=LNN, d_call=d_call)
            assert values(C.byref(pj), d_call) == L.MPST_ERR_INVALID, d_call
            valid()
        # what is allowed: no norms for the other two families, the limits themselves
        pj, keep = opts(basis=LNN, inv=None)
        assert values(C.byref(pj)) == 0
        pj, keep = opts(basis=F, orders=[[0, 80, -80], [2, 1, -1]], inv=None, max_order=80)
        assert values(C.byref(pj)) == 0
        pj, keep = opts(basis=LNN, orders=[[112, 0, 5], [2, 1, 4]], inv=None, max_order=112)
        assert values(C.byref(pj)) == 0
        # the data-set door: a rejected call leaves the context as it was
        lab = np.zeros(N, dtype=np.int32)
        kw = dict(basis=enc, d=d, sigmoid_transform=False, minmax=False, enc_range=(0.0, 1.0))
        eng.encode_dataset(0, X, lab, 1, orders=encoder, **kw)
        before = eng.get_encoded(0)
        assert np.abs(before - host).max() <= 16 * EPS * np.abs(host).max()
        with pytest.raises(L.MPSTError) as e:
            eng.encode_dataset(0, X, lab, 1, orders=dict(tab, orders=np.array([[1, 3, 113], [2, 1, 4]])), **kw)
        assert e.value.code == L.MPST_ERR_INVALID
        eo = L.mpst_encode_opts()
        eo.range_a, eo.range_b = 0.0, 1.0
        assert eng.lib.mpst_encode_proj_dataset(eng.ctx, 0, X.ctypes.data_as(dp), lab.ctypes.data_as(ip), N, T, d, 1, C.byref(eo), None,
                                                None, None, C.byref(sec)) == L.MPST_ERR_INVALID
        assert np.array_equal(eng.get_encoded(0), before)
        with pytest.raises(ValueError, match="shape"):                      # the binding checks what the library cannot: T and d
            eng.encode_values(X, enc, d=d, orders=dict(tab, orders=tab["orders"][:1]))
        with pytest.raises(ValueError, match="shape"):
            eng.encode_values(X, enc, d=d, orders=dict(tab, inv_norm=tab["inv_norm"][:1]))
        with pytest.raises(ValueError, match="one of them"):
            eng.encode_values(X, enc, d=d, orders=encoder, kde=encoder)
        with pytest.raises(L.MPSTError) as e:                               # without its tables the encoding has no device route
            eng.encode_values(X, enc, d=d)
        assert e.value.code == L.MPST_ERR_UNSUPPORTED
        cx = mt.fourier(project=True)                                       # a complex basis into a context fixed to a real type
        eng.set_dtype(np.float64)
        with pytest.raises(L.MPSTError, match="the MPS is real"):
            eng.encode_dataset(0, X, lab, 1, basis=cx, d=d, sigmoid_transform=False, minmax=False, enc_range=(0.0, 1.0),
                               orders=dict(basis="Fourier", orders=np.array([[0, 1, -1], [0, 2, 1]]), inv_norm=None))
    finally:
        eng.close()
