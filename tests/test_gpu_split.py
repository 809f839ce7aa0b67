"""Split bases and per-site grid tables on the device: k_encode_split against the host encoder (values and support), the ABI's
checks, fitMPS / classify with a histogram-split encoding, and the imputation engine with one grid table per site
(mpst_impute_opts.grid_per_site) against tests/impute_td_ref.py - the restatement of impute_at! that indexes the table with the site."""
import ctypes as C

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import _lib as L
from mpstime_jl_amd import encodings as E
from oracle import impute_numpy as I
from oracle import ref_numpy as R
from tests import impute_td_ref as TD

pytestmark = pytest.mark.gpu

# name, d, aux_basis_dim, tolerance of the auxiliary basis (tests/test_gpu_encode.py)
ENC_CASES = {"hist_legendre": ("hist_split_legendre", 6, 2, 1e-13), "hist_fourier": ("hist_split_fourier", 6, 2, 1e-14),
             "unif_sahand": ("unif_split_sahand", 8, 2, 1e-12), "unif_uniform": ("unif_split_uniform", 4, 2, 1e-13),
             "hist_stoudenmire": ("hist_split_stoudenmire", 4, 2, 1e-12)}


def _bins_hit(phi, aux):
    """which bins of every state carry weight, (..., nbins): the bin choice, on which host and device must agree exactly.  (Entry by
    entry the supports may differ where an auxiliary state has a zero: cos(pi / 2) is 6e-17 in NumPy and 0 from the device's cospi.)"""
    return (phi.reshape(phi.shape[:-1] + (-1, aux)) != 0).any(axis=-1)


def _fit(name, d, aux, Xfit):
    opts = mt.MPSOptions(encoding=name, d=d, aux_basis_dim=aux)
    enc = E.opts_encoding(opts)
    _, encoder = E.fit_encoding(enc, Xfit, np.zeros(len(Xfit), dtype=int), opts)
    return enc, encoder


@pytest.mark.parametrize("case", sorted(ENC_CASES))
def test_device_split_encoder_identity_preprocessing(engine_cls, case):
    """encode_values without transforms: host and device see the same x bit for bit, so the bin choice - the support of the state -
    must be identical, edges included; values to the auxiliary basis' tolerance."""
    name, d, aux, tol = ENC_CASES[case]
    enc0 = E.model_encoding(name)
    a, b = enc0.range
    rng = np.random.default_rng(17)
    enc, encoder = _fit(name, d, aux, rng.uniform(a, b, (40, 7)))
    bins = encoder.bins
    nb = d // aux
    X = rng.uniform(a, b, (29, 7))
    for col in (0, 6):                                  # interior and outer edges of sites 0 and 6 as values
        X[:nb + 1, col] = bins[col] if bins.ndim == 2 else bins
    host = encoder(X)
    eng = engine_cls(0)
    try:
        dev, _ = eng.encode_values(X, name, d=d, bins=bins)
        dev2, _ = eng.encode_values(X, enc, d=d, bins=bins)            # by Encoding
    finally:
        eng.close()
    assert dev.shape == host.shape == (29, 7, d) and dev.dtype == host.dtype
    assert np.array_equal(_bins_hit(dev, aux), _bins_hit(host, aux))
    assert np.abs(dev - host).max() <= tol
    assert np.array_equal(dev, dev2)
    # an interior edge: half of the auxiliary state in both neighbours
    k = 1
    assert np.count_nonzero(dev[k, 0]) <= 2 * aux and np.any(dev[k, 0, :aux] != 0) and np.any(dev[k, 0, aux:2 * aux] != 0)


@pytest.mark.parametrize("name,d,aux", [("hist_split_legendre", 6, 2), ("hist_split_fourier", 6, 3), ("unif_split_legendre_norm", 8, 2)])
def test_device_split_encoder_behind_the_preprocessing(engine_cls, name, d, aux):
    """Training and test sets through sigmoid + min-max + out-of-bounds rescale on the device, bins fitted on the host: no value is
    excluded - none lies within 1e-9 of an interior edge (asserted) -, the support is the host's, values within 1e-12."""
    rng = np.random.default_rng(4)
    Xtr = rng.normal(size=(64, 10)) + np.linspace(0, 1, 10)
    Xte = 1.6 * rng.normal(size=(40, 10)) + 0.3                     # wider than the training data: out-of-bounds rescales
    opts = mt.MPSOptions(encoding=name, d=d, aux_basis_dim=aux)
    enc = E.opts_encoding(opts)
    Xtr_s, Xte_s, norms, oob = E.transform_data(Xtr, Xte, opts, enc.range)
    assert len(oob) > 0
    _, encoder = E.fit_encoding(enc, Xtr_s, np.zeros(64, dtype=int), opts)
    bins = encoder.bins
    for Xs in (Xtr_s, Xte_s):
        inner = (bins[:, 1:-1] if bins.ndim == 2 else np.broadcast_to(bins[1:-1], (10, len(bins) - 2)))
        assert np.abs(Xs[:, :, None] - inner[None]).min() > 1e-9
    common = dict(d=d, sigmoid_transform=True, minmax=True, enc_range=enc.range, bins=bins)
    eng = engine_cls(0)
    try:
        if enc.iscomplex:
            eng.set_dtype(np.complex128)
        lab = np.zeros(64, dtype=np.int32)
        norms_d, _ = eng.encode_dataset(0, Xtr, lab, 1, basis=name, **common)
        tr = eng.get_encoded(0)
        oob_d, _ = eng.encode_dataset(1, Xte, np.zeros(40, dtype=np.int32), 1, basis=name, norms=norms_d, **common)
        te = eng.get_encoded(1)
        te_v, _ = eng.encode_values(Xte, name, norms=norms_d, rescale_out_of_bounds=True, **common)
    finally:
        eng.close()
    assert [o[0] for o in oob_d] == [o[0] for o in oob]
    for dev, Xs in ((tr, Xtr_s), (te, Xte_s)):
        host = encoder(Xs)
        assert np.array_equal(_bins_hit(dev, aux), _bins_hit(host, aux))
        assert np.abs(dev - host).max() <= 1e-12
    assert np.array_equal(te, te_v)                                   # mpst_encode_split_dataset + get_encoded == encode_split_values


def test_split_abi_errors(engine_cls):
    eng = engine_cls(0)
    try:
        X = np.zeros((3, 2))
        up = np.array([-1.0, 0.0, 1.0])
        with pytest.raises(L.MPSTError) as e:                           # d != nbins * aux_dim
            eng.encode_values(X, "unif_split_legendre", d=5, bins=up)
        assert e.value.code == L.MPST_ERR_INVALID
        with pytest.raises(L.MPSTError) as e:                           # decreasing edges
            eng.encode_values(X, "unif_split_legendre", d=4, bins=np.array([-1.0, 0.5, 0.0]))
        assert e.value.code == L.MPST_ERR_INVALID
        with pytest.raises(L.MPSTError) as e:                           # Stoudenmire needs aux_dim 2
            eng.encode_values(X, "unif_split_stoudenmire", d=6, bins=np.array([0.0, 0.5, 1.0]))
        assert e.value.code == L.MPST_ERR_UNSUPPORTED
        with pytest.raises(L.MPSTError) as e:                           # Sahand needs an even aux_dim
            eng.encode_values(X, "unif_split_sahand", d=6, bins=np.array([0.0, 0.5, 1.0]))
        assert e.value.code == L.MPST_ERR_UNSUPPORTED
        eo, out, sec = L.mpst_encode_opts(), np.zeros((3, 2, 4)), C.c_double()
        eo.range_a, eo.range_b = 0.0, 1.0
        dp = C.POINTER(C.c_double)
        call = lambda sp: eng.lib.mpst_encode_split_values(eng.ctx, X.ctypes.data_as(dp), 3, 2, 4, C.byref(eo), sp,
                                                           out.ctypes.data_as(C.c_void_p), None, C.byref(sec))
        assert call(C.byref(L.mpst_split_opts(1, 2, 2, 0, None))) == L.MPST_ERR_INVALID          # NULL bins
        assert call(None) == L.MPST_ERR_INVALID                                                  # NULL options
        assert call(C.byref(L.mpst_split_opts(1, 2, 0, 0, up.ctypes.data_as(dp)))) == L.MPST_ERR_INVALID   # nbins < 1
        assert call(C.byref(L.mpst_split_opts(9, 2, 2, 0, up.ctypes.data_as(dp)))) == L.MPST_ERR_UNSUPPORTED
        assert call(C.byref(L.mpst_split_opts(1, 2, 2, 0, up.ctypes.data_as(dp)))) == 0
    finally:
        eng.close()


# ---- fitMPS / classify with a histogram-split encoding ----------------------------------------------------------------------------
def _fit_data():
    rng = np.random.default_rng(23)
    X1, _ = mt.trendy_sine(10, 34, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(10, 34, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(34, dtype=np.int64), np.ones(34, dtype=np.int64)])
    p = rng.permutation(68)
    X, y = X[p], y[p]
    return X[:48], y[:48], X[48:], y[48:]


@pytest.fixture(scope="module")
def hist_fit():
    Xtr, ytr, Xte, yte = _fit_data()
    opts = mt.MPSOptions(encoding="hist_split_legendre", d=6, aux_basis_dim=2, chi_max=8, nsweeps=2, verbosity=-1)
    trained, info, te = mt.fitMPS(Xtr, ytr, Xte, yte, opts)
    return Xtr, ytr, Xte, yte, opts, trained, info, te


def test_fitmps_hist_split_host_and_device_encoding(hist_fit):
    """device_encode=True gives the states and the first logged losses of the host-encoded fit (the tolerances of
    test_fitmps_with_device_encoding_matches_host_encoding), the product states are the fitted host encoder's, and classify on raw data
    returns the argmax of the oracle's overlaps."""
    Xtr, ytr, Xte, yte, opts, trained, info, te = hist_fit
    b, info_b, te_b = mt.fitMPS(Xtr, ytr, Xte, yte, opts, device_encode=True)
    assert np.array_equal(_bins_hit(trained.train_data.phi, 2), _bins_hit(b.train_data.phi, 2)) and np.array_equal(_bins_hit(te.phi, 2), _bins_hit(te_b.phi, 2))
    assert np.max(np.abs(trained.train_data.phi - b.train_data.phi)) < 1e-13
    assert np.max(np.abs(te.phi - te_b.phi)) < 1e-13
    assert abs(info["train_KL_div"][0] - info_b["train_KL_div"][0]) < 1e-10
    assert abs(info["test_KL_div"][0] - info_b["test_KL_div"][0]) < 1e-10
    # the product states are the host encoder's, site by site, and sum to the auxiliary norm of one bin
    enc, _, encoder = E.fit_encoding_from_training_data(opts, Xtr, ytr)
    assert encoder.bins.shape == (10, 4)
    Xs, _ = E.transform_train_data(Xtr, opts, enc.range)
    order = np.argsort(ytr, kind="stable")
    assert np.array_equal(trained.train_data.phi, encoder(Xs[order]))
    # classify(raw) = argmax of the oracle's overlaps on the states classify_states builds
    states = mt.training.classify_states(trained, Xte)
    assert np.array_equal(states.phi != 0, encoder(E.transform_test_data(Xte, E.transform_train_data(Xtr, opts, enc.range)[1], opts, enc.range)[0]) != 0)
    yhat = R.contract_mps(trained.mps, states.phi)
    pred = mt.classify(trained, Xte)
    assert np.array_equal(pred, np.unique(ytr)[np.argmax(np.abs(yhat) ** 2, axis=1)])
    assert np.all(np.isfinite(info["train_KL_div"])) and info["train_KL_div"][-1] < info["train_KL_div"][0]


def test_hist_split_states_train_like_the_oracle(hist_fit, engine_cls):
    """Every bond update of the two sweeps on the host-encoded hist-split states against the oracle fed the same states, teacher-forced
    (tests/helpers.py: free-running fits diverge chaotically), with that helper's tolerances as the other fits use them."""
    from oracle.c_oracle import COracle
    from tests.helpers import teacher_forced_sweep
    Xtr, ytr, Xte, yte, opts, trained, info, te = hist_fit
    td = trained.train_data
    T = td.phi.shape[1]
    W0 = mt.generate_startingMPS(opts.chi_init, T, opts.d, 2, opts.init_rng)
    co = COracle(W0, td.phi, td.label_index, td.class_distribution, opts.chi_max, eta=opts.eta, rebuild_caches=False)
    co.build_caches()
    eng = engine_cls(0)
    try:
        eng.set_options(chi_max=opts.chi_max, eta=opts.eta, cutoff=opts.cutoff)
        eng.set_dataset(0, td.phi, td.label_index, 2)
        for sweep in range(2):
            worst, flips = teacher_forced_sweep(eng, co, td.phi, T, overlap_every=3)
            assert worst["loss"] < 1e-10 and worst["grad"] < 1e-8 and worst["S"] < 1e-9 and worst["overlap"] < 1e-8, (sweep, worst)
            assert flips <= 2
    finally:
        eng.close()


# ---- per-site grid tables in the imputation engine --------------------------------------------------------------------------------
def _td_problem(N, T, d, aux, chi, C, seed, ngrid, cx):
    """_problem of tests/test_gpu_impute_model.py with a histogram-split encoding: random normalised MPS, ragged masks, per-site bins
    from a separate sample, the grid table tabulated per site on the host."""
    rng = np.random.default_rng(seed)
    if cx:
        W = [a + 1j * b for a, b in zip(R.random_mps(T, d, chi, C, rng), R.random_mps(T, d, chi, C, rng))]
    else:
        W = R.random_mps(T, d, chi, C, rng)
    xs = -1.0 + (2.0 / (ngrid - 1)) * np.arange(ngrid)
    _, encoder = _fit("hist_split_fourier" if cx else "hist_split_legendre", d, aux, rng.uniform(-1, 1, (40, T)))
    X = rng.uniform(-0.95, 0.95, (N, T))
    y = rng.integers(0, C, N).astype(np.int32)
    m = (rng.uniform(size=(N, T)) < 0.4).astype(np.uint8)
    m[0] = 1
    m[1] = 0
    m[2, :] = 0
    m[2, T // 2] = 1
    dt = np.complex128 if cx else np.float64
    return W, xs, np.ascontiguousarray(encoder.table(xs, T), dtype=dt), X, y, np.ascontiguousarray(encoder(X), dtype=dt), m, rng


def _td_oracle(classes, phi, y, i, sites, xs, gp, method, order, u):
    ui = None if u is None else (u[i, sites] if order == "forwards" else u[i, sites][::-1])
    if method == "its_reject":
        return TD.impute(classes[y[i]], phi[i], sites, xs, gp, "quantile", order, True, ui, rejection_threshold=1.0, max_trials=3)
    if method == "quantile":
        return TD.impute(classes[y[i]], phi[i], sites, xs, gp, "quantile", order, False, ui[:, :1])
    return TD.impute(classes[y[i]], phi[i], sites, xs, gp, method, order, method == "median", None)


def _accept(runs, m, xs, f64, oracle):
    """The acceptance rule of tests/test_gpu_impute_batched_oracle.py, unchanged: equal within 1e-12, or the FIRST differing site of an
    instance off by at most one grid step (four: fp32 chain), at most 3 of the instances flipping (N // 2: fp32), WMAD within dx where
    nothing flipped."""
    N = m.shape[0]
    dx = xs[1] - xs[0]
    for method, (xg, eg, order) in runs.items():
        assert np.all(xg[m == 0] == 0.0) and np.all(np.isfinite(xg))
        flips = 0
        for i in range(N):
            sites = np.flatnonzero(m[i])
            if len(sites) == 0:
                continue
            xo, eo = oracle(i, sites, method)
            diff = np.abs(xg[i, sites] - xo)
            if order == "backwards":
                diff = diff[::-1]
            if np.any(diff > 1e-12):
                first = int(np.argmax(diff > 1e-12))
                assert diff[first] <= (1.0000001 if f64 else 4.0000001) * dx, (method, i, first, diff[first] / dx)
                assert np.all(diff[:first] <= 1e-12)
                flips += 1
            elif f64 and method in ("median", "its_reject") and eg is not None:
                assert np.abs(eg[i, sites] - eo).max() <= dx * 1.0000001, (method, i)
        assert flips <= (3 if f64 else N // 2), (method, flips)


@pytest.mark.parametrize("order", ["forwards", "backwards"])
@pytest.mark.parametrize("compute", ["f64", "f32"])
@pytest.mark.parametrize("cx,chi", [(False, 12), (True, 10)], ids=["hist_legendre_d6", "hist_fourier_d6"])
def test_per_site_table_against_the_restatement(engine_cls, compute, cx, chi, order):
    N, T, C, d, aux = 21, 10, 3, 6, 2
    W, xs, gp, X, y, phi, m, rng = _td_problem(N, T, d, aux, chi, C, seed=6000 + chi, ngrid=2001, cx=cx)
    assert gp.shape == (T, 2001, d)
    u = rng.uniform(0.02, 0.98, (N, T, 3))
    o = ["forwards", "backwards"].index(order)
    eng = engine_cls(0)
    try:
        run = lambda *a, **k: eng.impute_model(W, phi, y, m, xs, gp, *a, order=o, compute=compute, **k)[:2] + (order,)
        runs = {"median": run(0, True), "mode": run(1, False), "quantile": run(2, False, u[:, :, :1]),
                "its_reject": run(4, True, u, max_trials=3, rejection_threshold=1.0)}
        info = eng.impute_info()
        assert not info["closed_form_densities"] and not info["batched_sweep"], info          # the table route
        with pytest.raises(L.MPSTError) as e:
            eng.impute_model(W, phi, y, m, xs, gp, 3, True, order=o, compute=compute)
        assert e.value.code == L.MPST_ERR_UNSUPPORTED
    finally:
        eng.close()
    classes = I.expand_label_index(W)
    _accept(runs, m, xs, compute == "f64", lambda i, sites, method: _td_oracle(classes, phi, y, i, sites, xs, gp, method, order, u))


def test_per_site_mode_is_the_argmax_of_the_brute_force_density(engine_cls):
    """Independent of the restatement's chain algebra: for one instance with one missing site the density contracted from the full chain
    with density-matrix environments, on THAT site's table, peaks at the device's mode."""
    N, T, C, d, aux = 5, 8, 2, 6, 2
    W, xs, gp, X, y, phi, m, rng = _td_problem(N, T, d, aux, 7, C, seed=77, ngrid=801, cx=False)
    eng = engine_cls(0)
    try:
        x, _, _ = eng.impute_model(W, phi, y, m, xs, gp, 1, False)
    finally:
        eng.close()
    i, site = 2, T // 2                                   # the instance with exactly one missing site
    assert m[i].sum() == 1
    p = I.brute_force_conditional(I.expand_label_index(W)[y[i]], phi[i], m[i] == 0, site, {}, gp[site])
    assert x[i, site] == xs[int(np.argmax(p))]
    other = (site + 1) % T                                # with another site's table the density is a different one (shapes compared:
    q = I.brute_force_conditional(I.expand_label_index(W)[y[i]], phi[i], m[i] == 0, site, {}, gp[other])     # a random chain's scale is tiny)
    assert np.abs(p / p.max() - q / q.max()).max() > 1e-3


@pytest.mark.parametrize("cx", [False, True], ids=["legendre", "fourier"])
def test_stride_zero_identity(engine_cls, cx):
    """T copies of one table through the per-site door give the bits of the shared table on the table route (a grid perturbed off the
    uniform spacing defeats the closed-form recognition, as in the table-route tests)."""
    from tests.test_gpu_impute_model import _problem
    N, T, C, d, chi = 21, 10, 3, 6, 9
    W, xs, enc, grid_phi, X, y, phi, m, rng = _problem(N, T, d, chi, C, seed=91, ngrid=1201, cx=cx)
    xs = xs.copy()
    xs[1:-1] += 1e-7 * np.sin(np.arange(1, len(xs) - 1))               # still increasing, no longer uniform
    grid_phi = np.ascontiguousarray(enc(xs))
    per_site = np.ascontiguousarray(np.broadcast_to(grid_phi, (T,) + grid_phi.shape))
    u = rng.uniform(0.02, 0.98, (N, T, 3))
    eng = engine_cls(0)
    try:
        for compute in ("f64", "f32"):
            for args, kw in (((0, True), {}), ((1, False), {}), ((2, False, u[:, :, :1]), {}), ((4, True, u), dict(max_trials=3, rejection_threshold=1.0))):
                for o in (0, 1):
                    a = eng.impute_model(W, phi, y, m, xs, grid_phi, *args, order=o, compute=compute, **kw)
                    info = eng.impute_info()
                    assert not info["closed_form_densities"] and not info["batched_sweep"]
                    b = eng.impute_model(W, phi, y, m, xs, per_site, *args, order=o, compute=compute, **kw)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        eng.close()


def test_grid_per_site_values_other_than_0_and_1_are_invalid(engine_cls):
    from tests.test_gpu_impute_model import _problem
    W, xs, enc, grid_phi, X, y, phi, m, rng = _problem(3, 5, 2, 3, 2, seed=1, ngrid=101, cx=False)
    eng = engine_cls(0)
    try:
        real = L.ImputeOpts

        class Bad(L.ImputeOpts):
            def __init__(self, *a):
                super().__init__(*a)
                self.grid_per_site = 2
        L.ImputeOpts = Bad
        try:
            with pytest.raises(L.MPSTError) as e:
                eng.impute_model(W, phi, y, m, xs, grid_phi, 0, True)
        finally:
            L.ImputeOpts = real
        assert e.value.code == L.MPST_ERR_INVALID
    finally:
        eng.close()


def test_the_context_doors_and_trajectories_and_distributions_per_site(engine_cls):
    """mpst_impute (context), *_traj (K = 3: seeded = three single calls fed the generator's numbers) and *_dist (two levels, cdf stride
    50) with a per-site table, real model, N = 5, T = 8."""
    from tests import philox_ref
    N, T, C, d, aux, chi = 5, 8, 2, 6, 2, 6
    W, xs, gp, X, y, phi, m, rng = _td_problem(N, T, d, aux, chi, C, seed=303, ngrid=801, cx=False)
    order = np.argsort(y, kind="stable")
    y, phi, m = y[order], np.ascontiguousarray(phi[order]), np.ascontiguousarray(m[order])       # the context wants class-sorted sets
    classes = I.expand_label_index(W)
    rid = np.arange(100, 100 + N, dtype=np.int64)
    useed = philox_ref.uniforms(12345, rid, 3, T, 1)                   # (N, K, T, 1)
    eng = engine_cls(0)
    try:
        xm, em, _ = eng.impute_model(W, phi, y, m, xs, gp, 0, True)
        tr_x, _, _ = eng.impute_model(W, phi, y, m, xs, gp, 2, False, num_trajectories=3, seed=12345, row_id=rid)
        singles = [eng.impute_model(W, phi, y, m, xs, gp, 2, False, np.ascontiguousarray(useed[:, k]))[0] for k in range(3)]
        dm = eng.impute_model(W, phi, y, m, xs, gp, 0, True, levels=(0.1, 0.9), cdf_stride=50)
        eng.set_options(chi_max=chi)
        eng.set_dataset(1, phi, y, C)
        eng.set_mps(W)
        xc, ec, _ = eng.impute(1, m, xs, gp, 0, True)
        tc_x, _, _ = eng.impute(1, m, xs, gp, 2, False, num_trajectories=3, seed=12345, row_id=rid)
        dc = eng.impute(1, m, xs, gp, 0, True, levels=(0.1, 0.9), cdf_stride=50)
        assert not eng.impute_info()["closed_form_densities"]
    finally:
        eng.close()
    assert np.array_equal(xc, xm) and np.array_equal(ec, em)                      # the two plain doors agree
    assert tr_x.shape == (N, 3, T) and np.array_equal(tc_x, tr_x)
    for k in range(3):
        assert np.array_equal(tr_x[:, k], singles[k])
    for out in (dm, dc):
        assert np.array_equal(out[0], xm) and np.array_equal(out[1], em)
    assert np.array_equal(dm[3], dc[3]) and np.array_equal(dm[4], dc[4])
    q, cdf = dm[3], dm[4]
    idx = np.unique(np.concatenate([np.arange(0, len(xs), 50), [len(xs) - 1]]))
    dx = xs[1] - xs[0]
    checked = 0
    for i in range(N):
        sites = np.flatnonzero(m[i])
        if len(sites) == 0:
            continue
        xo, eo, cdfs = TD.impute(classes[y[i]], phi[i], sites, xs, gp, "median", "forwards", True, None, return_cdfs=True)
        if np.abs(xm[i, sites] - xo).max() > 1e-12:
            continue                                                             # a flipped median re-conditions the rest of the chain
        for r, j in enumerate(sites):
            assert np.abs(cdf[i, r] - cdfs[r][idx]).max() <= 1e-10
            for l, lev in enumerate((0.1, 0.9)):
                assert abs(q[i, j, l] - xs[int(np.argmin(np.abs(cdfs[r] - lev)))]) <= dx * 1.0000001
            checked += 1
    assert checked >= 5
    # a single missing site: the existing restatement fed that site's own table
    from tests import impute_dist_ref
    i = int(np.flatnonzero(m.sum(axis=1) == 1)[0])
    j = int(np.flatnonzero(m[i])[0])
    med, wm, cd, lidx, _ = impute_dist_ref.impute_med_and_cdfs(classes[y[i]], phi[i], [j], xs, gp[j], levels=(0.1, 0.9))
    assert abs(xm[i, j] - med[0]) <= dx * 1.0000001 and np.abs(cdf[i, 0] - cd[0][idx]).max() <= 1e-10


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_impute_dataset_and_get_cdfs_on_a_trained_hist_split_model(hist_fit):
    Xtr, ytr, Xte, yte, opts, trained, info, te = hist_fit
    imp = mt.init_imputation_problem(trained, Xte, yte, dx=1e-3, verbosity=0)
    xr = imp.x_guess_range
    T = Xte.shape[1]
    assert xr.xvals_enc.shape == (T, len(xr.xvals), 6)
    mask = np.zeros(Xte.shape, dtype=bool)
    mask[:, 3:7] = True
    ts, err = mt.impute_dataset(imp, mask, "median")
    assert np.all(np.isfinite(ts)) and np.all(np.isfinite(err[mask])) and np.allclose(ts[~mask], Xte[~mask], rtol=0, atol=1e-9)
    with pytest.raises(NotImplementedError, match="closed-form bases only"):
        mt.impute_dataset(imp, mask, "mean")
    # in the encoding's domain against the restatement, instance by instance
    xs_dom, err_dom = mt.impute_dataset(imp, mask, "median", invert_transform=False)
    enc, norms, raw, full, scaled, oob = mt.imputation._scaled_instances(imp, np.arange(len(Xte)), mask)
    # inside the training range: the guess range is the encoding's range, which the transformed training data spans exactly; in the
    # original units for every series the test transform did not have to rescale (a rescaled series is stretched back on the way out)
    a, b = enc.range
    assert xs_dom[mask].min() >= a and xs_dom[mask].max() <= b
    plain = np.setdiff1d(np.arange(len(Xte)), [int(o[0]) for o in oob])
    assert len(plain) > 0 and ts[plain][mask[plain]].min() >= Xtr.min() - 1e-9 and ts[plain][mask[plain]].max() <= Xtr.max() + 1e-9
    phi = imp.encoder(scaled)
    classes = I.expand_label_index(trained.mps)
    m8 = mask.astype(np.uint8)
    xg = np.where(mask, xs_dom, 0.0)
    eg = np.where(mask, err_dom, 0.0)
    lab = [imp.class_map[c] for c in yte.tolist()]
    _accept({"median": (xg, eg, "forwards")}, m8, xr.xvals, True,
            lambda i, sites, method: TD.impute(classes[lab[i]], phi[i], sites, xr.xvals, xr.xvals_enc, "median", "forwards", True, None))
    cdfs, ts1, pe, target = mt.get_cdfs(imp, int(yte[0]), 0, np.arange(3, 7), stride=10)
    assert len(cdfs) == 4 and all(np.all(np.diff(c) >= -1e-15) and abs(c[-1] - 1.0) < 1e-12 and c[0] == 0.0 for c in cdfs)
    assert np.all(np.isfinite(ts1[0])) and ts1[0].min() >= a and ts1[0].max() <= b


def test_fit_batch_fits_each_folds_bins_from_its_own_rows():
    Xtr, ytr, Xte, yte = _fit_data()
    opts = mt.MPSOptions(encoding="hist_split_legendre", d=6, aux_basis_dim=2, chi_max=6, nsweeps=1, verbosity=-1)
    folds = [(np.arange(0, 32), np.arange(32, 48)), (np.arange(16, 48), np.arange(0, 16))]
    jobs = [(Xtr[tr], ytr[tr], opts, Xtr[va], ytr[va]) for tr, va in folds]
    out = mt.tuning.fit_batch(jobs)
    bins = []
    for (tr, va), res in zip(folds, out):
        assert res.error is None
        trained = res.mps
        enc, _, encoder = E.fit_encoding_from_training_data(trained.opts, trained.train_data.original_data, trained.train_data.labels)
        Xs, _ = E.transform_train_data(Xtr[tr], opts, enc.range)
        assert np.array_equal(encoder.bins, E.hist_split(Xs, 3, *enc.range))
        assert np.array_equal(trained.train_data.phi, encoder(Xs[np.argsort(ytr[tr], kind="stable")]))
        bins.append(encoder.bins)
    assert not np.array_equal(bins[0], bins[1])
