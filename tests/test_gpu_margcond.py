"""mpst_marginal_conditionals on the device against the NumPy restatement (tests/margcond_ref.py, pinned to the dense amplitude tensor
by tests/test_margcond_host.py), against the shipped kernels where the two questions coincide, block by block and row by row, its
refusals, and end to end through the Python layer.

Bounds (the project's own; not from what the kernels give): |nll - ref| <= 1e-10, |pit - ref| <= 1e-12,
|mean - ref| <= 1e-12 max|grid_x|; median, every level and the WMAD are selections on the grid and must be EQUAL wherever the
restatement's own selection margin exceeds 1e-9.  At most 1 % of the (series, site) pairs of a case may be excused by that margin,
which is asserted on the restatement alone before the device is looked at.  nll and pit are NaN exactly at the missing sites without a
true value; the states there are NaN in the inputs, so a kernel that read them would show.

Largest deviations found on the MI355X: chains of up to ten sites nll 4.5e-12 (one value next to a zero of the density), pit 8.3e-15,
mean 8.0e-15; T = 1000 nll 9.9e-13, pit 2.7e-13, mean 3.6e-13 (the restatement itself is 1.5e-13 in F and 6.2e-13 in nll off
extended-precision walks there); no pair excused in any case."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import marginal
from tests import margcond_ref as M

pytestmark = pytest.mark.gpu

NLL_TOL, PIT_TOL, MEAN_TOL = 1e-10, 1e-12, 1e-12
LEVELS = (0.05, 0.5, 0.95)
# (T, d, chi, C, N): one site and a bond of one; ragged bonds and a ragged tile; three classes; bonds of 72 (global scratch for real
# and complex models, five column tiles on four waves: the second tile of a wave); a thousand sites
SHAPES = [(1, 3, 1, 2, 3), (9, 4, 7, 2, 19), (10, 3, 12, 3, 17), (6, 4, 72, 2, 5)]
LONG = (1000, 4, 8, 2, 2)


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case(T, d, chi, C_, N, cx=False, label="last", ngrid=201, per_site=False):
    """(inputs, restatement) - built once, shared by the tests below, never modified"""
    seed = 9000 + 31 * T + 7 * d + chi + 3 * C_ + N + ngrid + (1 if cx else 0) + (2 if label == "mid" else 0) + (4 if per_site else 0)
    long_chain = T >= 1000
    inp = M.make_case(T, d, chi, C_, N, seed, cx=cx, label_site=T // 2 if label == "mid" else None, ngrid=ngrid, long_chain=long_chain,
                      per_site=per_site, full_bonds=chi > 64)
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    ref = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gphi, LEVELS)
    for a in list(W) + [phi, lab, miss, x_in, xs, gphi, x]:
        a.setflags(write=False)
    return inp, ref


def check(out, inp, ref, what=""):
    """the restatement decides alone first, then the device is compared"""
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    excused = ref.excused
    assert excused.mean() <= 0.01, (what, float(excused.mean()))
    nanpat = miss & ~np.isfinite(x_in)
    ok = ~nanpat
    with np.errstate(invalid="ignore"):
        dn = float(np.abs(np.where(out.nll == ref.sc.nll, 0.0, out.nll - ref.sc.nll))[ok].max()) if ok.any() else 0.0
    dp = float(np.abs(out.pit - ref.sc.pit)[ok].max()) if ok.any() else 0.0
    dm = float(np.abs(out.mean - ref.mean).max())
    print(f"{what}: |nll - ref| = {dn:.3e} (bound {NLL_TOL:g}), |pit - ref| = {dp:.3e} (bound {PIT_TOL:g}), |mean - ref| = {dm:.3e} "
          f"(bound {MEAN_TOL * np.abs(xs).max():g}), excused {int(excused.sum())} of {excused.size}")
    assert np.array_equal(np.isnan(out.nll), nanpat), np.argwhere(np.isnan(out.nll) != nanpat)
    assert np.array_equal(np.isnan(out.pit), nanpat), np.argwhere(np.isnan(out.pit) != nanpat)
    for a in (out.median, out.err, out.mean, out.quantiles):
        assert np.all(np.isfinite(a))
    sel = ~excused
    assert np.array_equal(out.median[sel], ref.sc.median[sel]), np.argwhere(sel & (out.median != ref.sc.median))
    assert np.array_equal(out.err[sel], ref.sc.err[sel]), np.argwhere(sel & (out.err != ref.sc.err))
    assert np.array_equal(out.quantiles[sel], ref.sc.quantiles[sel]), np.argwhere(sel[:, :, None] & (out.quantiles != ref.sc.quantiles))
    assert np.array_equal(out.quantiles[:, :, 1], out.median)           # level 0.5 is the median
    assert dn <= NLL_TOL and dp <= PIT_TOL and dm <= MEAN_TOL * np.abs(xs).max()


def run(eng, inp, levels=LEVELS, **kw):
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    return eng.marginal_conditionals(W, phi, lab, miss, x_in, xs, gphi, levels=levels, **kw)


def test_the_masks_hold_every_pattern():
    (W, phi, lab, miss, x_in, xs, gphi, x), _ = case(9, 4, 7, 2, 19)
    T = miss.shape[1]
    assert not miss[0].any() and miss[1].all() and miss[2].sum() == 2 and miss[2, 0] and miss[2, T - 1]
    assert miss[3].sum() >= 2 and np.all(np.diff(np.flatnonzero(miss[3])) == 1) and miss[4].sum() == 1
    frac = miss[5:].mean()
    assert 0.15 < frac < 0.45
    held = miss & np.isfinite(x_in)
    assert held.any() and (miss & ~held).any() and np.isnan(phi[miss & ~held]).all()


@pytest.mark.parametrize("ngrid", [201, 257])
@pytest.mark.parametrize("label", ["last", "mid"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_against_the_restatement(eng, shape, cx, label, ngrid):
    inp, ref = case(*shape, cx, label, ngrid)
    check(run(eng, inp), inp, ref, f"{'complex' if cx else 'real'} {shape} {label} {ngrid}")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_one_table_per_site(eng, cx):
    inp, ref = case(9, 4, 7, 2, 19, cx, "mid", 201, True)
    assert inp[6].ndim == 3
    check(run(eng, inp), inp, ref, f"{'complex' if cx else 'real'} per-site table")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_long_chain_is_rescaled(eng, cx):
    """T = 1000: the unscaled densities leave the range of fp64; every output finite where it is due, bounds as above"""
    inp, ref = case(*LONG, cx)
    check(run(eng, inp), inp, ref, f"T = 1000 {'complex' if cx else 'real'}")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_nothing_missing_is_mpst_site_conditionals(eng, cx):
    W, phi, lab, miss, x_in, xs, gphi, x = case(9, 4, 7, 2, 19, cx)[0]
    ph = np.asarray(mt.model_encoding("Fourier" if cx else "Legendre_No_Norm").encode(x.ravel(), 4)).reshape(phi.shape)
    nll, pit, med, err, q, _ = eng.site_conditionals(W, ph, lab, x, xs, gphi, levels=LEVELS)
    for mask in (None, np.zeros(x.shape, dtype=bool)):
        out = eng.marginal_conditionals(W, ph, lab, mask, x, xs, gphi, levels=LEVELS)
        print(f"nothing missing: |nll - site| = {np.abs(out.nll - nll).max():.3e}, |pit - site| = {np.abs(out.pit - pit).max():.3e}")
        assert np.array_equal(out.median, med) and np.array_equal(out.quantiles, q)
        assert np.abs(out.nll - nll).max() <= NLL_TOL and np.abs(out.pit - pit).max() <= PIT_TOL


@pytest.mark.parametrize("ngrid", [257, 201])
def test_one_missing_site_is_the_median_imputer_and_the_held_out_score(eng, ngrid):
    """the N T one-missing-site replicas: at the missing site the median and the levels of mpst_impute_model_dist (the conditioned
    state is pure there, so its |rho phi|^2 and the Born value differ by a constant), and with the true value supplied the nll and
    pit of mpst_site_conditionals on the complete series"""
    W, phi, lab, miss, x_in, xs, gphi, x = case(9, 4, 7, 2, 19, False, "last", ngrid)[0]
    ph = np.asarray(mt.model_encoding("Legendre_No_Norm").encode(x.ravel(), 4)).reshape(phi.shape)
    N, T = x.shape
    nll, pit, med, err, q, _ = eng.site_conditionals(W, ph, lab, x, xs, gphi, levels=LEVELS)
    mask = np.tile(np.eye(T, dtype=np.uint8), (N, 1))
    sel = mask.astype(bool)
    rp, rl, rx = np.repeat(ph, T, axis=0), np.repeat(lab, T), np.repeat(x, T, axis=0)
    xi, ei, _, qi, _ = eng.impute_model(W, rp, rl, mask, xs, gphi, method=0, get_wmad=True, levels=LEVELS)
    out = eng.marginal_conditionals(W, rp, rl, mask, rx, xs, gphi, levels=LEVELS)
    assert np.array_equal(out.median[sel], xi[sel]) and np.array_equal(out.quantiles[sel], qi[sel])
    dn, dp = np.abs(out.nll[sel].reshape(N, T) - nll).max(), np.abs(out.pit[sel].reshape(N, T) - pit).max()
    print(f"ngrid {ngrid}: held-out |nll - site| = {dn:.3e}, |pit - site| = {dp:.3e}")
    assert np.array_equal(out.median[sel].reshape(N, T), med) and np.array_equal(out.quantiles[sel].reshape(N, T, -1), q)
    assert dn <= NLL_TOL and dp <= PIT_TOL


def _tiled(inp, reps):
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    return W, np.tile(phi, (reps, 1, 1)), np.tile(lab, reps), np.tile(miss, (reps, 1)), np.tile(x_in, (reps, 1)), xs, gphi, np.tile(x, (reps, 1))


FIELDS = ("nll", "pit", "median", "err", "mean", "quantiles")


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(getattr(a, f)[rows_a], getattr(b, f)[rows_b], equal_nan=True) for f in FIELDS)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_blocks_do_not_change_the_result(eng, monkeypatch, cx):
    """N = 136 at 10 * (144 + 9 + 8) * 8 = 12 880 bytes per instance (complex: 25 120) under a scratch budget of 1 MB: blocks of 83
    (complex: 42) instances, the same bits as one block"""
    inp = _tiled(case(10, 3, 12, 3, 17, cx)[0], 8)
    one = run(eng, inp)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    two = run(eng, inp)
    assert same_bits(one, two)
    assert same_bits(one, one, slice(0, 17), slice(119, 136))           # the replicas: what travels along does not matter


@pytest.mark.parametrize("shape,cx", [((9, 4, 7, 2, 19), False), ((9, 4, 7, 2, 19), True), ((6, 4, 72, 2, 5), False)],
                         ids=["lds-real", "lds-complex", "global-scratch"])
def test_rows_do_not_depend_on_their_neighbours(eng, shape, cx):
    inp = case(*shape, cx)[0]
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    full = run(eng, inp)
    for i in range(0, x.shape[0], 3):
        alone = eng.marginal_conditionals(W, phi[i:i + 1], lab[i:i + 1], miss[i:i + 1], x_in[i:i + 1], xs, gphi, levels=LEVELS)
        assert same_bits(alone, full, slice(None), slice(i, i + 1)), i


def test_outputs_may_be_skipped(eng):
    inp, ref = case(9, 4, 7, 2, 19)
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    out = run(eng, inp, levels=None, get_wmad=False)
    assert out.quantiles is None and out.err is None
    sel = ~ref.excused
    assert np.array_equal(out.median[sel], ref.sc.median[sel])
    # straight through the C interface: only the mean, no x and no mask
    ph = np.asarray(mt.model_encoding("Legendre_No_Norm").encode(x.ravel(), 4)).reshape(phi.shape)
    m, keep = marginal.model_struct(W, ph, "f64")
    labs = np.ascontiguousarray(lab, dtype=np.int32)
    m.label_idx = labs.ctypes.data_as(C.POINTER(C.c_int32))
    dp = C.POINTER(C.c_double)
    o = mt._lib.SiteCondOpts(0, 0, 0, 0, None)
    mean = np.zeros(x.shape)
    rc = eng.lib.mpst_marginal_conditionals(eng.ctx, C.byref(m), None, None, xs.ctypes.data_as(dp), C.c_void_p(gphi.ctypes.data), len(xs),
                                            C.byref(o), None, None, None, None, mean.ctypes.data_as(dp), None, None)
    assert rc == 0 and np.all(np.isfinite(mean))
    full = eng.marginal_conditionals(W, ph, lab, None, x, xs, gphi)
    assert np.array_equal(mean, full.mean)


def test_refusals_leave_the_context_as_it_was(eng):
    inp, ref = case(9, 4, 7, 2, 19)
    W, phi, lab, miss, x_in, xs, gphi, x = inp
    before = run(eng, inp)
    lib, dp = eng.lib, C.POINTER(C.c_double)
    INV, UNS = mt._lib.MPST_ERR_INVALID, mt._lib.MPST_ERR_UNSUPPORTED
    safe = np.where(np.isnan(phi), 0.0, phi)

    def call(model=True, x_=True, gx=True, gp=True, opt=True, ngrid=len(xs), outs=(1, 1, 1, 1, 1, 1), W_=W, phi_=safe, lab_=lab, compute="f64",
             levels=LEVELS, gps=0):
        m, keep = marginal.model_struct(W_, phi_, compute)
        labs = None if lab_ is None else np.ascontiguousarray(lab_, dtype=np.int32)
        m.label_idx = None if labs is None else labs.ctypes.data_as(C.POINTER(C.c_int32))
        lv = np.ascontiguousarray(levels, dtype=np.float64)
        o = mt._lib.SiteCondOpts(gps, 1, len(lv), 0, lv.ctypes.data_as(dp))
        n_, t_ = phi_.shape[:2]
        bufs = [np.zeros((n_, t_)) for _ in range(5)] + [np.zeros((n_, t_, max(1, len(lv))))]
        ptrs = [b.ctypes.data_as(dp) if on else None for b, on in zip(bufs, outs)]
        xx, mm = np.zeros((n_, t_)), np.zeros((n_, t_), dtype=np.uint8)
        rc = lib.mpst_marginal_conditionals(eng.ctx, C.byref(m) if model else None, mm.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            xx.ctypes.data_as(dp) if x_ else None, xs.ctypes.data_as(dp) if gx else None,
                                            C.c_void_p(gphi.ctypes.data) if gp else None, ngrid, C.byref(o) if opt else None, *ptrs, None)
        return rc, lib.mpst_last_error(eng.ctx).decode()

    for kw in (dict(model=False), dict(gx=False), dict(gp=False), dict(opt=False)):
        rc, msg = call(**kw)
        assert rc == INV and "NULL argument" in msg, (kw, rc, msg)
    rc, msg = call(outs=(0, 0, 0, 0, 0, 0))
    assert rc == INV and "every output is NULL" in msg
    rc, msg = call(x_=False)
    assert rc == INV and "pit_out needs the values x" in msg
    rc, msg = call(x_=False, outs=(1, 0, 1, 1, 1, 1))
    assert rc == 0, msg
    rc, msg = call(ngrid=1)
    assert rc == INV and "fewer than 2 grid values" in msg
    rc, msg = call(levels=np.linspace(0.05, 0.95, 17))
    assert rc == INV and "nq must lie in 0 .. 16" in msg
    rc, msg = call(levels=(0.5, 1.0))
    assert rc == INV and "is not inside (0, 1)" in msg
    rc, msg = call(outs=(1, 1, 1, 1, 1, 0))
    assert rc == INV and "nq > 0 needs levels[nq] and q_out" in msg
    rc, msg = call(lab_=None)
    assert rc == INV and "label_idx is NULL" in msg
    rc, msg = call(lab_=np.where(np.arange(len(lab)) == 3, 2, lab))
    assert rc == INV and "out of range" in msg
    rc, msg = call(gps=2)
    assert rc == INV and "grid_per_site must be 0" in msg
    rc, msg = call(compute="f32")
    assert rc == UNS and "fp64 only" in msg
    rng = np.random.default_rng(3)
    from tests.marginal_ref import gaussian_chain, random_states
    for d_, C_ in ((2, 17), (17, 2)):
        Wb = gaussian_chain(3, d_, 2, C_, 2, False, rng)
        rc, msg = call(W_=Wb, phi_=random_states(2, 3, d_, False, rng), lab_=np.zeros(2))
        assert rc == UNS and "marginal conditionals hold chi_max <= 128" in msg, (rc, msg)
    Wb = gaussian_chain(5, 16, 129, 1, 2, False, rng)            # (bond dimensions 1, 16, 129, 129, 16, 1)
    rc, msg = call(W_=Wb, phi_=random_states(2, 5, 16, False, rng), lab_=np.zeros(2))
    assert rc == UNS and "marginal conditionals hold chi_max <= 128" in msg, (rc, msg)
    assert same_bits(before, run(eng, inp))


# ---- end to end through the Python layer ----
def _problem(encoding, **kw):
    rng = np.random.default_rng(31)
    X1, _ = mt.trendy_sine(7, 30, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(7, 30, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(30, dtype=np.int64), np.ones(30, dtype=np.int64)])
    p = rng.permutation(60)
    X, y = X[p], y[p]
    opts = mt.MPSOptions(encoding=encoding, d=4, chi_max=8, nsweeps=2, verbosity=-1, **kw)
    trained, _, _ = mt.fitMPS(X[:52], y[:52], X[52:], y[52:], opts)
    return mt.init_imputation_problem(trained, X[52:], y[52:], dx=0.01, verbosity=0)


@pytest.fixture(scope="module", params=["Legendre_No_Norm", "hist_split_legendre"])
def problem(request):
    return _problem(request.param, **(dict(aux_basis_dim=2) if request.param.startswith("hist") else {}))


def test_python_layer_end_to_end(problem, eng):
    imp = problem
    N, T = imp.X_test.shape
    rng = np.random.default_rng(5)
    mask = rng.uniform(size=(N, T)) < 0.3
    mask[0] = False
    mask[1, 2:5] = True
    mc = mt.marginal_conditionals(imp, mask, quantiles=LEVELS, engine=eng)
    assert isinstance(mc, mt.MarginalConditionals) and mc.nll.shape == (N, T) and mc.quantiles.shape == (N, T, 3) and mc.seconds > 0.0
    assert np.array_equal(mc.missing, mask)
    # the test set holds every true value: held-out scores everywhere, NaN only for a true value outside the encoding's range
    assert np.all(np.isfinite(mc.pit)) and np.all((mc.pit >= 0.0) & (mc.pit <= 1.0))
    assert not np.isnan(mc.nll[~mask]).any() and np.all(np.isfinite(mc.median)) and np.all(np.isfinite(mc.mean))
    assert np.all(mc.quantiles[:, :, 0] <= mc.median) and np.all(mc.median <= mc.quantiles[:, :, 2])
    # a complete row is the leave-one-out conditional of site_conditionals
    sc = mt.site_conditionals(imp, rows=[0], quantiles=LEVELS, engine=eng)
    assert np.array_equal(mc.median[0], sc.median[0]) and np.abs(mc.nll[0] - sc.nll[0]).max() <= NLL_TOL
    # impute_marginal keeps the known values and fills the rest with the statistic
    enc_dom = mt.impute_marginal(imp, mask, invert_transform=False, engine=eng)
    assert np.array_equal(enc_dom[~mask], mc.x[~mask]) and np.array_equal(enc_dom[mask], mc.median[mask])
    assert np.array_equal(mt.impute_marginal(imp, mask, statistic="mean", invert_transform=False, engine=eng)[mask], mc.mean[mask])
    filled, bands = mt.impute_marginal(imp, mask, quantiles=LEVELS, engine=eng)
    assert np.allclose(filled[~mask], imp.X_test[~mask], rtol=0, atol=1e-9 * np.abs(imp.X_test).max())
    assert np.all(np.isfinite(filled)) and np.all(bands[:, :, 0] <= filled + 1e-12) and np.all(filled <= bands[:, :, 2] + 1e-12)
    assert np.allclose(bands[~mask], filled[~mask][:, None], rtol=0, atol=1e-9 * np.abs(imp.X_test).max())
    # forecasts: the bands contain the median; at horizon 1 the conditioned state is the sequential imputer's
    point, fb = mt.forecast(imp, 3, engine=eng)
    assert point.shape == (N, 3) and fb.shape == (N, 3, 2)
    assert np.all(fb[:, :, 0] <= point) and np.all(point <= fb[:, :, 1])
    one, _ = mt.forecast(imp, 1, invert_transform=False, engine=eng)
    last = np.zeros((N, T), dtype=bool)
    last[:, -1] = True
    seq = mt.impute_dataset(imp, last, "median", invert_transform=False, engine=eng)[0]
    assert np.array_equal(one[:, 0], seq[:, -1])
    # anomaly scores of incomplete series: the known sites' scores, the masked sites left out
    prof = mt.anomaly_scores(imp, reduce=None, missing_mask=mask, engine=eng)
    assert np.array_equal(np.isnan(prof), mask) and np.array_equal(prof[~mask], mc.nll[~mask])
    assert np.array_equal(mt.anomaly_scores(imp, reduce="max", missing_mask=mask, engine=eng), np.nanmax(prof, axis=1))
    assert np.array_equal(mt.anomaly_scores(imp, engine=eng), mt.site_conditionals(imp, get_wmad=False, engine=eng).nll.mean(axis=1))
    with pytest.raises(ValueError):
        mt.forecast(imp, 0)
    with pytest.raises(ValueError):
        mt.impute_marginal(imp, mask, statistic="mode")
