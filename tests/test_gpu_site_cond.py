"""mpst_site_conditionals on the device against the NumPy restatement (tests/site_cond_ref.py), against the median imputer on the
one-missing-site replicas, row by row, block by block, through the Python layer with one grid table per site, and its refusals.

Bounds (from the project, not from what the kernels give): pit within 1e-12 absolute (the normalised-cdf bound of the distribution
outputs), nll within 1e-10 absolute (the bound of tests/test_gpu_marginal.py); median, WMAD and every level are selections on the
grid and must be EQUAL wherever the restatement's own margins exceed 1e-9 - which is asserted for every (series, site, level) of
every case before the device is looked at.


The WMAD of the EXISTING median imputer is not the restatement's double everywhere: on a grid that is not made of exact doubles the two
grid values at the tipping distance deviate from the median by doubles a few 1e-16 apart, weighted_median returns the one at which the
cumulative weight passes half the total, k_imp_left the lower one (its tests allow one grid step against the oracle).  This call
follows weighted_median, so test_against_the_median_imputer_on_the_replicas asks for equal WMADs on the 257-point grid (step 2^-7,
exact doubles: the two deviations are the same double) and, on the 201-point grid, for medians and levels equal and WMADs within the
rounding of the grid values."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import conditionals, marginal
from tests import site_cond_ref as S

pytestmark = pytest.mark.gpu

PIT_TOL, NLL_TOL = 1e-12, 1e-10
LEVELS = (0.05, 0.5, 0.95)


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case(T, d, chi, C_, N, cx=False, label="last", ngrid=201, long_chain=False, scaled=False):
    """(inputs, restatement) - built once, shared by the tests below, never modified.  ``scaled``: the restatement in its scaled form
    (the definition as stated; tests/test_site_cond_host.py pins it to the brute-force form), where the brute-force form underflows
    (T = 1000) or takes minutes on the host (chi = 72: dense 72 x 72 environments through an unoptimised einsum)"""
    seed = 4000 + 31 * T + 7 * d + chi + 3 * C_ + N + ngrid + (1 if cx else 0) + (2 if label == "mid" else 0)
    inp = S.make_case(T, d, chi, C_, N, seed, cx=cx, label_site=T // 2 if label == "mid" else None, ngrid=ngrid, long_chain=long_chain)
    W, phi, lab, x, xs, gphi = inp
    ref = (S.scaled_site_conditionals if long_chain or scaled else S.site_conditionals_ref)(W, phi, lab, x, xs, gphi, LEVELS)
    for a in list(W) + [phi, lab, x, xs, gphi]:
        a.setflags(write=False)
    return inp, ref


def check(got, ref, what=""):
    """the restatement decides alone first, then the device is compared"""
    assert ref.margins_ok(1e-9), (what, ref.med_margin.min(), ref.lev_margin.min(), ref.err_margin.min())
    nll, pit, med, err, q = got[:5]
    dn, dp = float(np.abs(nll - ref.nll).max()), float(np.abs(pit - ref.pit).max())
    print(f"{what}: |nll - ref| = {dn:.3e} (bound {NLL_TOL:g}), |pit - ref| = {dp:.3e} (bound {PIT_TOL:g}), smallest margins "
          f"{ref.med_margin.min():.2e} / {ref.lev_margin.min():.2e} / {ref.err_margin.min():.2e}")
    assert np.all(np.isfinite(nll)) and np.all(np.isfinite(pit))
    assert np.array_equal(med, ref.median), np.argwhere(med != ref.median)
    assert np.array_equal(err, ref.err), np.argwhere(err != ref.err)
    assert np.array_equal(q, ref.quantiles), np.argwhere(q != ref.quantiles)
    assert np.array_equal(q[:, :, 1], med)                      # level 0.5 is the median
    assert dn < NLL_TOL and dp < PIT_TOL


# (T, d, chi, C, N): one ragged tile; a ragged last tile of sixteen; three tiles with C = 1
REAL_SHAPES = [(6, 3, 4, 2, 5), (9, 4, 7, 2, 19), (12, 4, 12, 1, 33)]


@pytest.mark.parametrize("ngrid", [201, 257])
@pytest.mark.parametrize("label", ["last", "mid"])
@pytest.mark.parametrize("T,d,chi,C_,N", REAL_SHAPES, ids=["6-3-4-2-5", "9-4-7-2-19", "12-4-12-1-33"])
def test_real_models_against_the_restatement(eng, T, d, chi, C_, N, label, ngrid):
    (W, phi, lab, x, xs, gphi), ref = case(T, d, chi, C_, N, False, label, ngrid)
    check(eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS), ref, f"real {T}-{d}-{chi}-{C_}-{N} {label} {ngrid}")


@pytest.mark.parametrize("label", ["last", "mid"])
def test_complex_model_against_the_restatement(eng, label):
    (W, phi, lab, x, xs, gphi), ref = case(7, 4, 5, 2, 6, True, label)
    check(eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS), ref, f"complex 7-4-5-2-6 {label}")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_bond_dimension_beyond_one_wave_per_tile(eng, cx):
    """chi = 72: five column tiles on four waves (the second tile of a wave), beyond the LDS limit of the environment pass"""
    (W, phi, lab, x, xs, gphi), ref = case(10, 4, 72, 1, 3, cx, "last", 101, scaled=True)
    check(eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS), ref, f"chi 72 {'complex' if cx else 'real'}")


def test_long_chain_is_rescaled(eng):
    """T = 1000: the unscaled environments underflow (ln of the overlap loses about 0.9 per site); every output finite, bounds as above,
    against the scaled form of the definition (which tests/test_site_cond_host.py pins to the brute-force form)"""
    (W, phi, lab, x, xs, gphi), ref = case(1000, 4, 8, 1, 3, False, "last", 101, True)
    got = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    assert all(np.all(np.isfinite(a)) for a in got[:5])
    check(got, ref, "T = 1000")


@pytest.mark.parametrize("ngrid", [257, 201])
def test_against_the_median_imputer_on_the_replicas(eng, ngrid):
    """impute_model(levels=..., median) on the N T one-missing-site replicas: medians and levels equal to this call's on both grids.
    WMADs: equal on the 257-point grid, whose values are exact doubles.  On the 201-point grid the imputer names the lower of the two
    grid values at the tipping distance where weighted_median (and this call) may name the upper one: the same deviation in exact
    arithmetic, and as doubles apart by the rounding of two grid values, each half a unit in the last place of the largest one."""
    (W, phi, lab, x, xs, gphi), ref = case(9, 4, 7, 2, 19, False, "last", ngrid)
    N, T = x.shape
    nll, pit, med, err, q, _ = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    mask = np.tile(np.eye(T, dtype=np.uint8), (N, 1))
    xi, ei, _, qi, _ = eng.impute_model(W, np.repeat(phi, T, axis=0), np.repeat(lab, T), mask, xs, gphi, method=0, get_wmad=True, levels=LEVELS)
    sel = mask.astype(bool)
    ei = ei[sel].reshape(N, T)
    assert np.array_equal(xi[sel].reshape(N, T), med)
    assert np.array_equal(qi[sel].reshape(N, T, len(LEVELS)), q) and np.array_equal(q[:, :, 1], med)
    print(f"ngrid {ngrid}: {int((ei != err).sum())} of {err.size} WMADs differ from the imputer's, largest |difference| {np.abs(ei - err).max():.3e}")
    if ngrid == 257:
        assert np.array_equal(ei, err)
    else:
        assert np.abs(ei - err).max() <= 2.0 * np.spacing(np.abs(xs).max())


def test_rows_do_not_depend_on_their_neighbours(eng):
    """every row sent alone gives what it gave in the batch: within the bounds (required), and bit for bit (what the design promises)"""
    (W, phi, lab, x, xs, gphi), ref = case(9, 4, 7, 2, 19)
    full = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    exact = True
    for i in range(x.shape[0]):
        one = eng.site_conditionals(W, phi[i:i + 1], lab[i:i + 1], x[i:i + 1], xs, gphi, levels=LEVELS)
        assert np.abs(one[0] - full[0][i]).max() < NLL_TOL and np.abs(one[1] - full[1][i]).max() < PIT_TOL
        assert all(np.array_equal(one[k][0], full[k][i]) for k in (2, 3, 4))
        exact = exact and all(np.array_equal(one[k][0], full[k][i]) for k in (0, 1))
    print("rows alone equal the batch bit for bit:", exact)
    assert exact


def test_blocks_do_not_change_the_result(eng, monkeypatch):
    """N = 700 under a scratch budget of 1 MB: two blocks of instances, the same bits as in one"""
    W, phi, lab, x, xs, gphi = S.make_case(12, 4, 12, 2, 700, seed=77, label_site=5, ngrid=65)
    one = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    two = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    assert all(np.array_equal(a, b) for a, b in zip(one[:5], two[:5]))
    few = eng.site_conditionals(W, phi[640:], lab[640:], x[640:], xs, gphi, levels=LEVELS)
    assert all(np.array_equal(a, b[640:]) for a, b in zip(few[:5], one[:5]))


def test_outputs_may_be_skipped_and_zero_density_gives_nan(eng):
    (W, phi, lab, x, xs, gphi), ref = case(6, 3, 4, 2, 5)
    nll, pit, med, err, q, _ = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=None, get_wmad=False)
    assert q is None and np.all(err == 0.0) and np.array_equal(med, ref.median) and np.abs(nll - ref.nll).max() < NLL_TOL
    # a series whose state at site 2 is zero: every OTHER site of it has a vanishing conditional (Z = 0), site 2 itself does not
    ph = np.array(phi)
    ph[1, 2] = 0.0
    nll, pit, med, err, q, _ = eng.site_conditionals(W, ph, lab, x, xs, gphi, levels=LEVELS)
    others = [t for t in range(x.shape[1]) if t != 2]
    assert all(np.all(np.isnan(a[1][others])) for a in (nll, pit, med, err, q))
    assert np.isposinf(nll[1, 2]) and np.isfinite(pit[1, 2]) and med[1, 2] == ref.median[1, 2]
    keep = [0, 2, 3, 4]
    assert np.array_equal(med[keep], ref.median[keep]) and np.all(np.isfinite(nll[keep]))


@pytest.fixture(scope="module")
def hist_problem():
    """a hist_split_legendre model (d = 4, aux_basis_dim = 2, T = 7) trained for two sweeps on trendy_sine data, N = 8 test series:
    (imputation problem, its labels, the trained model, the raw test series, site_conditionals(imp), the restatement fed with encoder.table)"""
    rng = np.random.default_rng(31)
    X1, _ = mt.trendy_sine(7, 30, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(7, 30, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(30, dtype=np.int64), np.ones(30, dtype=np.int64)])
    p = rng.permutation(60)
    X, y = X[p], y[p]
    opts = mt.MPSOptions(encoding="hist_split_legendre", d=4, aux_basis_dim=2, chi_max=8, nsweeps=2, verbosity=-1)
    trained, _, _ = mt.fitMPS(X[:52], y[:52], X[52:], y[52:], opts)
    imp = mt.init_imputation_problem(trained, X[52:], y[52:], dx=0.01, verbosity=0)
    xr = imp.x_guess_range
    assert xr.xvals_enc.shape == (7, len(xr.xvals), 4)
    out = mt.site_conditionals(imp, quantiles=LEVELS)
    assert out.x.shape == (8, 7)
    lab = np.array([imp.class_map[c] for c in y[52:].tolist()], dtype=np.int32)
    table = np.asarray(imp.encoder.table(xr.xvals, 7))
    ref = S.site_conditionals_ref(imp.mps, np.asarray(imp.encoder(out.x)), lab, out.x, xr.xvals, table, LEVELS)
    return imp, y[52:], trained, X[52:], out, ref


def test_per_site_tables_through_the_python_layer(hist_problem):
    imp, yte, trained, Xte, out, ref = hist_problem
    check((out.nll, out.pit, out.median, out.err, out.quantiles), ref, "hist_split_legendre, one table per site")
    sc = mt.anomaly_scores(imp, rows=[1, 4], reduce=None)
    assert np.array_equal(sc, out.nll[[1, 4]])
    assert np.array_equal(mt.anomaly_scores(imp, reduce="max"), out.nll.max(axis=1))
    assert np.array_equal(mt.anomaly_scores(imp), out.nll.mean(axis=1))
    with pytest.raises(KeyError):
        mt.site_conditionals(mt.init_imputation_problem(trained, Xte, yte + 5, dx=0.01, verbosity=0))


def test_refusals_by_message_leave_the_context_as_it_was(eng):
    (W, phi, lab, x, xs, gphi), ref = case(6, 3, 4, 2, 5)
    before = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    lib, dp = eng.lib, C.POINTER(C.c_double)
    N, T = x.shape
    INV, UNS = mt._lib.MPST_ERR_INVALID, mt._lib.MPST_ERR_UNSUPPORTED

    def call(model=True, x_=True, gx=True, gp=True, ngrid=len(xs), opts=None, outs=(1, 1, 1, 1, 1), W_=W, phi_=phi, lab_=lab, compute="f64",
             levels=LEVELS, gps=0):
        m, keep = marginal.model_struct(W_, phi_, compute)
        labs = None if lab_ is None else np.ascontiguousarray(lab_, dtype=np.int32)
        m.label_idx = None if labs is None else labs.ctypes.data_as(C.POINTER(C.c_int32))
        lv = np.ascontiguousarray(levels, dtype=np.float64)
        o = opts or mt._lib.SiteCondOpts(gps, 1, len(lv), 0, lv.ctypes.data_as(dp))
        n_, t_ = phi_.shape[:2]
        bufs = [np.zeros((n_, t_)) for _ in range(4)] + [np.zeros((n_, t_, max(1, len(lv))))]
        ptrs = [b.ctypes.data_as(dp) if on else None for b, on in zip(bufs, outs)]
        xx = np.zeros((n_, t_))
        rc = lib.mpst_site_conditionals(eng.ctx, C.byref(m) if model else None, xx.ctypes.data_as(dp) if x_ else None,
                                        xs.ctypes.data_as(dp) if gx else None, C.c_void_p(gphi.ctypes.data) if gp else None, ngrid,
                                        C.byref(o), *ptrs, None)
        return rc, lib.mpst_last_error(eng.ctx).decode()

    for kw in (dict(model=False), dict(x_=False), dict(gx=False), dict(gp=False)):
        rc, msg = call(**kw)
        assert rc == INV and "NULL argument" in msg, (kw, rc, msg)
    rc, msg = call(outs=(0, 0, 0, 0, 0))
    assert rc == INV and "every output is NULL" in msg
    rc, msg = call(ngrid=1)
    assert rc == INV and "fewer than 2 grid values" in msg
    rc, msg = call(levels=np.linspace(0.05, 0.95, 17))
    assert rc == INV and "nq must lie in 0 .. 16" in msg
    for bad in ((0.5, 1.0), (0.0,), (-0.2, 0.5)):
        rc, msg = call(levels=bad)
        assert rc == INV and "is not inside (0, 1)" in msg
    rc, msg = call(outs=(1, 1, 1, 1, 0))
    assert rc == INV and "nq > 0 needs levels[nq] and q_out" in msg
    rc, msg = call(lab_=None)
    assert rc == INV and "label_idx is NULL" in msg
    for badlab in (np.array([0, 1, 2, 0, 1]), np.array([0, -1, 0, 1, 1])):
        rc, msg = call(lab_=badlab)
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
        assert rc == UNS and "site conditionals hold chi_max <= 128" in msg, (rc, msg)
    Wb = gaussian_chain(5, 16, 129, 1, 2, False, rng)            # (bond dimensions 1, 16, 129, 129, 16, 1)
    rc, msg = call(W_=Wb, phi_=random_states(2, 5, 16, False, rng), lab_=np.zeros(2))
    assert rc == UNS and "site conditionals hold chi_max <= 128" in msg, (rc, msg)
    with pytest.raises(mt.MPSTError) as ei:
        eng.site_conditionals(W, phi, lab, x, xs, gphi, compute="f32")
    assert ei.value.code == UNS
    after = eng.site_conditionals(W, phi, lab, x, xs, gphi, levels=LEVELS)
    assert all(np.array_equal(a, b) for a, b in zip(before[:5], after[:5]))
    check(after, ref, "after the refusals")
