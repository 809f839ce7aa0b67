"""mpst_observed_conditionals on the device against the NumPy restatement (tests/observed_ref.py, pinned to the dense amplitude tensor
and an extended-precision walk by tests/test_observed_host.py), against mpst_marginal_conditionals where the two questions coincide,
block by block and row by row, its refusals, and end to end through the Python layer.

Bounds (not from what the kernels give):
* operators: per entry (ngrid + 8) 2^-52 sum_k w_k k_k |g_k[s]| |g_k[s']| - the worst case of a sum of ngrid rounded terms in any
  order plus the ulps of exp - on the real and on the imaginary part;
* walk and grid, the restatement fed the device's own E_out so that the operators' rounding does not leak in: |nll_obs - ref| <= 1e-10,
  |pit - ref| <= 1e-12, both means 1e-12 max|grid_x|; median, WMAD and every level of both groups EQUAL wherever the
  restatement's selection margin exceeds 1e-9, at most 1 % of a case's pairs excused by it; logev 1e-10 (logarithms of
  traces), at T = 1000 the larger of that and four times the restatement's own distance from the longdouble walk.
phi is NaN wherever the call must not read it.

Largest deviations found on the MI355X: operators 4.7 % of their bound; nll_obs 2.9e-13, pit 3.0e-14, means 2.3e-14, logev 2.1e-13
(T = 1000: 1.1e-13, the restatement itself 1.2e-12 off the longdouble walk); one pair in 170 excused at most (the one narrow interval
of a case), 10 of 2000 at T = 1000."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import marginal
from mpstime_jl_amd import observations as ob
from tests import margcond_ref as M
from tests import observed_ref as O

pytestmark = pytest.mark.gpu

NLL_TOL, PIT_TOL, MEAN_TOL, LOGEV_TOL = 1e-10, 1e-12, 1e-12, 1e-10
LEVELS = O.LEVELS


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


def run(eng, inp, levels=LEVELS, **kw):
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    return eng.observed_conditionals(W, phi, lab, mt.ObservationModel(kind, a, b, E_user), x_in, xs, gp, levels=levels, return_operators=True, **kw)


_RESULTS = {}


def device_and_reference(eng, spec):
    """(inputs, device result, restatement on the device's own operators) of a committed case - computed once, never modified"""
    if spec not in _RESULTS:
        shape, cx, label, ngrid, per_site = spec
        inp = O.case(*shape, cx, label, ngrid, per_site)
        W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
        out = run(eng, inp)
        ref = O.observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x_in, xs, gp, LEVELS, E_given=out.operators)
        _RESULTS[spec] = (inp, out, ref)
    return _RESULTS[spec]


def spec_id(s):
    return f"{'-'.join(map(str, s[0]))}-{'cx' if s[1] else 're'}-{s[2]}-{s[3]}{'-persite' if s[4] else ''}"


@pytest.mark.parametrize("spec", O.gpu_cases(), ids=spec_id)
def test_operators(eng, spec):
    inp, out, _ = device_and_reference(eng, spec)
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    N, T = kind.shape
    d = W[0].shape[1]
    worst = 0.0
    for i in range(N):
        for t in range(T):
            k, E = int(kind[i, t]), out.operators[i, t]
            g = gp[t] if gp.ndim == 3 else gp
            if k == O.MISSING:
                assert np.array_equal(E, np.eye(d))
            elif k == O.OPERATOR:
                assert np.array_equal(E, E_user[i, t])
            elif k == O.EXACT:
                ref = np.outer(phi[i, t], np.conj(phi[i, t]))
                bound = 4 * 2.0 ** -52 * np.outer(np.abs(phi[i, t]), np.abs(phi[i, t]))      # a product of two numbers (four real products and a sum when complex)
                assert np.all(np.abs((E - ref).real) <= bound) and np.all(np.abs((E - ref).imag) <= bound), (i, t)
            else:
                ref, bound = O.operator_quadrature(k, a[i, t], b[i, t], xs, g)
                err = np.maximum(np.abs((E - ref).real), np.abs((E - ref).imag))
                assert np.all(err <= bound), (i, t, k, float((err / np.maximum(bound, 1e-300)).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{spec_id(spec)}: operators at most {worst:.3e} of their bound")


def check(inp, out, ref, what, logev_tol=LOGEV_TOL):
    """the restatement decides alone first, then the device is compared"""
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    excused = ref.excused
    assert excused.mean() <= 0.01, (what, float(excused.mean()))
    soft = kind >= O.GAUSS
    nll_nan = (kind == O.MISSING) & ~np.isfinite(x_in)
    pit_nan = soft | nll_nan
    post_nan = (kind == O.EXACT) | (kind == O.OPERATOR)
    with np.errstate(invalid="ignore"):
        dn = float(np.abs(np.where(out.nll_obs == ref.pred.nll, 0.0, out.nll_obs - ref.pred.nll))[~nll_nan].max()) if (~nll_nan).any() else 0.0
    dp = float(np.abs(out.pit - ref.pred.pit)[~pit_nan].max()) if (~pit_nan).any() else 0.0
    dm = float(np.abs(out.pred_mean - ref.pred_mean).max())
    dq = float(np.abs(out.post_mean - ref.post_mean)[~post_nan].max()) if (~post_nan).any() else 0.0
    dl = float(np.abs(out.logev - ref.logev).max())
    print(f"{what}: |nll_obs - ref| = {dn:.3e} (bound {NLL_TOL:g}), |pit - ref| = {dp:.3e} (bound {PIT_TOL:g}), |pred mean - ref| = {dm:.3e}, "
          f"|post mean - ref| = {dq:.3e} (bound {MEAN_TOL * np.abs(xs).max():g}), |logev - ref| = {dl:.3e} (bound {logev_tol:g}), "
          f"excused {int(excused.sum())} of {excused.size}")
    assert np.array_equal(np.isnan(out.nll_obs), nll_nan), np.argwhere(np.isnan(out.nll_obs) != nll_nan)
    assert np.array_equal(np.isnan(out.pit), pit_nan), np.argwhere(np.isnan(out.pit) != pit_nan)
    for v in (out.pred_median, out.pred_err, out.pred_mean, out.pred_quantiles, out.logev):
        assert np.all(np.isfinite(v))
    for v in (out.post_median, out.post_err, out.post_mean, out.post_quantiles.min(axis=2)):
        assert np.array_equal(np.isnan(v), post_nan), np.argwhere(np.isnan(v) != post_nan)
    sel = ~excused
    for dev, want in ((out.pred_median, ref.pred.median), (out.pred_err, ref.pred.err), (out.pred_quantiles, ref.pred.quantiles),
                      (out.post_median, ref.post.median), (out.post_err, ref.post.err), (out.post_quantiles, ref.post.quantiles)):
        assert np.array_equal(dev[sel], want[sel], equal_nan=True), np.argwhere((dev != want) & ~np.isnan(want) & (sel if dev.ndim == 2 else sel[:, :, None]))
    assert np.array_equal(out.pred_quantiles[:, :, 1], out.pred_median)         # level 0.5 is the median
    miss = kind == O.MISSING
    assert np.array_equal(out.post_median[miss], out.pred_median[miss]) and np.array_equal(out.post_mean[miss], out.pred_mean[miss])
    assert np.array_equal(out.post_quantiles[miss], out.pred_quantiles[miss]) and np.array_equal(out.post_err[miss], out.pred_err[miss])
    assert dn <= NLL_TOL and dp <= PIT_TOL and dm <= MEAN_TOL * np.abs(xs).max() and dq <= MEAN_TOL * np.abs(xs).max()
    assert dl <= logev_tol


@pytest.mark.parametrize("spec", O.gpu_cases(), ids=spec_id)
def test_walk_and_grid_against_the_restatement(eng, spec):
    inp, out, ref = device_and_reference(eng, spec)
    tol = LOGEV_TOL
    if spec[0] == O.LONG:
        dist = O.long_logev_distance(spec[1])
        tol = max(LOGEV_TOL, 4 * dist)
        print(f"T = 1000: the restatement is {dist:.3e} off the longdouble walk")
    check(inp, out, ref, spec_id(spec), tol)


# ---- cross-checks on the device ----
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_exact_and_missing_kinds_are_mpst_marginal_conditionals(eng, cx):
    W, phi, lab, miss, x_in, xs, gp, x = M.make_case(9, 4, 7, 2, 19, 9000 + (1 if cx else 0), cx=cx, label_site=4, ngrid=201)
    mref = M.marginal_conditionals_ref(W, phi, lab, miss, x_in, xs, gp, LEVELS)
    assert mref.excused.mean() <= 0.01
    mc = eng.marginal_conditionals(W, phi, lab, miss, x_in, xs, gp, levels=LEVELS)
    z = np.zeros(x_in.shape)
    out = eng.observed_conditionals(W, phi, lab, mt.ObservationModel(miss.astype(np.uint8), z, z), x_in, xs, gp, levels=LEVELS)
    with np.errstate(invalid="ignore"):
        dn = np.nanmax(np.abs(np.where(out.nll_obs == mc.nll, 0.0, out.nll_obs - mc.nll)))
        dp = np.nanmax(np.abs(out.pit - mc.pit))
    dm = np.abs(out.pred_mean - mc.mean).max()
    print(f"|nll_obs - nll| = {dn:.3e}, |pit - pit| = {dp:.3e}, |mean - mean| = {dm:.3e}")
    assert np.array_equal(np.isnan(out.nll_obs), np.isnan(mc.nll)) and np.array_equal(np.isnan(out.pit), np.isnan(mc.pit))
    assert dn <= NLL_TOL and dp <= PIT_TOL and dm <= MEAN_TOL * np.abs(xs).max()
    sel = ~mref.excused
    assert np.array_equal(out.pred_median[sel], mc.median[sel]) and np.array_equal(out.pred_err[sel], mc.err[sel])
    assert np.array_equal(out.pred_quantiles[sel], mc.quantiles[sel])
    # kind NULL: every site EXACT - the leave-one-out conditionals of the complete series
    ph = np.asarray(mt.model_encoding("Fourier" if cx else "Legendre_No_Norm").encode(x.ravel(), 4)).reshape(phi.shape)
    full = eng.marginal_conditionals(W, ph, lab, None, x, xs, gp, levels=LEVELS)
    m, keep = marginal.model_struct(W, ph, "f64")
    labs = np.ascontiguousarray(lab, dtype=np.int32)
    m.label_idx = labs.ctypes.data_as(C.POINTER(C.c_int32))
    dp_ = C.POINTER(C.c_double)
    nll, lev = np.zeros(x.shape), np.zeros(len(lab))
    o = mt._lib.SiteCondOpts(0, 0, 0, 0, None)
    outs = mt._lib.ObservedOut(nll_obs=nll.ctypes.data_as(dp_), logev=lev.ctypes.data_as(dp_))
    gpc = np.ascontiguousarray(gp)
    rc = eng.lib.mpst_observed_conditionals(eng.ctx, C.byref(m), None, None, None, None, None, xs.ctypes.data_as(dp_), C.c_void_p(gpc.ctypes.data),
                                            len(xs), C.byref(o), C.byref(outs), None)
    assert rc == 0, eng.lib.mpst_last_error(eng.ctx).decode()
    assert np.abs(nll - full.nll).max() <= NLL_TOL
    lm, _ = marginal.marginal_model(eng, W, ph, None)
    assert np.abs(lev - lm[np.arange(len(lab)), lab]).max() <= LOGEV_TOL          # logev of a complete series: ln |<phi|W_c>|^2


def test_an_interval_of_one_grid_value_is_not_an_exact_site(eng):
    """a == b on a grid value: the operator is w_k g_k g_k^H from the TABLE, the posterior sits on that value; an EXACT site would use
    the encoded state and give no posterior"""
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = O.case(9, 4, 7, 2, 19)
    kind, a, b = kind.copy(), a.copy(), b.copy()
    kind[6, 3], a[6, 3], b[6, 3] = O.INTERVAL, xs[77], xs[77]
    out = eng.observed_conditionals(W, phi, lab, mt.ObservationModel(kind, a, b, E_user), x_in, xs, gp, levels=LEVELS, return_operators=True)
    want = (xs[1] - xs[0]) * np.outer(gp[77], np.conj(gp[77]))
    assert np.abs(out.operators[6, 3] - want).max() <= 4 * 2.0 ** -52 * np.abs(want).max()
    assert out.post_median[6, 3] == xs[77] and np.isfinite(out.nll_obs[6, 3]) and np.isnan(out.pit[6, 3])


@pytest.mark.parametrize("spec", [((9, 4, 7, 2, 19), False, "last", 201, False), ((10, 3, 12, 3, 17), True, "last", 201, False),
                                  ((6, 4, 72, 2, 5), False, "last", 201, False)], ids=spec_id)
def test_an_operator_site_fed_a_gauss_operator_acts_as_that_site(eng, spec):
    inp, out, ref = device_and_reference(eng, spec)
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    g = kind == O.GAUSS
    assert g.any()
    kind2, E2 = np.where(g, O.OPERATOR, kind).astype(np.uint8), np.array(E_user)
    E2[g] = out.operators[g]
    alt = eng.observed_conditionals(W, phi, lab, mt.ObservationModel(kind2, a, b, E2), x_in, xs, gp, levels=LEVELS)
    fin = np.isfinite(out.nll_obs)
    dn, dl = np.abs(alt.nll_obs - out.nll_obs)[fin].max(), np.abs(alt.logev - out.logev).max()
    dm = np.abs(alt.pred_mean - out.pred_mean).max()
    print(f"operator for gauss: |nll_obs| {dn:.3e}, |logev| {dl:.3e}, |pred mean| {dm:.3e}")
    assert dn <= NLL_TOL and dl <= LOGEV_TOL and dm <= MEAN_TOL * np.abs(xs).max()
    sel = ~ref.excused
    assert np.array_equal(alt.pred_median[sel], out.pred_median[sel]) and np.array_equal(alt.pred_quantiles[sel], out.pred_quantiles[sel])
    assert np.array_equal(alt.post_median[sel & ~g], out.post_median[sel & ~g], equal_nan=True) and np.all(np.isnan(alt.post_median[g]))


# ---- invariance ----
FIELDS = ("pred_median", "pred_err", "pred_mean", "pred_quantiles", "post_median", "post_err", "post_mean", "post_quantiles", "nll_obs", "pit",
          "logev", "operators")


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(getattr(a, f)[rows_a], getattr(b, f)[rows_b], equal_nan=True) for f in FIELDS)


def _tiled(inp, reps):
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    t2 = lambda v: np.tile(v, (reps, 1))
    return W, np.tile(phi, (reps, 1, 1)), np.tile(lab, reps), t2(kind), t2(a), t2(b), np.tile(E_user, (reps, 1, 1, 1)), t2(x_in), xs, gp


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_blocks_do_not_change_the_result(eng, monkeypatch, cx):
    """N = 136 at (10 * (144 + 18 + 14) + 1) * 8 = 14 088 bytes per instance (complex: 27 048) under a scratch budget of 1 MB: blocks of
    76 (complex: 39) instances, the same bits as one block"""
    inp = _tiled(O.case(10, 3, 12, 3, 17, cx), 8)
    one = run(eng, inp)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    two = run(eng, inp)
    assert same_bits(one, two)
    assert same_bits(one, one, slice(0, 17), slice(119, 136))           # the replicas: what travels along does not matter


@pytest.mark.parametrize("shape,cx", [((9, 4, 7, 2, 19), False), ((10, 3, 12, 3, 17), True), ((6, 4, 72, 2, 5), False)],
                         ids=["lds-real", "lds-complex", "global-scratch"])
def test_rows_do_not_depend_on_their_neighbours(eng, shape, cx):
    inp = O.case(*shape, cx)
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    full = run(eng, inp)
    for i in range(0, kind.shape[0], 3):
        s = slice(i, i + 1)
        alone = run(eng, (W, phi[s], lab[s], kind[s], a[s], b[s], E_user[s], x_in[s], xs, gp))
        assert same_bits(alone, full, slice(None), s), i


# ---- refusals ----
def test_refusals_leave_the_context_as_it_was(eng):
    inp = O.case(9, 4, 7, 2, 19)
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = inp
    before = run(eng, inp)
    lib, dp = eng.lib, C.POINTER(C.c_double)
    INV, UNS = mt._lib.MPST_ERR_INVALID, mt._lib.MPST_ERR_UNSUPPORTED
    safe = np.where(np.isnan(phi), 0.0, phi)
    N, T = kind.shape
    ALL = ("pred_med", "pred_err", "pred_mean", "pred_q", "post_med", "post_err", "post_mean", "post_q", "nll_obs", "pit", "logev")

    def call(model=True, kind_=kind, a_=a, b_=b, E_=E_user, x_=True, gx=True, gp_=True, opt=True, out=True, ngrid=len(xs), outs=ALL, W_=W, phi_=safe,
             lab_=lab, compute="f64", levels=LEVELS, gps=0):
        m, keep = marginal.model_struct(W_, phi_, compute)
        labs = None if lab_ is None else np.ascontiguousarray(lab_, dtype=np.int32)
        m.label_idx = None if labs is None else labs.ctypes.data_as(C.POINTER(C.c_int32))
        lv = np.ascontiguousarray(levels, dtype=np.float64)
        o = mt._lib.SiteCondOpts(gps, 1, len(lv), 0, lv.ctypes.data_as(dp))
        n_, t_ = phi_.shape[:2]
        bufs = {k: np.zeros((n_, t_, max(1, len(lv)))) for k in ALL}
        oo = mt._lib.ObservedOut(**{k: bufs[k].ctypes.data_as(dp) for k in outs})
        k8 = None if kind_ is None else np.ascontiguousarray(np.resize(kind_, (n_, t_)), dtype=np.uint8)
        aa = None if a_ is None else np.ascontiguousarray(np.resize(a_, (n_, t_)), dtype=np.float64)
        bb = None if b_ is None else np.ascontiguousarray(np.resize(b_, (n_, t_)), dtype=np.float64)
        ee = None if E_ is None else np.ascontiguousarray(np.nan_to_num(E_), dtype=np.float64)
        xx = np.zeros((n_, t_))
        rc = lib.mpst_observed_conditionals(eng.ctx, C.byref(m) if model else None, None if k8 is None else k8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            None if aa is None else aa.ctypes.data_as(dp), None if bb is None else bb.ctypes.data_as(dp),
                                            None if ee is None else C.c_void_p(ee.ctypes.data), xx.ctypes.data_as(dp) if x_ else None,
                                            xs.ctypes.data_as(dp) if gx else None, C.c_void_p(gp.ctypes.data) if gp_ else None, ngrid,
                                            C.byref(o) if opt else None, C.byref(oo) if out else None, None)
        return rc, lib.mpst_last_error(eng.ctx).decode()

    rc, msg = call()
    assert rc == 0, msg
    for kw in (dict(model=False), dict(gx=False), dict(gp_=False), dict(opt=False), dict(out=False)):
        rc, msg = call(**kw)
        assert rc == INV and "NULL argument" in msg, (kw, rc, msg)
    rc, msg = call(outs=())
    assert rc == INV and "every output is NULL" in msg
    rc, msg = call(x_=False)
    assert rc == INV and "pit needs the values x" in msg
    rc, msg = call(x_=False, outs=tuple(k for k in ALL if k != "pit"))
    assert rc == 0, msg
    rc, msg = call(outs=("logev",), levels=())
    assert rc == 0, msg
    rc, msg = call(ngrid=1)
    assert rc == INV and "fewer than 2 grid values" in msg
    rc, msg = call(levels=np.linspace(0.05, 0.95, 17))
    assert rc == INV and "nq must lie in 0 .. 16" in msg
    rc, msg = call(levels=(0.5, 1.0))
    assert rc == INV and "is not inside (0, 1)" in msg
    rc, msg = call(outs=("pred_med", "nll_obs"))
    assert rc == INV and "nq > 0 needs levels[nq] and q_out" in msg
    rc, msg = call(lab_=None)
    assert rc == INV and "label_idx is NULL" in msg
    rc, msg = call(lab_=np.where(np.arange(len(lab)) == 3, 2, lab))
    assert rc == INV and "out of range" in msg
    rc, msg = call(gps=2)
    assert rc == INV and "grid_per_site must be 0" in msg
    rc, msg = call(compute="f32")
    assert rc == UNS and "fp64 only" in msg
    # the refusals of this call
    i, t = np.argwhere(kind == O.GAUSS)[0]
    j, u = np.argwhere(kind == O.INTERVAL)[0]

    def edited(arr, at, val):
        out = np.array(arr)
        out[at] = val
        return out
    rc, msg = call(kind_=edited(kind, (7, 2), 5))
    assert rc == INV and "kind[7][2] = 5 is not one of MPST_OBS_*" in msg
    for bad in (0.0, -1.0, np.inf, np.nan):
        rc, msg = call(b_=edited(b, (i, t), bad))
        assert rc == INV and f"MPST_OBS_GAUSS at [{i}][{t}]" in msg, (bad, rc, msg)
    rc, msg = call(a_=edited(a, (i, t), np.nan))
    assert rc == INV and f"MPST_OBS_GAUSS at [{i}][{t}]" in msg
    rc, msg = call(a_=edited(a, (j, u), b[j, u] + 0.1))
    assert rc == INV and f"MPST_OBS_INTERVAL at [{j}][{u}]" in msg
    for arr, bad in (("a_", -np.inf), ("b_", np.inf), ("a_", np.nan)):
        rc, msg = call(**{arr: edited(a if arr == "a_" else b, (j, u), bad)})
        assert rc == INV and f"MPST_OBS_INTERVAL at [{j}][{u}]" in msg, (arr, bad, rc, msg)
    rc, msg = call(E_=None)
    assert rc == INV and "MPST_OBS_OPERATOR and E_user is NULL" in msg
    rc, msg = call(a_=None)
    assert rc == INV and "needs a and b" in msg
    rc, msg = call(kind_=None, a_=None, b_=None, E_=None)           # every site EXACT: nothing else is read
    assert rc == 0, msg
    rng = np.random.default_rng(3)
    from tests.marginal_ref import gaussian_chain, random_states
    for d_, C_ in ((2, 17), (17, 2)):
        Wb = gaussian_chain(3, d_, 2, C_, 2, False, rng)
        rc, msg = call(W_=Wb, phi_=random_states(2, 3, d_, False, rng), lab_=np.zeros(2), kind_=None, E_=None)
        assert rc == UNS and "observed conditionals hold chi_max <= 128" in msg, (rc, msg)
    Wb = gaussian_chain(5, 16, 129, 1, 2, False, rng)            # (bond dimensions 1, 16, 129, 129, 16, 1)
    rc, msg = call(W_=Wb, phi_=random_states(2, 5, 16, False, rng), lab_=np.zeros(2), kind_=None, E_=None)
    assert rc == UNS and "observed conditionals hold chi_max <= 128" in msg, (rc, msg)
    assert same_bits(before, run(eng, inp))


# ---- end to end through the Python layer ----
@functools.lru_cache(maxsize=None)
def _problem():
    rng = np.random.default_rng(31)
    X1, _ = mt.trendy_sine(7, 30, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(7, 30, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(30, dtype=np.int64), np.ones(30, dtype=np.int64)])
    p = rng.permutation(60)
    X, y = X[p], y[p]
    opts = mt.MPSOptions(encoding="Legendre_No_Norm", d=4, chi_max=8, nsweeps=2, verbosity=-1)
    trained, _, _ = mt.fitMPS(X[:52], y[:52], X[52:], y[52:], opts)
    return trained, mt.init_imputation_problem(trained, X[52:], y[52:], dx=0.01, verbosity=0)


def test_python_layer_end_to_end(eng):
    trained, imp = _problem()
    X = imp.X_test
    N, T = X.shape
    # the smallest raw sd every site can resolve: the grid spacing over the smallest slope of the transform
    slope = ob.encode_observations(imp, mt.gaussian_noise(X, 1.0)).model.b
    dx = imp.x_guess_range.xvals[1] - imp.x_guess_range.xvals[0]
    low = 1.0001 * dx / slope.min()
    near, bands = mt.denoise(imp, low, engine=eng)
    far, fbands = mt.denoise(imp, 50 * low, engine=eng)
    for ts, bd in ((near, bands), (far, fbands)):
        assert ts.shape == (N, T) and bd.shape == (N, T, 2) and np.all(np.isfinite(ts)) and np.all(np.isfinite(bd))
        assert np.all(bd[:, :, 0] <= ts) and np.all(ts <= bd[:, :, 1])
    dnear, dfar = np.abs(near - X).mean(), np.abs(far - X).mean()
    print(f"denoise: mean |x_hat - x| = {dnear:.4f} at sd {low:.4f}, {dfar:.4f} at sd {50 * low:.4f}")
    assert dnear < dfar
    assert (bands[:, :, 1] - bands[:, :, 0]).mean() < (fbands[:, :, 1] - fbands[:, :, 0]).mean()
    mean, _ = mt.denoise(imp, 5 * low, statistic="mean", quantiles=None, invert_transform=False, engine=eng)
    a_, b_ = -1.0, 1.0
    assert np.all((mean >= a_) & (mean <= b_))
    with pytest.raises(ValueError, match="pass the value as exact"):
        mt.denoise(imp, 0.01 * low, engine=eng)
    # sd 0 is an exact site and is kept
    sig = np.full((N, T), 5 * low)
    sig[:, 2] = 0.0
    part, _ = mt.denoise(imp, sig, engine=eng)
    assert np.abs(part[:, 2] - X[:, 2]).max() <= 1e-9 * max(1.0, np.abs(X).max())
    # observed_conditionals: a mixture in raw units
    model = mt.gaussian_noise(X, sig, missing_mask=np.arange(T)[None, :].repeat(N, 0) == 4)
    oc = mt.observed_conditionals(imp, model, quantiles=LEVELS, engine=eng)
    exact, miss, g = model.kind == ob.EXACT, model.kind == ob.MISSING, model.kind == ob.GAUSS
    assert np.all(np.isfinite(oc.nll_obs[~miss])) and np.all(np.isnan(oc.nll_obs[miss]))
    assert np.all(np.isnan(oc.post_median[exact])) and np.all(np.isfinite(oc.post_median[~exact]))
    assert np.array_equal(oc.post_median[miss], oc.pred_median[miss]) and np.all(np.isfinite(oc.pit[exact])) and np.all(np.isnan(oc.pit[~exact]))
    # the posterior of a noisy site is at least as narrow as its predictive distribution, on average
    assert (oc.post_quantiles[g][:, 2] - oc.post_quantiles[g][:, 0]).mean() <= (oc.pred_quantiles[g][:, 2] - oc.pred_quantiles[g][:, 0]).mean()
    # classification: all-EXACT kinds are classify; a posterior is a distribution
    every = mt.gaussian_noise(X, 0.0)
    assert np.array_equal(mt.classify_noisy(imp, every, engine=eng), mt.classify(trained, X, engine=eng))
    lp = mt.noisy_log_likelihoods(imp, every, engine=eng)
    lm = mt.log_marginals(trained, X, np.zeros((N, T), dtype=bool), engine=eng)
    assert lp.shape == (N, 2) and np.abs(lp - lm).max() <= 1e-10
    post = mt.noisy_class_posteriors(imp, mt.gaussian_noise(X, 5 * low), engine=eng)
    assert post.shape == (N, 2) and np.abs(post.sum(axis=1) - 1).max() <= 1e-12 and np.all(post >= 0)
    ln = mt.noisy_log_likelihoods(imp, every, normalise_classes=True, engine=eng)
    lmn = mt.log_marginals(trained, X, np.zeros((N, T), dtype=bool), normalise_classes=True, engine=eng)
    assert np.abs(ln - lmn).max() <= 1e-10
