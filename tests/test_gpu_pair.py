"""Pair analysis on the device (mpst_pair_analysis, csrc/mpst_analysis.hip: k_an_pair / k_an_pair_ent) through ctypes and the C
ABI, against the NumPy restatement in tests/pair_ref.py: ``brute_force`` (the dense state) where d^T is small, ``transfer`` (the
recursion as matrix products) beyond.  Tolerance 1e-10 on mi, mean and cov, the bound of the other analysis and query tests; the two
host forms differ by 2e-14.  Each case prints its largest deviation."""
import ctypes as C
import os

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import analysis
from tests import analysis_ref as A
from tests import pair_plan as PP
from tests import pair_ref as P
from tests.test_pair_ref import sym_obs, trained

pytestmark = pytest.mark.gpu

TOL = 1e-10
LN2 = float(np.log(2.0))
DP = C.POINTER(C.c_double)

CHI20 = (1, 4, 16, 20, 20, 20, 20, 20, 20, 20, 16, 4, 1)          # T = 12, d = 4: the second 16-column tile, state in LDS
CHI72 = (1, 72, 72, 72, 72, 72, 1)                                # T = 6, d = 2: state in global scratch
CHI40 = (1, 4, 16, 40, 40, 40, 40, 40, 40, 40, 16, 4, 1)          # T = 12, d = 4: global scratch, three tiles


@pytest.fixture(scope="module")
def engine():
    eng = mt.SweepEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return PP.build(tmp_path_factory.mktemp("pair_plan_gpu"))


def call(eng, W, obs=None, mi=True, mean=None, cov=None, per_site=None, struct=None):
    """The raw C call: (rc, mi, mean, cov, seconds).  mean / cov default to 'wherever there is an observable'."""
    m = analysis._Model(W)
    st = struct(m.struct) if struct else m.struct
    T, Cn = m.T, m.C
    mean = obs is not None if mean is None else mean
    cov = obs is not None if cov is None else cov
    o = None if obs is None else np.ascontiguousarray(obs, dtype=np.float64)
    a_mi = np.full((Cn, T, T), -7.0) if mi else None
    a_mean = np.full((Cn, T), -7.0) if mean else None
    a_cov = np.full((Cn, T, T), -7.0) if cov else None
    ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None
    sec = C.c_double()
    per_site = int(o is not None and o.ndim == 3) if per_site is None else per_site
    rc = eng.lib.mpst_pair_analysis(eng.ctx, C.byref(st), ptr(o), per_site, ptr(a_mi), ptr(a_mean), ptr(a_cov), C.byref(sec))
    return rc, a_mi, a_mean, a_cov, sec.value


def ok(eng, *a, **k):
    rc, mi, mean, cov, _ = call(eng, *a, **k)
    assert rc == 0, (rc, eng.lib.mpst_last_error(eng.ctx))
    return mi, mean, cov


def compare(name, got, ref, tol=TOL):
    worst = 0.0
    for g, r in zip(got, ref):
        if g is None:
            continue
        assert g.shape == r.shape
        worst = max(worst, float(np.abs(g - r).max()))
    print(f"{name}: largest deviation {worst:.2e}")
    assert worst <= tol, (name, worst)
    return worst


# ---- against the dense state ------------------------------------------------------------------------------------------------
BRUTE = {
    "base": ((1, 2, 4, 4, 3, 2, 1), 2, 2, None),
    "odd bonds, six blocks, label mid-chain": ((1, 3, 7, 7, 5, 3, 1), 3, 2, 2),
    "canon shrinks a bond": ((1, 5, 3, 1), 2, 2, 0),
    "T = 1": ((1, 1), 2, 2, None),
    "T = 2": ((1, 2, 1), 2, 2, None),
    "d = 11: a 121 x 121 Jacobi": ((1, 4, 4, 1), 11, 2, None),
}


@pytest.mark.parametrize("name", list(BRUTE))
def test_against_the_dense_state(name, engine):
    chi, d, Cn, label = BRUTE[name]
    W = P.chain_model(chi, d, Cn, label, seed=len(chi) + d)
    O = sym_obs(d, 5, T=len(chi) - 1)
    got, ref = ok(engine, W, O), P.brute_force(W, O)
    compare(name, got, ref)
    if len(chi) == 2:
        assert np.abs(got[0]).max() <= TOL              # one site: a pure state, mi = [[0]]


def test_product_state(engine):
    """All bonds 1: I = 0 and cov = 0 off the diagonal to 1e-12."""
    W = P.chain_model((1, 1, 1, 1), 3, 2, seed=9)
    mi, mean, cov = ok(engine, W, sym_obs(3, 2))
    compare("product state", (mi, mean, cov), P.brute_force(W, sym_obs(3, 2)))
    off = ~np.eye(3, dtype=bool)
    print("product state: max |I|", np.abs(mi).max(), "max |cov| off the diagonal", np.abs(cov[:, off]).max())
    assert np.abs(mi).max() <= 1e-12 and np.abs(cov[:, off]).max() <= 1e-12


def test_ghz_chain(engine):
    mi, mean, cov = ok(engine, P.ghz_model(5, C=2), np.diag([1.0, -1.0]))
    np.testing.assert_allclose(mi, LN2, atol=TOL, rtol=0)
    np.testing.assert_allclose(cov, 1.0, atol=TOL, rtol=0)
    np.testing.assert_allclose(mean, 0.0, atol=TOL, rtol=0)


def test_d_12_has_moments_but_no_mutual_information(engine):
    W = P.chain_model((1, 4, 4, 1), 12, 2, seed=3)
    O = sym_obs(12, 6)
    rc = call(engine, W, O)[0]
    assert rc == mt._lib.MPST_ERR_UNSUPPORTED and b"d <= 11" in engine.lib.mpst_last_error(engine.ctx)
    _, mean, cov = ok(engine, W, O, mi=False)
    ref = P.brute_force(W, O)
    compare("d = 12 moments", (mean, cov), ref[1:])
    with pytest.warns(RuntimeWarning, match="11"):
        r = mt.pair_analysis(trained(W), observable=O, engine=engine)
    assert r.mutual_information is None
    compare("d = 12 pair_analysis", (r.mean, r.covariance), ref[1:])


def test_d_16_moments(engine):
    W = P.chain_model((1, 4, 4, 1), 16, 2, seed=4)
    O = sym_obs(16, 7, T=3)
    _, mean, cov = ok(engine, W, O, mi=False)
    compare("d = 16 moments", (mean, cov), P.brute_force(W, O)[1:])


# ---- against the recursion on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chi20():
    W = P.chain_model(CHI20, 4, 3, 5, seed=20)
    O = sym_obs(4, 8, T=12)
    return W, O, P.transfer(W, O)


def test_second_column_tile_three_classes(chi20, engine, plan_exe):
    W, O, ref = chi20
    _, plans = PP.run(plan_exe, [PP.case(3, 12, 4, 20)])
    assert plans[PP.case(3, 12, 4, 20)]["lds"] == 1
    compare("chi = 20, T = 12, d = 4, C = 3", ok(engine, W, O), ref)


def test_state_in_global_scratch(engine, plan_exe):
    W = P.chain_model(CHI72, 2, 2, 3, seed=72)
    O = sym_obs(2, 9)
    _, plans = PP.run(plan_exe, [PP.case(2, 6, 2, 72)])
    assert plans[PP.case(2, 6, 2, 72)]["lds"] == 0
    got = ok(engine, W, O)
    compare("chi = 72, T = 6, d = 2 (transfer)", got, P.transfer(W, O))
    compare("chi = 72, T = 6, d = 2 (brute force)", got, P.brute_force(W, O))


def test_properties(chi20, engine):
    W, O, _ = chi20
    mi, mean, cov = ok(engine, W, O)
    assert np.array_equal(mi, mi.transpose(0, 2, 1)) and np.array_equal(cov, cov.transpose(0, 2, 1))
    # the partial trace of rho_ij, through the moments: with O_j = 1 the pair moment is mean_i, so every covariance vanishes
    Oid = np.broadcast_to(np.eye(4), (12, 4, 4)).copy()
    _, m1, c1 = ok(engine, W, Oid, mi=False)
    print("identity observable: max |cov|", np.abs(c1).max(), "max |mean - 1|", np.abs(m1 - 1).max())
    assert np.abs(c1).max() <= 1e-12 and np.abs(m1 - 1.0).max() <= 1e-12
    mixed = O.copy()
    mixed[1::2] = np.eye(4)                     # O_j = 1 on the odd sites only: cov[i][j] = 0 wherever one of the two is odd
    _, _, c2 = ok(engine, W, mixed, mi=False)
    odd = np.zeros((12, 12), dtype=bool)
    odd[1::2, :] = True
    odd[:, 1::2] = True
    assert np.abs(c2[:, odd]).max() <= 1e-12 and np.abs(c2[:, ~odd]).max() > 1e-6
    # 0 <= I(i:j) <= 2 min(S_i, S_j)
    S = np.diagonal(mi, axis1=1, axis2=2)
    off = ~np.eye(12, dtype=bool)
    upper = 2.0 * np.minimum(S[:, :, None], S[:, None, :])
    assert np.all(mi[:, off] >= -TOL) and np.all((mi <= upper + TOL)[:, off])


def test_diagonal_is_single_site_spectrum_where_rho_correct_is_a_no_op(chi20, engine):
    W, _, _ = chi20
    mins = []
    A.single_site_spectrum(W, mins)
    assert min(float(m.min()) for m in mins) > 1e-8
    mi, _, _ = ok(engine, W)
    see = mt.single_site_spectrum(trained(W), engine=engine)
    for c in range(3):
        np.testing.assert_allclose(np.diagonal(mi[c]), see[c], atol=TOL, rtol=0)


def test_blocks_and_placement_do_not_change_the_bits(engine, plan_exe, monkeypatch):
    """MPST_IMPUTE_CHUNK_GB = 0.001 cuts the stored rho_ij into blocks and lowers the workgroup cap (both asserted through the
    plan); mi, mean and cov are the same bits as without it."""
    W = P.chain_model(CHI40, 4, 2, 11, seed=40)
    O = sym_obs(4, 10, T=12)
    small, full = PP.case(2, 12, 4, 40, override="0.001"), PP.case(2, 12, 4, 40)
    _, plans = PP.run(plan_exe, [small, full])
    assert len(plans[small]["row0"]) - 1 >= 2 and plans[small]["workgroups"] < plans[full]["workgroups"] == 24
    assert plans[small]["lds"] == 0
    monkeypatch.delenv("MPST_IMPUTE_CHUNK_GB", raising=False)
    a = ok(engine, W, O)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    b = ok(engine, W, O)
    monkeypatch.delenv("MPST_IMPUTE_CHUNK_GB")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    compare("chi = 40, T = 12, d = 4", a, P.transfer(W, O))


def test_observable_forms(engine):
    W = P.chain_model((1, 3, 7, 7, 5, 3, 1), 3, 2, 2, seed=9)
    O = sym_obs(3, 1)
    a = ok(engine, W, O)
    b = ok(engine, W, np.broadcast_to(O, (6, 3, 3)).copy())
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    Os = sym_obs(3, 2, T=6)
    compare("per-site observable", ok(engine, W, Os), P.brute_force(W, Os))
    # outputs one at a time give the bits of the full call
    full = ok(engine, W, Os)
    assert np.array_equal(ok(engine, W, Os, mi=False, cov=False)[1], full[1])
    assert np.array_equal(ok(engine, W, Os, mi=False, mean=False)[2], full[2])
    assert np.array_equal(ok(engine, W)[0], full[0])


def test_zero_class_gives_nan_in_its_slices_only(engine):
    W = P.chain_model((1, 2, 4, 2, 1), 2, 2, 1, seed=5)
    O = sym_obs(2, 3)
    ref = ok(engine, W, O)
    W[1][..., 1] = 0.0
    got = ok(engine, W, O)
    for g, r in zip(got, ref):
        assert np.all(np.isnan(g[1])) and np.array_equal(g[0], r[0])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_as_it_was(engine):
    W = P.chain_model((1, 2, 4, 4, 3, 2, 1), 2, 2, seed=1)
    O = sym_obs(2, 4)
    lib, INV, UNS = engine.lib, mt._lib.MPST_ERR_INVALID, mt._lib.MPST_ERR_UNSUPPORTED
    fresh = mt.SweepEngine(0)
    try:
        want = ok(fresh, W, O)
    finally:
        fresh.close()
    err = lambda: lib.mpst_last_error(engine.ctx).decode()
    assert call(engine, W, O, mi=False, mean=False, cov=False)[0] == INV and "NULL" in err()
    assert call(engine, W, None, mean=True)[0] == INV and "observable" in err()
    assert call(engine, W, None, mi=False, cov=True)[0] == INV
    assert call(engine, W, O, per_site=2)[0] == INV and "obs_per_site" in err()
    assert call(engine, W, O, per_site=-1)[0] == INV

    def complex_dtype(st):
        st.dtype = 1
        return st
    assert call(engine, W, O, struct=complex_dtype)[0] == UNS and "complex" in err()

    def f32(st):
        st.compute = 1
        return st
    assert call(engine, W, O, struct=f32)[0] == UNS

    def bad_chain(st):
        st.chi[0] = 2
        return st
    assert call(engine, W, O, struct=bad_chain)[0] == INV and "chi[0] and chi[T] must be 1" in err()
    with pytest.raises(ValueError, match="complex"):
        mt.pair_analysis(trained([t.astype(np.complex128) for t in W]), observable=O, engine=engine)
    got = ok(engine, W, O)
    for g, r in zip(got, want):
        assert np.array_equal(g, r)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    rng = np.random.default_rng(7)
    X1, _ = mt.trendy_sine(10, 24, period=(4.0, 5.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(10, 24, period=(6.0, 7.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
    tm, _, _ = mt.fitMPS(np.concatenate([X1, X2]), np.repeat([0, 1], 24), opts=mt.MPSOptions(d=4, chi_max=8, nsweeps=2, eta=0.05, verbosity=-1))
    return tm


def test_python_layer(fitted, engine):
    r, sec = mt.pair_analysis(fitted, engine=engine, return_seconds=True)
    X = mt.position_operator(fitted)
    assert X.shape == (10, 4, 4) and sec > 0.0
    mi, mean, cov = P.transfer(fitted.mps, X)
    compare("fitted model", (r.mutual_information, r.mean, r.covariance), (mi, mean, cov))
    r2 = mt.pair_analysis(fitted, logfn="log2", engine=engine)
    np.testing.assert_allclose(r2.mutual_information, r.mutual_information / np.log(2.0), rtol=1e-14)
    assert np.array_equal(r2.covariance, r.covariance)
    var = np.diagonal(r.covariance, axis1=1, axis2=2)
    diag = np.diagonal(r.correlation, axis1=1, axis2=2)
    assert np.all(var > 0.0)
    np.testing.assert_allclose(diag, 1.0, rtol=0, atol=1e-12)
    sd = np.sqrt(var)
    np.testing.assert_allclose(r.correlation, r.covariance / (sd[:, :, None] * sd[:, None, :]), rtol=1e-14)
    assert np.all(np.abs(r.correlation) <= 1.0 + 1e-9)
    none = mt.pair_analysis(fitted, observable=None, engine=engine)
    assert none.mean is None and none.covariance is None and none.correlation is None
    assert np.array_equal(none.mutual_information, r.mutual_information)
    ml = mt.mutual_information(fitted, engine=engine)
    assert len(ml) == 2 and np.array_equal(ml[0], r.mutual_information[0])
    means, corr = mt.model_correlations(fitted, engine=engine)
    assert np.array_equal(means[1], r.mean[1]) and np.array_equal(corr[1], r.correlation[1], equal_nan=True)
    with pytest.raises(ValueError, match="logfn"):
        mt.pair_analysis(fitted, logfn="ln", engine=engine)


def test_correlation_is_nan_where_a_variance_is_not_positive():
    cov = np.array([[[4.0, 2.0], [2.0, 0.0]]])
    c = analysis._correlation(cov)
    assert c[0, 0, 0] == 1.0 and np.isnan(c[0, 0, 1]) and np.isnan(c[0, 1, 1])
