"""mpst_window_conditionals on the device against the window-local form of the NumPy restatement (tests/window_ref.py, which
tests/test_window_host.py pins to the masked difference of marginal likelihoods and to the dense amplitude tensor), against the
existing device call on the window-masked replicas, row by row, block by block, through the Python layer, and its refusals.

Bound (the project's for fp64 log likelihoods against a NumPy restatement, tests/test_gpu_marginal.py and tests/test_gpu_site_cond.py,
not taken from what the kernel gives): |nll - ref| < 1e-10 absolute; 2e-10 against the difference of two mpst_marginal_model results,
each of which has that bound.  NaN exactly where t + w > T."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import conditionals, marginal
from tests import window_ref as WR
from tests.marginal_ref import gaussian_chain, random_states

pytestmark = pytest.mark.gpu

NLL_TOL = 1e-10


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """(W, phi, lab, max_width, restatement) - built once, shared by the tests below, never modified"""
    W, phi, lab, mw = WR.make_case(name)
    ref = WR.window_nll_local(W, phi, lab, mw)
    for a in list(W) + [phi, lab, ref]:
        a.setflags(write=False)
    return W, phi, lab, mw, ref


def check(nll, ref, what):
    N, T, mw = ref.shape
    hole = WR.expected_nan(N, T, mw)
    assert nll.shape == ref.shape
    assert np.array_equal(np.isnan(ref), hole)
    dev = float(np.abs(nll[~hole] - ref[~hole]).max())
    print(f"{what}: largest |nll - ref| = {dev:.3e} over {int((~hole).sum())} windows (bound {NLL_TOL:g})")
    assert np.array_equal(np.isnan(nll), hole), np.argwhere(np.isnan(nll) != hole)[:5]
    assert np.all(np.isfinite(nll[~hole]))
    assert dev < NLL_TOL


@pytest.mark.parametrize("name", list(WR.SHAPES))
def test_against_the_restatement(eng, name):
    W, phi, lab, mw, ref = case(name)
    nll, secs = eng.window_conditionals(W, phi, lab, mw)
    check(nll, ref, name)
    walk, win = eng.impute_phases()
    assert secs > 0.0 and walk > 0.0 and win > 0.0


def test_against_marginal_likelihoods_of_the_masked_replicas(eng):
    """nll = mpst_marginal_model(window mask) - mpst_marginal_model(no mask) at the series' class; every window in one batched call"""
    W, phi, lab, mw, _ = case("second-tile")
    N, T = phi.shape[:2]
    nll, _ = eng.window_conditionals(W, phi, lab, mw)
    wins = [(i, t, w) for i in range(N) for t in range(T) for w in range(1, min(mw, T - t) + 1)]
    mask = np.zeros((len(wins) + N, T), dtype=np.uint8)
    for n, (i, t, w) in enumerate(wins):
        mask[n, t:t + w] = 1
    rows = np.array([i for i, _, _ in wins] + list(range(N)))
    logp, _ = eng.marginal_model(W, phi[rows], mask)
    full = logp[len(wins):][np.arange(N), lab]
    worst = 0.0
    for n, (i, t, w) in enumerate(wins):
        worst = max(worst, abs(nll[i, t, w - 1] - (logp[n, lab[i]] - full[i])))
    print(f"largest |nll - (marginal(masked) - marginal(complete))| = {worst:.3e} over {len(wins)} windows (bound {2 * NLL_TOL:g})")
    assert worst < 2 * NLL_TOL


@pytest.mark.parametrize("name", ["ragged-tile", "second-tile", "complex-mid", "big-real", "long-200"])
def test_invariants_on_unit_norm_states(eng, name):
    """Cauchy-Schwarz: every finite entry >= 0 and non-decreasing in the width, with 1e-10 for rounding"""
    W, phi, lab, mw, _ = case(name)
    nll, _ = eng.window_conditionals(W, phi, lab, mw)
    fin = np.isfinite(nll)
    assert np.all(nll[fin] >= -NLL_TOL)
    for w in range(1, mw):
        both = fin[:, :, w] & fin[:, :, w - 1]
        assert np.all(nll[:, :, w][both] >= nll[:, :, w - 1][both] - NLL_TOL)


def test_rows_do_not_depend_on_their_neighbours(eng):
    W, phi, lab, mw, _ = case("second-tile")
    full, _ = eng.window_conditionals(W, phi, lab, mw)
    for i in (0, 7, 15, 16, 18):
        one, _ = eng.window_conditionals(W, phi[i:i + 1], lab[i:i + 1], mw)
        assert one[0].tobytes() == full[i].tobytes(), i


def test_blocks_do_not_change_the_result(eng, monkeypatch):
    """N = 700 under a scratch budget of 1 MB: 1 073 741 / (12 * (2 * 12 + 5) * 8) = 385 fit, two blocks of 384 and 316 - the same bits
    as in one; and the last 60 series alone"""
    rng = np.random.default_rng(77)
    W = gaussian_chain(12, 4, 12, 2, 5, False, rng)
    phi = random_states(700, 12, 4, False, rng)
    lab = (np.arange(700) % 2).astype(np.int32)
    one, _ = eng.window_conditionals(W, phi, lab, 5)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    two, _ = eng.window_conditionals(W, phi, lab, 5)
    monkeypatch.delenv("MPST_IMPUTE_CHUNK_GB")
    assert one.tobytes() == two.tobytes()
    few, _ = eng.window_conditionals(W, phi[640:], lab[640:], 5)
    assert few.tobytes() == one[640:].tobytes()
    hole = WR.expected_nan(700, 12, 5)
    assert np.array_equal(np.isnan(one), hole)
    ref = WR.window_nll_local(W, phi[:3], lab[:3], 5)
    assert np.abs(one[:3][~hole[:3]] - ref[~hole[:3]]).max() < NLL_TOL


def test_degenerate_series(eng):
    """A series whose state at site 2 is zero has no amplitude.  The rows l~_{t-1}, t > 2, and r~_{t+1}, t < 2, of its walk are zero:
    a start behind site 2 has no x_0 (NaN for every width); a start before it closes its first width on a zero row (a closing form that
    is not positive: NaN, and NaN for the wider ones of the start); the start AT site 2 sums the site out - closing form positive,
    |x . r|^2 = 0: +inf for every width.  The other series do not notice."""
    W, phi, lab, mw, ref = case("ragged-tile")
    ph = np.array(phi)
    ph[1, 2] = 0.0
    nll, _ = eng.window_conditionals(W, ph, lab, mw)
    keep = [0, 2, 3, 4]
    assert nll[keep].tobytes() == eng.window_conditionals(W, phi, lab, mw)[0][keep].tobytes()
    T = ph.shape[1]
    assert np.all(np.isnan(nll[1, [0, 1, 3, 4, 5]]))
    assert np.all(np.isposinf(nll[1, 2, :T - 2])) and np.all(np.isnan(nll[1, 2, T - 2:]))


@pytest.fixture(scope="module")
def fitted():
    """a hist_split_legendre model (d = 4, aux_basis_dim = 2, T = 7) trained for two sweeps on trendy_sine data, N = 8 test series:
    (the trained model, the raw test series, their labels, the imputation problem)"""
    rng = np.random.default_rng(31)
    X1, _ = mt.trendy_sine(7, 30, period=(4.0, 6.0), slope=[-2.0, 0.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(7, 30, period=(8.0, 11.0), slope=[0.0, 2.0], sigma=0.1, rng=rng)
    X = np.concatenate([X1, X2])
    y = np.concatenate([np.zeros(30, dtype=np.int64), np.ones(30, dtype=np.int64)])
    p = rng.permutation(60)
    X, y = X[p], y[p]
    opts = mt.MPSOptions(encoding="hist_split_legendre", d=4, aux_basis_dim=2, chi_max=8, nsweeps=2, verbosity=-1)
    trained, _, _ = mt.fitMPS(X[:52], y[:52], X[52:], y[52:], opts)
    return trained, X[52:], y[52:], mt.init_imputation_problem(trained, X[52:], y[52:], dx=0.01, verbosity=0)


def test_through_the_python_layer(eng, fitted):
    trained, Xte, yte, imp = fitted
    out = mt.window_conditionals(imp, 4, engine=eng)
    assert out.x.shape == (8, 7) and out.nll.shape == (8, 7, 4)
    lab = np.array([imp.class_map[c] for c in yte.tolist()], dtype=np.int32)
    direct, _ = conditionals.window_conditionals_model(eng, imp.mps, np.asarray(imp.encoder(out.x)), lab, 4)
    assert out.nll.tobytes() == direct.tobytes()
    assert np.array_equal(np.isnan(out.nll), WR.expected_nan(8, 7, 4))
    ref = WR.window_nll_local(imp.mps, np.asarray(imp.encoder(out.x)), lab, 4)
    ok = ~np.isnan(ref)
    assert np.abs(out.nll[ok] - ref[ok]).max() < NLL_TOL
    sub = mt.window_conditionals(imp, 4, rows=[1, 4], engine=eng)
    assert sub.nll.tobytes() == out.nll[[1, 4]].tobytes()
    # the scores are slices of the map
    for width in (1, 3, 4):
        prof = mt.window_anomaly_scores(imp, width, reduce=None, engine=eng)
        want = mt.window_conditionals(imp, width, engine=eng).nll[:, :7 - width + 1, width - 1]
        assert prof.shape == (8, 7 - width + 1) and prof.tobytes() == want.tobytes()
        assert np.array_equal(prof, out.nll[:, :7 - width + 1, width - 1])
        assert np.array_equal(mt.window_anomaly_scores(imp, width, engine=eng), want.max(axis=1))
        assert np.array_equal(mt.window_anomaly_scores(imp, width, reduce="mean", engine=eng), want.mean(axis=1))
        assert np.array_equal(mt.window_anomaly_scores(imp, width, per_site=True, reduce=None, engine=eng), want / width)
    empty = mt.window_conditionals(imp, 2, rows=np.array([], dtype=np.int64), engine=eng)
    assert empty.x.shape == (0, 7) and empty.nll.shape == (0, 7, 2)
    with pytest.raises(KeyError):
        mt.window_conditionals(mt.init_imputation_problem(trained, Xte, yte + 5, dx=0.01, verbosity=0), 2, engine=eng)


def test_refusals_by_message_leave_the_context_as_it_was(eng):
    W, phi, lab, mw, ref = case("ragged-tile")
    before, _ = eng.window_conditionals(W, phi, lab, mw)
    lib, dp = eng.lib, C.POINTER(C.c_double)
    INV, UNS = mt._lib.MPST_ERR_INVALID, mt._lib.MPST_ERR_UNSUPPORTED

    def call(model=True, out=True, width=mw, W_=W, phi_=phi, lab_=lab, compute="f64"):
        m, keep = marginal.model_struct(W_, phi_, compute)
        labs = None if lab_ is None else np.ascontiguousarray(lab_, dtype=np.int32)
        m.label_idx = None if labs is None else labs.ctypes.data_as(C.POINTER(C.c_int32))
        n_, t_ = phi_.shape[:2]
        buf = np.zeros((n_, t_, max(1, width)))
        rc = lib.mpst_window_conditionals(eng.ctx, C.byref(m) if model else None, width, buf.ctypes.data_as(dp) if out else None, None)
        return rc, lib.mpst_last_error(eng.ctx).decode()

    T = phi.shape[1]
    for bad in (0, T + 1, -3):
        rc, msg = call(width=bad)
        assert rc == INV and f"max_width must lie in 1 .. T = {T}" in msg, (bad, rc, msg)
    for kw in (dict(model=False), dict(out=False)):
        rc, msg = call(**kw)
        assert rc == INV and "NULL argument" in msg, (kw, rc, msg)
    rc, msg = call(lab_=None)
    assert rc == INV and "label_idx is NULL" in msg
    for badlab in (np.array([0, 1, 2, 0, 1]), np.array([0, -1, 0, 1, 1])):
        rc, msg = call(lab_=badlab)
        assert rc == INV and "out of range" in msg
    rc, msg = call(compute="f32")
    assert rc == UNS and "fp64 only" in msg
    rng = np.random.default_rng(3)
    for d_, C_ in ((2, 17), (17, 2)):
        Wb = gaussian_chain(3, d_, 2, C_, 2, False, rng)
        rc, msg = call(W_=Wb, phi_=random_states(2, 3, d_, False, rng), lab_=np.zeros(2), width=1)
        assert rc == UNS and "window conditionals hold chi_max <= 128" in msg, (rc, msg)
    Wb = gaussian_chain(5, 16, 129, 1, 2, False, rng)            # (bond dimensions 1, 16, 129, 129, 16, 1)
    rc, msg = call(W_=Wb, phi_=random_states(2, 5, 16, False, rng), lab_=np.zeros(2), width=2)
    assert rc == UNS and "window conditionals hold chi_max <= 128" in msg, (rc, msg)
    with pytest.raises(mt.MPSTError) as ei:
        eng.window_conditionals(W, phi, lab, 0)
    assert ei.value.code == INV
    after, _ = eng.window_conditionals(W, phi, lab, mw)
    assert before.tobytes() == after.tobytes()
    check(after, ref, "after the refusals")
