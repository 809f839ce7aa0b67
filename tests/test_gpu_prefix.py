"""mpst_prefix_marginals on the device against the NumPy restatement (tests/prefix_ref.py: log_marginals_ref over the suffix masks),
against mpst_marginal_model at both ends, and end to end through prefix_posteriors / classify_early / causal_scores."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import marginal, prefix
from tests import marginal_ref as MR
from tests import prefix_ref as PR

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10         # the project's bound for ln l in fp64 (tests/test_gpu_marginal.py)
D, CN = 6, 3


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


def label_site(label, T):
    return {"last": T - 1, "mid": T // 2, "first": 0}[label]


@functools.lru_cache(maxsize=None)
def model(chi, cx, label, N, T, d=D, Cn=CN):
    """(W, phi) - built once, shared by the tests below, never modified"""
    rng = np.random.default_rng(2000 + 11 * chi + (1 if cx else 0) + 3 * label_site(label, T) + N)
    W = MR.gaussian_chain(T, d, chi, Cn, label_site(label, T), cx, rng, scale=1.0 / np.sqrt(d * chi))
    phi = MR.random_states(N, T, d, cx, rng)
    for a in W + [phi]:
        a.setflags(write=False)
    return W, phi


@functools.lru_cache(maxsize=None)
def restated(chi, cx, label, N, T):
    ref = PR.prefix_log_marginals_ref(*model(chi, cx, label, N, T))
    ref.setflags(write=False)
    return ref


# chi = 12: not a multiple of 16, three tiles of series, the last one partial; chi = 7: below one tile; chi = 72: beyond one 64-column
# wave tile and beyond the LDS route of the density recursion; chi = 128: the upper limit (at T = 4 and d = 6 the ends of the chain cap
# the bonds at 36: test_the_largest_bond has a chain whose middle bond is 128)
SHAPES = [(12, 37, 10), (7, 21, 10), (72, 3, 6), (128, 2, 4)]
SHAPE_IDS = ["chi12", "chi7", "chi72_big", "chi128"]


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("chi,N,T", SHAPES, ids=SHAPE_IDS)
def test_against_the_restatement(eng, chi, N, T, cx, label):
    W, phi = model(chi, cx, label, N, T)
    ref = restated(chi, cx, label, N, T)
    got, _ = eng.prefix_model(W, phi)
    assert got.shape == (N, T + 1, CN)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    err = np.abs(got - ref).max()
    print(f"chi={chi} cx={cx} label={label}: largest |d ln l| = {err:.3e}")
    assert err <= F64_TOL


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_the_largest_bond(eng, cx, label):
    """chi = 128 at T = 6: bonds 1, 6, 36, 128, 36, 6, 1.  One series, and the restatement at the prefix lengths 0, 3 (the row and the
    table of the 128-bond), 4 and T only: the NumPy density steps through that bond take a second each."""
    W, phi = model(128, cx, label, 1, 6)
    assert max(t.shape[2] for t in W) == 128
    lengths = [0, 3, 4, 6]
    ref = PR.prefix_log_marginals_ref(W, phi, lengths)
    got, _ = eng.prefix_model(W, phi)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    err = np.abs(got[:, lengths] - ref).max()
    print(f"chi=128 T=6 cx={cx} label={label}: largest |d ln l| = {err:.3e}")
    assert err <= F64_TOL
    assert np.all(got[:, 1:] <= got[:, :-1] + 1e-12)


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_end_points(eng, cx, label):
    W, phi = model(12, cx, label, 37, 10)
    N, T = phi.shape[:2]
    got, _ = eng.prefix_model(W, phi)
    full, _ = eng.marginal_model(W, phi, None)
    none, _ = eng.marginal_model(W, phi[:1], np.ones((1, T), dtype=np.uint8))
    assert np.abs(got[:, T] - full).max() <= F64_TOL
    assert np.abs(got[0, 0] - none[0]).max() <= F64_TOL
    assert all(np.array_equal(got[i, 0], got[0, 0]) for i in range(N))


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_a_permutation_of_the_series_permutes_the_bits(eng, cx):
    W, phi = model(12, cx, "mid", 37, 10)
    perm = np.random.default_rng(3).permutation(phi.shape[0])
    a, _ = eng.prefix_model(W, phi)
    b, _ = eng.prefix_model(W, phi[perm])
    assert np.array_equal(a[perm], b)


def test_blocks_do_not_change_the_result(eng, monkeypatch):
    """N = 136, T = 64, chi = 24, label last, under a budget of 1 073 741 bytes: 64 * 3 + 1 = 193 tables of 24 * 24 * 8 bytes and the
    65 * 3 logs take 890 904 of them; a series needs 4 * 24 * 8 + 65 * 3 * 8 = 2328, so 78 fit and a block is 64 series (four tiles):
    blocks of 64, 64 and 8 (tests/test_prefix_host.py has the same sum).  The bits of one block."""
    W, phi = model(24, False, "last", 136, 64)
    one, _ = eng.prefix_model(W, phi)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    cut, _ = eng.prefix_model(W, phi)
    assert np.all(np.isfinite(one)) and np.array_equal(one, cut)


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("chi,N,T", SHAPES, ids=SHAPE_IDS)
def test_monotone_in_the_prefix_length(eng, chi, N, T, cx, label):
    """unit-norm states: a longer prefix cannot be more likely (Cauchy-Schwarz)"""
    W, phi = model(chi, cx, label, N, T)
    got, _ = eng.prefix_model(W, phi)
    assert np.all(got[:, 1:] <= got[:, :-1] + 1e-12)


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_a_vanishing_row_is_minus_infinity_from_there_on(eng, cx, label):
    W, phi = model(12, cx, label, 37, 10)
    zeroed = np.array(phi)
    zeroed[5, 3] = 0.0
    a, _ = eng.prefix_model(W, phi)
    b, _ = eng.prefix_model(W, zeroed)
    assert not np.any(np.isnan(b))
    assert np.all(np.isfinite(b[5, :4])) and np.all(np.isneginf(b[5, 4:]))
    assert np.array_equal(b[5, :4], a[5, :4])
    others = np.arange(phi.shape[0]) != 5
    assert np.array_equal(a[others], b[others])


@functools.lru_cache(maxsize=None)
def long_case():
    T = 1000
    rng = np.random.default_rng(77)
    W = MR.normalised_chain(T, 2, 8, 2, rng)
    phi = MR.random_states(2, T, 2, False, rng)
    lengths = list(range(0, T + 1, 50))
    return W, phi, lengths, PR.prefix_log_marginals_ref(W, phi, lengths)


def test_long_chain(eng):
    """T = 1000: ln l of the complete series is far below ln(5e-324) = -744.4, where an unscaled fp64 chain has underflowed; every
    50th prefix length is restated (all 1001 are too slow in NumPy)"""
    W, phi, lengths, ref = long_case()
    T = len(W)
    got, _ = eng.prefix_model(W, phi)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    err = np.abs(got[:, lengths] - ref).max()
    print(f"T=1000: ln l down to {got.min():.1f}, largest |d ln l| at every 50th prefix = {err:.3e}")
    assert got.min() < -745.0
    assert err <= F64_TOL * T / 10


def test_argument_errors(eng):
    W, phi = model(7, False, "last", 21, 10)
    lib, dp = eng.lib, C.POINTER(C.c_double)
    m, keep = marginal.model_struct(W, phi)
    out = np.zeros((phi.shape[0], phi.shape[1] + 1, CN))
    assert lib.mpst_prefix_marginals(eng.ctx, None, out.ctypes.data_as(dp), None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_prefix_marginals(eng.ctx, C.byref(m), None, None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_prefix_marginals(eng.ctx, C.byref(m), out.ctypes.data_as(dp), None) == 0          # seconds may be NULL
    want, _ = eng.prefix_model(W, phi)
    assert np.array_equal(out, want)
    m32, keep32 = marginal.model_struct(W, phi, "f32")
    assert lib.mpst_prefix_marginals(eng.ctx, C.byref(m32), out.ctypes.data_as(dp), None) == mt._lib.MPST_ERR_UNSUPPORTED
    del keep, keep32
    rng = np.random.default_rng(2)
    Wb = MR.gaussian_chain(3, 2, 2, 17, 2, False, rng)
    with pytest.raises(mt.MPSTError) as ei:
        eng.prefix_model(Wb, MR.random_states(2, 3, 2, False, rng))
    assert ei.value.code == mt._lib.MPST_ERR_UNSUPPORTED


def test_phases_are_the_two_kernels(eng):
    W, phi = model(12, False, "mid", 37, 10)
    _, secs = eng.prefix_model(W, phi)
    env, walk = eng.impute_phases()
    assert env > 0.0 and walk > 0.0 and env + walk <= secs * (1.0 + 1e-6) + 1e-6


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_end_to_end(eng):
    from tests.test_gpu_split import _fit_data
    Xtr, ytr, Xte, yte = _fit_data()
    trained, _, _ = mt.fitMPS(Xtr, ytr, Xte, yte, mt.MPSOptions(chi_max=8, nsweeps=2, verbosity=-1, d=4))
    N, T = Xte.shape
    lp = mt.prefix_log_marginals(trained, Xte, engine=eng)
    assert lp.shape == (N, T + 1, len(np.unique(ytr))) and np.all(np.isfinite(lp))
    post = mt.prefix_posteriors(trained, Xte, engine=eng)
    for t in (1, T // 2, T):
        want = mt.class_posteriors(trained, Xte, PR.suffix_mask(N, T, t), engine=eng)
        assert np.abs(post[:, t] - want).max() <= 1e-9
    never = mt.classify_early(trained, Xte, threshold=2.0, engine=eng)
    assert np.all(never.lengths == T) and np.array_equal(never.labels, mt.classify(trained, Xte))
    at_once = mt.classify_early(trained, Xte, threshold=0.0, min_length=3, engine=eng)
    assert np.all(at_once.lengths == 3)
    labels = np.unique(ytr)
    idx = np.searchsorted(labels, yte)
    scores = mt.causal_scores(trained, Xte, labels=yte, engine=eng)
    rows = np.arange(N)
    assert scores.shape == (N, T)
    assert np.abs(scores.sum(axis=1) - (lp[rows, 0, idx] - lp[rows, T, idx])).max() <= 1e-9
    lpn = mt.prefix_log_marginals(trained, Xte, normalise_classes=True, engine=eng)
    assert np.array_equal(lpn, lp - lp[:, :1])
    curve = mt.early_accuracy_curve(trained, Xte, yte, engine=eng)
    assert curve.shape == (T + 1,) and curve[T] == np.mean(mt.classify(trained, Xte) == yte)
    assert np.array_equal(prefix.early_decisions(lp, 2.0)[0], np.argmax(lp[:, T], axis=1))
