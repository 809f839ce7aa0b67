"""mpst_segment_marginals on the device against the NumPy restatement (tests/segment_ref.py: log_marginals_ref over the complement
masks), against mpst_prefix_marginals and mpst_marginal_model where their questions coincide, and end to end through
segment_posteriors / most_discriminative_segment."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import marginal, segments
from tests import marginal_ref as MR
from tests import segment_ref as SR

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10         # the project's bound for ln l in fp64 (tests/test_gpu_marginal.py, tests/test_gpu_prefix.py)
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
    rng = np.random.default_rng(2700 + 11 * chi + (1 if cx else 0) + 3 * label_site(label, T) + N)
    W = MR.gaussian_chain(T, d, chi, Cn, label_site(label, T), cx, rng, scale=1.0 / np.sqrt(d * chi))
    phi = MR.random_states(N, T, d, cx, rng)
    for a in W + [phi]:
        a.setflags(write=False)
    return W, phi


# the eight segments restated where all 21 are too slow in NumPy: both ends, the 128-bond on either side, widths 1 .. T
LISTED = ((0, 1), (0, 3), (2, 2), (3, 1), (3, 3), (1, 4), (0, 6), (5, 1))


@functools.lru_cache(maxsize=None)
def restated(chi, cx, label, N, T, mw, listed):
    ref = SR.segment_log_marginals_ref(*model(chi, cx, label, N, T), mw, None if listed is None else list(listed))
    ref.setflags(write=False)
    return ref


def in_triangle(T, mw):
    return segments.valid_triangle(T, mw)


# (chi, N, T, max_width, the segments restated): chi = 12: every segment, chi not a multiple of 16; chi = 7: max_width < T; chi = 56:
# complex models leave the LDS route while real ones stay on it; chi = 72: the global-scratch route and a second column tile;
# chi = 128: the upper limit, bonds 1, 6, 36, 128, 36, 6, 1
SHAPES = [(12, 5, 10, 10, None), (7, 3, 10, 4, None), (56, 1, 6, 6, None), (72, 1, 6, 6, LISTED), (128, 1, 6, 6, LISTED)]
SHAPE_IDS = ["chi12", "chi7_narrow", "chi56", "chi72_big", "chi128"]


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("chi,N,T,mw,listed", SHAPES, ids=SHAPE_IDS)
def test_against_the_restatement(eng, chi, N, T, mw, listed, cx, label):
    W, phi = model(chi, cx, label, N, T)
    ref = restated(chi, cx, label, N, T, mw, listed)
    got, _, _ = eng.segment_model(W, phi, mw)
    assert got.shape == (N, T, mw, CN)
    tri = in_triangle(T, mw)
    # the corner beyond the end of the chain is NaN, exactly; nothing inside the triangle is
    assert np.all(np.isnan(got[:, ~tri])) and np.all(np.isfinite(got[:, tri]))
    at = ~np.isnan(ref)
    assert at.sum() == N * CN * (tri.sum() if listed is None else len(listed)) and np.all(np.isfinite(ref[at]))
    err = np.abs(got[at] - ref[at]).max()
    print(f"chi={chi} cx={cx} label={label}: largest |d ln l| = {err:.3e}")
    assert err <= F64_TOL
    if chi == 128:
        assert max(t.shape[2] for t in W) == 128
        wider, narrower = got[:, :, 1:], got[:, :, :-1]
        ok = tri[None, :, 1:, None] & np.ones_like(wider, dtype=bool)
        assert np.all(wider[ok] <= narrower[ok] + 1e-12)


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_against_the_other_queries(eng, cx, label):
    """start 0 is the prefix question, the widest segment the complete series, lnorm the empty prefix; and every entry is what the
    device's own mpst_marginal_model gives for the complement-masked replica"""
    W, phi = model(12, cx, label, 5, 10)
    N, T = phi.shape[:2]
    got, lnorm, _ = eng.segment_model(W, phi, T)
    pre, _ = eng.prefix_model(W, phi)
    full, _ = eng.marginal_model(W, phi, None)
    for t in range(1, T + 1):
        assert np.abs(got[:, 0, t - 1] - pre[:, t]).max() <= F64_TOL
    assert np.abs(lnorm - pre[0, 0]).max() <= F64_TOL
    assert np.abs(got[:, 0, T - 1] - full).max() <= F64_TOL
    segs = SR.all_segments(T, T)
    reps = np.concatenate([phi] * len(segs))
    mask = np.concatenate([SR.complement_mask(N, T, a, w) for a, w in segs])
    dev, _ = eng.marginal_model(W, reps, mask)
    worst = max(np.abs(got[:, a, w - 1] - dev[k * N:(k + 1) * N]).max() for k, (a, w) in enumerate(segs))
    print(f"cx={cx} label={label}: largest |d ln l| against marginal_model on {len(segs) * N} replicas = {worst:.3e}")
    assert worst <= F64_TOL


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_monotone_in_the_width(eng, cx, label):
    """unit-norm states: a wider segment from the same start cannot be more likely (Cauchy-Schwarz)"""
    W, phi = model(12, cx, label, 5, 10)
    got, _, _ = eng.segment_model(W, phi, 10)
    ok = in_triangle(10, 10)[None, :, 1:, None] & np.ones_like(got[:, :, 1:], dtype=bool)
    assert np.all(got[:, :, 1:][ok] <= got[:, :, :-1][ok] + 1e-12)


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_a_permutation_of_the_series_permutes_the_bits(eng, cx):
    W, phi = model(12, cx, "mid", 5, 10)
    perm = np.random.default_rng(3).permutation(phi.shape[0])
    a, _, _ = eng.segment_model(W, phi, 10)
    b, _, _ = eng.segment_model(W, phi[perm], 10)
    assert np.array_equal(a[perm], b, equal_nan=True)


def test_blocks_do_not_change_the_result(eng, monkeypatch):
    """N = 136, T = 24, chi = 24, label last, max_width = 8, under a budget of 1 073 741 bytes: 25 * 4 = 100 tables of 24 * 24 * 8
    bytes and the 2 * 25 * 3 logs take 462 000 of them; a series brings 24 * 8 * 3 * 8 = 4608 bytes of results, so 132 fit and a
    block is 128 series (eight tiles): blocks of 128 and 8 (tests/test_segment_host.py has the same sum).  The bits of one block."""
    W, phi = model(24, False, "last", 136, 24)
    one, _, _ = eng.segment_model(W, phi, 8)
    assert eng.impute_info()["env_workgroups"] == 1 and eng.impute_info()["chains"] == 136 * 24
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
    cut, _, _ = eng.segment_model(W, phi, 8)
    assert eng.impute_info()["env_workgroups"] == 2
    tri = in_triangle(24, 8)
    assert np.all(np.isfinite(one[:, tri])) and np.array_equal(one, cut, equal_nan=True)


@pytest.mark.parametrize("label", ["last", "mid", "first"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_a_vanishing_state_is_minus_infinity_where_it_is_read(eng, cx, label):
    """the state of series 2 at site 3 is zero: -inf exactly in the segments that contain site 3, the bits of everything else kept"""
    W, phi = model(12, cx, label, 5, 10)
    zeroed = np.array(phi)
    zeroed[2, 3] = 0.0
    a, _, _ = eng.segment_model(W, phi, 10)
    b, _, _ = eng.segment_model(W, zeroed, 10)
    tri = in_triangle(10, 10)
    holds = tri & (np.arange(10)[:, None] <= 3) & (np.arange(10)[:, None] + np.arange(1, 11)[None, :] > 3)
    assert not np.any(np.isnan(b[:, tri]))
    assert np.all(np.isneginf(b[2][holds])) and np.all(np.isfinite(b[2][tri & ~holds]))
    assert np.array_equal(b[2][~holds], a[2][~holds], equal_nan=True)
    others = np.arange(phi.shape[0]) != 2
    assert np.array_equal(a[others], b[others], equal_nan=True)


@functools.lru_cache(maxsize=None)
def long_case():
    T, mw = 1000, 8
    rng = np.random.default_rng(78)
    W = MR.normalised_chain(T, 2, 8, 2, rng)
    phi = MR.random_states(2, T, 2, False, rng)
    segs = [(a, w) for a in range(0, T, 100) for w in range(1, mw + 1)]
    return W, phi, mw, segs, SR.segment_log_marginals_ref(W, phi, mw, segs)


def test_long_chain(eng):
    """T = 1000, two series, max_width = 8: the tables pass through all thousand sites; every 100th start is restated at every width.
    The bound is the prefix marginals' for their long chain, 1e-10 * T / 10 = 1e-8."""
    W, phi, mw, segs, ref = long_case()
    T = len(W)
    got, _, _ = eng.segment_model(W, phi, mw)
    tri = in_triangle(T, mw)
    assert np.all(np.isfinite(got[:, tri])) and np.all(np.isnan(got[:, ~tri]))
    at = ~np.isnan(ref)
    assert at.sum() == 2 * 2 * len(segs)
    err = np.abs(got[at] - ref[at]).max()
    print(f"T=1000: largest |d ln l| at every 100th start = {err:.3e}")
    assert err <= F64_TOL * T / 10


def test_argument_errors(eng):
    W, phi = model(7, False, "last", 3, 10)
    lib, dp = eng.lib, C.POINTER(C.c_double)
    N, T = phi.shape[:2]
    m, keep = marginal.model_struct(W, phi)
    out, ln = np.zeros((N, T, 4, CN)), np.zeros(CN)
    want, lnorm, _ = eng.segment_model(W, phi, 4)
    before = eng.impute_info()
    assert lib.mpst_segment_marginals(eng.ctx, C.byref(m), 0, out.ctypes.data_as(dp), None, None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_segment_marginals(eng.ctx, C.byref(m), T + 1, out.ctypes.data_as(dp), None, None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_segment_marginals(eng.ctx, C.byref(m), 4, None, None, None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_segment_marginals(eng.ctx, None, 4, out.ctypes.data_as(dp), None, None) == mt._lib.MPST_ERR_INVALID
    m32, keep32 = marginal.model_struct(W, phi, "f32")
    assert lib.mpst_segment_marginals(eng.ctx, C.byref(m32), 4, out.ctypes.data_as(dp), None, None) == mt._lib.MPST_ERR_UNSUPPORTED
    assert eng.impute_info() == before                                  # a rejected call leaves the context as it was
    # ... and the call after them succeeds; lnorm_out and seconds may be NULL
    assert lib.mpst_segment_marginals(eng.ctx, C.byref(m), 4, out.ctypes.data_as(dp), None, None) == 0
    assert np.array_equal(out, want, equal_nan=True)
    assert lib.mpst_segment_marginals(eng.ctx, C.byref(m), 4, out.ctypes.data_as(dp), ln.ctypes.data_as(dp), None) == 0
    assert np.array_equal(ln, lnorm)
    del keep, keep32
    rng = np.random.default_rng(2)
    Wb = MR.gaussian_chain(3, 2, 2, 17, 2, False, rng)
    with pytest.raises(mt.MPSTError) as ei:
        eng.segment_model(Wb, MR.random_states(2, 3, 2, False, rng), 2)
    assert ei.value.code == mt._lib.MPST_ERR_UNSUPPORTED


def test_phases_are_the_tables_and_the_walk(eng):
    W, phi = model(12, False, "mid", 5, 10)
    _, _, secs = eng.segment_model(W, phi, 10)
    tables, walk = eng.impute_phases()
    assert tables > 0.0 and walk > 0.0 and tables + walk <= secs * (1.0 + 1e-6) + 1e-6


# ---- end to end -------------------------------------------------------------------------------------------------------------------
STRETCH = (8, 16)       # the sites on which the two classes of segment_fit_data differ
E2E_WIDTH = 6


def segment_fit_data(ntr=200, nte=40, T=24, seed=5):
    """The two ``trendy_sine`` classes of shim_check.py (periods in (12, 15) and in (16, 19), slopes -3 / 0 / 3, noise 0.1) at phase
    zero, made to differ only on the sites STRETCH: a series of class 1 follows the slower sine there and the curve of its own
    class-0 parameters everywhere else."""
    rng = np.random.default_rng(seed)
    t0, t1 = STRETCH

    def draw(n):
        X, y = np.empty((n, T)), np.arange(n) % 2
        for i in range(n):
            p0, p1, m = rng.uniform(12.0, 15.0), rng.uniform(16.0, 19.0), rng.choice([-3.0, 0.0, 3.0])
            X[i] = mt.trendy_sine(T, 1, period=p0, slope=m, phase=0.0)[0][0]
            if y[i] == 1:
                X[i, t0:t1] = mt.trendy_sine(T, 1, period=p1, slope=m, phase=0.0)[0][0, t0:t1]
        return X + 0.1 * rng.standard_normal((n, T)), y
    Xtr, ytr = draw(ntr)
    Xte, yte = draw(nte)
    return Xtr, ytr, Xte, yte


def overlap_share(best):
    """the share of series whose segment has a site inside STRETCH"""
    return float(np.mean((best.start < STRETCH[1]) & (best.start + best.width > STRETCH[0])))


@functools.lru_cache(maxsize=None)
def segment_fit():
    Xtr, ytr, Xte, yte = segment_fit_data()
    trained, _, _ = mt.fitMPS(Xtr, ytr, Xte, yte, mt.MPSOptions(chi_max=12, nsweeps=5, verbosity=-1, d=4))
    return trained, Xte, yte


def test_end_to_end(eng):
    """The classes differ on the sites STRETCH only, so that is where the evidence has to be found: the best segment of at most
    E2E_WIDTH sites of most test series overlaps it.  By chance 49 % would (63 of the 129 segments do).

    Measured on this model (chi_max = 12, d = 4, 5 sweeps, 200 training and 40 test series, test accuracy 0.80): the NumPy restatement
    (segment_ref over all 129 segments, 19 s, so not repeated here) puts the best segment of 36 of the 40 series on the stretch, a
    share of 0.900, and the device the same 36; ln l differs by at most 1.2e-13 between the two.  The margin is one series, 0.025:
    rounding of ln l cannot move a best segment - the closest call between a segment on the stretch and one off it is a posterior
    gap of 5.0e-3, against 1e-10 - so the margin only covers a fit whose last bits differ and move that closest series."""
    trained, Xte, yte = segment_fit()
    N, T = Xte.shape
    labels = np.unique(trained.train_data.labels)
    idx = np.searchsorted(labels, yte)
    post = mt.segment_posteriors(trained, Xte, E2E_WIDTH, engine=eng)
    tri = in_triangle(T, E2E_WIDTH)
    assert post.shape == (N, T, E2E_WIDTH, len(labels))
    assert np.all(np.isnan(post[:, ~tri])) and np.abs(post[:, tri].sum(axis=-1) - 1.0).max() <= 1e-12
    best = mt.most_discriminative_segment(trained, Xte, y=yte, max_width=E2E_WIDTH, engine=eng)
    assert np.all(best.start + best.width <= T) and np.all(best.width >= 1) and np.all(best.width <= E2E_WIDTH)
    rows = np.arange(N)
    mine = post[rows, best.start, best.width - 1, idx]
    assert np.array_equal(best.posterior, mine)
    assert np.all(best.posterior >= np.nanmax(post[rows, :, :, idx], axis=(1, 2)))
    share = overlap_share(best)
    print(f"best segments on the stretch: {share:.3f}; median posterior there {np.median(best.posterior):.3f}")
    assert share > 0.5 and share >= 0.900 - 1.0 / N
    # the widest segment from the first site, at max_width = T, is the complete series
    full = mt.segment_log_marginals(trained, Xte, T, engine=eng)[:, 0, T - 1]
    assert np.array_equal(labels[np.argmax(full, axis=1)], mt.classify(trained, Xte))
    assert np.array_equal(mt.classify_segment(trained, Xte, 0, T, engine=eng), mt.classify(trained, Xte))
    # the evidence map at width 4 and the accuracy map agree with the NumPy functions on the same array
    lpn = mt.segment_log_marginals(trained, Xte, E2E_WIDTH, normalise_classes=True, engine=eng)
    ev = mt.segment_evidence(trained, Xte, y=yte, width=4, engine=eng)
    assert ev.shape == (N, T) and np.array_equal(ev, segments.evidence_from(lpn[:, :, :4], idx, 4), equal_nan=True)
    amap = mt.segment_accuracy_map(trained, Xte, yte, E2E_WIDTH, engine=eng)
    assert amap.shape == (T, E2E_WIDTH) and np.all(np.isnan(amap[~tri]))
    on, off = amap[8:11, E2E_WIDTH - 1].mean(), amap[:2, E2E_WIDTH - 1].mean()
    print(f"accuracy from {E2E_WIDTH} sites on the stretch {on:.3f}, ahead of it {off:.3f}")
    assert on > off
