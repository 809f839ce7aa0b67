"""mpst_marginal_model on the device against the NumPy restatement (tests/marginal_ref.py), against the complete-data overlaps,
against ||W_c||^2, and end to end through log_marginals / class_posteriors / classify(..., missing_mask=)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import marginal
from oracle import impute_numpy as IN
from oracle import ref_numpy as R
from tests import marginal_ref as MR
from tests.helpers import load_engine

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10         # every site contributes about d chi eps ~ 1e-14 to ln l and T <= 1000: two decades of margin
# fp32 compute path: the largest |ln l (device) - ln l (fp64 restatement)| over the 16 cases of test_against_the_restatement_fp32
# measured on an MI355X (3.772e-05, at chi72_big-real-last; most cases sit near 1e-06, the outliers are the rows whose amplitude is
# small against its terms, the same rows that reach 6e-13 in fp64), and the bound: four times that, because the order of the
# reductions differs between machines
F32_MEASURED = 3.772e-5
F32_BOUND = 4.0 * F32_MEASURED


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


def special_masks(N, T, ls, rng):
    """ragged at 40 %; row 0 all missing, row 1 none, row 2 one site and - N > 3 - row 3 exactly the label site (N = 3: the one
    missing site of row 2 IS the label site)"""
    m = rng.random((N, T)) < 0.4
    m[0] = True
    m[1] = False
    m[2] = False
    if N > 3:
        m[2, (ls + 3) % T] = True
        m[3] = False
        m[3, ls] = True
    else:
        m[2, ls] = True
    return m


@functools.lru_cache(maxsize=None)
def case(chi, cx, label, N=21, T=10, ragged_only=False):
    """(W, phi, mask, fp64 restatement) - built once, shared by the tests below, never modified"""
    d, Cn = 6, 3
    rng = np.random.default_rng(1000 + 7 * chi + (1 if cx else 0) + (2 if label == "mid" else 0) + N)
    if label == "last":
        W = R.random_mps(T, d, chi, Cn, rng, dtype=np.complex128 if cx else np.float64)
        ls = T - 1
    else:
        ls = T // 2
        W = MR.gaussian_chain(T, d, chi, Cn, ls, cx, rng, scale=1.0 / np.sqrt(d * chi))
    phi = MR.random_states(N, T, d, cx, rng)
    mask = rng.random((N, T)) < 0.4 if ragged_only else special_masks(N, T, ls, rng)
    ref = MR.log_marginals_ref(W, phi, mask)
    for a in W + [phi, mask, ref]:
        a.setflags(write=False)
    return W, phi, mask, ref


# chi = 12: not a multiple of 16; chi = 7: below one tile; chi = 72 (T = 6): beyond the LDS limit, from global scratch - N = 3 as the
# special rows alone and N = 6 ragged, so that known and missing sites meet a matrix there too
SHAPES = [(12, 21, 10, False), (7, 21, 10, False), (72, 3, 6, False), (72, 6, 6, True)]
SHAPE_IDS = ["chi12", "chi7", "chi72_big", "chi72_big_ragged"]


@pytest.mark.parametrize("label", ["last", "mid"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("chi,N,T,ragged", SHAPES, ids=SHAPE_IDS)
def test_against_the_restatement_fp64(eng, chi, N, T, ragged, cx, label):
    W, phi, mask, ref = case(chi, cx, label, N, T, ragged)
    got, _ = eng.marginal_model(W, phi, mask)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    err = np.abs(got - ref).max()
    print(f"fp64 chi={chi} cx={cx} label={label}: largest |d ln l| = {err:.3e}")
    assert err <= F64_TOL


@pytest.mark.parametrize("label", ["last", "mid"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("chi,N,T,ragged", SHAPES, ids=SHAPE_IDS)
def test_against_the_restatement_fp32(eng, chi, N, T, ragged, cx, label):
    """fp32 chain contractions, fp64 log accumulator, against the fp64 restatement.  Measured on an MI355X over all 16 cases of this
    test: largest |d ln l| = 3.772e-05 (F32_MEASURED); the bound is 4 x that, 1.509e-04."""
    W, phi, mask, ref = case(chi, cx, label, N, T, ragged)
    got, _ = eng.marginal_model(W, phi, mask, compute="f32")
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref).max()
    print(f"fp32 chi={chi} cx={cx} label={label}: largest |d ln l| = {err:.3e}")
    assert err <= F32_BOUND


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_complete_data_is_the_classifier_overlap(eng, cx):
    W, phi, _, _ = case(12, cx, "last")
    yhat = R.contract_mps(W, phi)
    a, _ = eng.marginal_model(W, phi, None)
    b, _ = eng.marginal_model(W, phi, np.zeros(phi.shape[:2], dtype=np.uint8))
    assert np.array_equal(a, b)                                  # NULL and the all-zero mask: the same bits
    assert np.abs(a - np.log(np.abs(yhat) ** 2)).max() <= 1e-10
    if not cx:
        N = phi.shape[0]
        ds = R.EncodedSet(phi, np.zeros(N, dtype=np.int32), np.array([N, 0, 0]))
        e2 = mt.SweepEngine(0)
        try:
            load_engine(e2, ds, W, R.SweepOptions(nsweeps=1, chi_max=12, eta=0.02), test=ds)
            _, yh = e2.classify(1, return_overlaps=True)
        finally:
            e2.close()
        assert np.abs(a - np.log(np.abs(yh) ** 2)).max() <= 1e-10


@pytest.mark.parametrize("label", ["last", "mid"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_nothing_known_is_the_norm_of_the_class_slice(eng, cx, label):
    W, phi, _, _ = case(12, cx, label)
    Cn = 3
    want = np.array([2.0 * np.log(IN.mps_norm3(MR.class_slice(W, c))) for c in range(Cn)])
    junk = np.array(phi)
    junk[::2] = np.nan
    junk[1::2] *= 1e30
    got, _ = eng.marginal_model(W, junk, np.ones(phi.shape[:2], dtype=np.uint8))
    assert np.abs(got[0] - want).max() <= 1e-10
    assert all(np.array_equal(got[i], got[0]) for i in range(len(got)))          # whatever phi holds


@pytest.mark.parametrize("compute", ["f64", "f32"])
@pytest.mark.parametrize("chi,N,T,ragged", SHAPES[::2], ids=SHAPE_IDS[::2])
def test_masked_values_are_not_read(eng, chi, N, T, ragged, compute):
    W, phi, mask, _ = case(chi, True, "mid", N, T, ragged)
    a, _ = eng.marginal_model(W, phi, mask, compute=compute)
    poisoned = np.array(phi)
    poisoned[mask] = np.nan
    b, _ = eng.marginal_model(W, poisoned, mask, compute=compute)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def long_case(T):
    rng = np.random.default_rng(31 + T)
    W = MR.normalised_chain(T, 4, 8, 2, rng)
    phi = R.legendre_encode(rng.uniform(-1, 1, (4, T)), 4)
    return W, phi, MR.log_marginals_ref(W, phi, None)


def test_long_chain_fp64(eng):
    """T = 1000: ln l is below -800, where an unscaled fp64 chain has underflowed"""
    W, phi, ref = long_case(1000)
    assert np.all(np.isfinite(ref)) and ref.max() < -800.0
    got, _ = eng.marginal_model(W, phi, None)
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref).max()
    print(f"T=1000 fp64: ln l in [{ref.min():.1f}, {ref.max():.1f}], largest |d ln l| = {err:.3e}")
    assert err <= F64_TOL


def test_long_chain_fp32(eng):
    """T = 200: ln l is below -103, past the fp32 denormals; the bound of the T = 10 cases scaled by T / 10 (3.018e-03; measured
    on an MI355X: 6.986e-05 at ln l in [-190.1, -173.1])"""
    W, phi, ref = long_case(200)
    assert np.all(np.isfinite(ref)) and ref.max() < -103.0
    got, _ = eng.marginal_model(W, phi, None, compute="f32")
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref).max()
    print(f"T=200 fp32: ln l in [{ref.min():.1f}, {ref.max():.1f}], largest |d ln l| = {err:.3e}")
    assert err <= F32_BOUND * 200 / 10


@pytest.mark.parametrize("label", ["last", "mid"])
def test_zero_likelihood_is_minus_infinity(eng, label):
    W, phi, mask, ref = case(12, False, label)
    ls = MR.label_site_of(W)
    Wz = [np.array(t) for t in W]
    Wz[ls][..., 1] = 0.0
    got, _ = eng.marginal_model(Wz, phi, mask)
    assert not np.any(np.isnan(got))
    assert np.all(np.isneginf(got[:, 1]))
    assert np.all(np.isfinite(got[:, [0, 2]])) and np.abs(got[:, [0, 2]] - ref[:, [0, 2]]).max() <= F64_TOL


def test_abi_errors(eng):
    W, phi, mask, _ = case(7, False, "last")
    lib, dp = eng.lib, C.POINTER(C.c_double)
    model, keep = marginal.model_struct(W, phi)
    logp = np.zeros((phi.shape[0], 3))
    assert lib.mpst_marginal_model(eng.ctx, None, None, logp.ctypes.data_as(dp), None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_marginal_model(eng.ctx, C.byref(model), None, None, None) == mt._lib.MPST_ERR_INVALID
    assert lib.mpst_marginal_model(eng.ctx, C.byref(model), None, logp.ctypes.data_as(dp), None) == 0      # seconds may be NULL
    del keep
    rng = np.random.default_rng(2)
    for d, Cn in ((2, 17), (17, 2)):
        Wb = MR.gaussian_chain(3, d, 2, Cn, 2, False, rng)
        with pytest.raises(mt.MPSTError) as ei:
            eng.marginal_model(Wb, MR.random_states(2, 3, d, False, rng), None)
        assert ei.value.code == mt._lib.MPST_ERR_UNSUPPORTED


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _parent_classify(trained, X):
    """mt.classify as it was before the missing_mask keyword"""
    from mpstime_jl_amd.options import engine_options, safe_options
    from mpstime_jl_amd.training import classify_states
    labels = np.unique(trained.train_data.labels)
    states = classify_states(trained, X)
    e = mt.SweepEngine(0)
    try:
        Cn = int(trained.mps[-1].shape[3])
        e.set_options(**engine_options(safe_options(trained.opts)))
        e.set_dataset(0, trained.train_data.phi[:1], trained.train_data.label_index[:1], Cn)
        e.set_dataset(1, states.phi, np.zeros(len(states), dtype=np.int32), Cn)
        e.set_mps(trained.mps)
        return labels[e.classify(1)]
    finally:
        e.close()


@pytest.mark.parametrize("opts", [dict(d=4), dict(encoding="hist_split_legendre", d=6, aux_basis_dim=2)], ids=["legendre", "hist_split_td"])
def test_end_to_end(eng, opts, monkeypatch):
    from tests.test_gpu_split import _fit_data
    Xtr, ytr, Xte, yte = _fit_data()
    trained, _, _ = mt.fitMPS(Xtr, ytr, Xte, yte, mt.MPSOptions(chi_max=8, nsweeps=2, verbosity=-1, **opts))
    rng = np.random.default_rng(5)
    Xc = np.stack([mt.mar(x, 0.3, rng)[0] for x in Xte])
    mask = np.isnan(Xc)
    assert mask.any(axis=1).all()
    labels = np.unique(ytr)
    pred = mt.classify(trained, Xc, engine=eng, missing_mask=mask)
    phi, _ = marginal.marginal_states(trained, Xc, mask)
    ref = MR.log_marginals_ref(trained.mps, phi, mask)
    top = np.sort(ref, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-8
    assert (~clear).sum() <= 1
    assert np.array_equal(pred[clear], labels[np.argmax(ref, axis=1)][clear])
    lp = mt.log_marginals(trained, Xc, mask, engine=eng)
    assert np.abs(lp - ref).max() <= F64_TOL
    post = mt.class_posteriors(trained, Xc, mask, engine=eng)
    assert np.abs(post.sum(axis=1) - 1.0).max() <= 1e-12 and np.array_equal(np.argmax(post, axis=1), np.argmax(lp, axis=1))
    lpn = mt.log_marginals(trained, Xc, mask, normalise_classes=True, engine=eng)
    allrow = mt.log_marginals(trained, Xte[:1], np.ones((1, Xte.shape[1]), dtype=bool), engine=eng)[0]
    assert np.array_equal(lpn, lp - allrow)
    # without the keyword: the code path of before, which never enters the new module
    monkeypatch.setattr(marginal, "log_marginals", lambda *a, **k: pytest.fail("classify without a mask entered marginal.py"))
    monkeypatch.setattr(marginal, "classify_incomplete", lambda *a, **k: pytest.fail("classify without a mask entered marginal.py"))
    assert np.array_equal(mt.classify(trained, Xte), _parent_classify(trained, Xte))
