"""Model overlaps on the device (mpst_model_overlaps, csrc/mpst_overlap.hip: k_overlap) through the Python layer and the C ABI, against the
NumPy restatement in tests/overlap_ref.py.  Every normalised overlap and every ln norm within 1e-10 absolute, the project's fp64 query
tolerance (F64_TOL of tests/test_gpu_marginal.py); tests/test_overlap_ref.py holds the restatement itself to 1e-11 against long double on
the same shapes.  Each case prints its largest deviation; measured on an MI355X: at most 1.8e-14 over the real cases and the complex
cases at T = 10 and 6, 1.3e-12 (normalised overlap) and 3.4e-13 (ln norm) at complex T = 1000, where the restatement itself is 1.2e-12
from long double (DESIGN.md §21 has the table)."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import overlaps as OV
from tests import overlap_ref as R
from tests.marginal_ref import gaussian_chain

pytestmark = pytest.mark.gpu

TOL = 1e-10
L = mt._lib
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case(name, cx):
    """(models [a, b, c], log norms, normalised blocks of all six pairs) - computed once, shared, never written to"""
    models = R.case_models(name, cx)
    log_norm, blocks = R.normalised_ref(models)
    return models, log_norm, blocks


def block(ov, a, b):
    o = ov.offsets
    return ov.overlap[o[a]:o[a + 1], o[b]:o[b + 1]]


def deviation(ov, log_norm, blocks):
    worst_n = max(float(np.abs(x - y).max()) for x, y in zip(ov.log_norm, log_norm))
    worst_o = max(float(np.abs(block(ov, a, b) - ref).max()) for (a, b), ref in blocks.items())
    return worst_o, worst_n


# ---- the five shapes of the issue, real and complex, all six pairs ---------------------------------------------------------------
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_against_the_restatement(eng, name, cx):
    models, log_norm, blocks = case(name, cx)
    k = R.CASES[name]
    # signal conditions, on the reference values: a kernel that returns zeros cannot pass
    assert np.all(np.abs(np.diagonal(blocks[(0, 1)])) >= 0.5)
    if k["chi"] <= 20 and k["T"] == 10:
        aa = np.abs(blocks[(0, 0)])
        assert (aa - np.diag(np.diag(aa))).max() >= 0.05
    ov = mt.model_overlaps(models, engine=eng)
    assert ov.overlap.dtype == (np.complex128 if cx else np.float64) and list(ov.offsets) == [0, k["C"], 2 * k["C"], 3 * k["C"]]
    assert np.all(np.isfinite(ov.overlap)) and np.all(np.isfinite(ov.lg))
    worst_o, worst_n = deviation(ov, log_norm, blocks)
    print(f"{name}-{'complex' if cx else 'real'}: largest deviation of a normalised overlap {worst_o:.2e}, of a ln norm {worst_n:.2e}")
    assert worst_o <= TOL and worst_n <= TOL
    assert np.array_equal(ov.fidelity, np.abs(ov.overlap)) and np.array_equal(ov.overlap, ov.overlap.conj().T)
    if k["T"] == 1000:
        assert np.abs(block(ov, 0, 2)).max() <= 1e-10 and np.isfinite(ov.lg[list(map(tuple, ov.pairs)).index((0, 2))])


# ---- the dense states: different C, so the Cmax padding -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def brute_models():
    rng = np.random.default_rng(77)
    return [gaussian_chain(5, 4, 6, 3, 2, True, rng, scale=0.3), gaussian_chain(5, 4, 9, 2, 2, True, rng, scale=0.3)]


def test_against_the_dense_states(eng):
    A, B = brute_models()
    ov = mt.model_overlaps([A, B], engine=eng)
    assert ov.g.shape == (3, 3, 3)
    worst = 0.0
    for q, (a, b) in enumerate(ov.pairs):
        ref = R.overlap_brute([A, B][a], [A, B][b])
        got = ov.g[q] * np.exp(ov.lg[q])
        ca, cb = ref.shape
        assert np.all(got[ca:] == 0) and np.all(got[:, cb:] == 0)                # entries beyond C_a x C_b are zero
        worst = max(worst, float(np.abs(got[:ca, :cb] - ref).max() / np.abs(ref).max()))
    print(f"dense states: largest relative deviation {worst:.2e}")
    assert worst <= 1e-12


# ---- 2 ln ||psi_c|| = the marginal likelihood with everything missing ---------------------------------------------------------------
@pytest.mark.parametrize("label", [9, 5], ids=["last", "mid"])
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_norms_against_the_marginals(eng, cx, label):
    rng = np.random.default_rng(31 + label + cx)
    W = gaussian_chain(10, 5, 12, 3, label, cx, rng, scale=0.2)
    phi = np.ones((1, 10, 5), dtype=np.complex128 if cx else np.float64)
    lp, _ = eng.marginal_model(W, phi, np.ones((1, 10), dtype=np.uint8))
    ov = mt.model_overlaps([W], engine=eng)
    err = float(np.abs(2 * ov.log_norm[0] - lp[0]).max())
    print(f"norms against marginals ({'complex' if cx else 'real'}, label {label}): {err:.2e}")
    assert err <= 1e-10


# ---- structure: self blocks, pair order, independence of the company and of the blocks ------------------------------------------------
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_self_blocks_and_pair_order(eng, cx):
    models, _, _ = case("chi7_mid", cx)
    table = np.array([[0, 0], [1, 1], [2, 2], [0, 1], [1, 0], [2, 1], [1, 2]], dtype=np.int32)
    g, lg, _ = OV.overlaps_raw(eng, models, table, cx)
    G = g * np.exp(lg)[:, None, None]
    for k in range(3):
        n = np.sqrt(np.abs(np.diagonal(G[k]).real))
        S = G[k] / n[:, None] / n[None, :]
        assert np.abs(S - S.conj().T).max() <= 1e-12 and np.abs(np.diagonal(S) - 1.0).max() <= 1e-12
    for q, r in ((3, 4), (6, 5)):
        scale = np.abs(G[q]).max()
        assert np.abs(G[r] - G[q].conj().T).max() <= 1e-12 * scale


def _raw_by_pair(eng, models, table, cx):
    g, lg, _ = OV.overlaps_raw(eng, models, None if table is None else np.array(table, dtype=np.int32), cx)
    K = len(models)
    pairs = [(a, b) for a in range(K) for b in range(a, K)] if table is None else [tuple(q) for q in table]
    return {q: (g[i].copy(), lg[i]) for i, q in enumerate(pairs)}


@pytest.mark.parametrize("name,cx", [("chi7_mid", False), ("chi40_scratch", False), ("chi40_scratch", True)], ids=["lds", "scratch-real", "scratch-complex"])
def test_a_pair_does_not_depend_on_its_company_or_its_block(eng, name, cx, monkeypatch):
    models, _, _ = case(name, cx)
    everything = _raw_by_pair(eng, models, None, cx)
    alone = _raw_by_pair(eng, models, [(0, 1)], cx)
    shuffled = _raw_by_pair(eng, models, [(2, 2), (1, 2), (0, 1), (0, 0)], cx)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.000001")       # the floor of the budget: one pair (complex) or two (real) per block at chi 72
    tiny = _raw_by_pair(eng, models, None, cx)
    monkeypatch.delenv("MPST_IMPUTE_CHUNK_GB")
    for other in (alone, shuffled, tiny):
        for q, (g, lg) in other.items():
            assert np.array_equal(g, everything[q][0]) and lg == everything[q][1], q


# ---- rescaling ----------------------------------------------------------------------------------------------------------------------
def test_a_norm_of_1e_minus_3000(eng):
    models, _, _ = case("long_mid", False)
    small = [[1e-3 * t for t in models[0]]] + list(models[1:])
    ov, ovs = mt.model_overlaps(models, engine=eng), mt.model_overlaps(small, engine=eng)
    shift = ovs.log_norm[0] - ov.log_norm[0]
    assert np.abs(shift - 1000 * np.log(1e-3)).max() <= 1e-9
    assert np.abs(ovs.overlap - ov.overlap).max() <= 1e-10 and np.all(np.isfinite(ovs.overlap))
    assert np.array_equal(ovs.log_norm[1], ov.log_norm[1])


# ---- edge shapes ----------------------------------------------------------------------------------------------------------------------
EDGES = {
    "K = 1, C = 1": dict(T=4, d=3, chi=5, C=1, label=3),
    "T = 2": dict(T=2, d=4, chi=4, C=2, label=1),
    "T = 1": dict(T=1, d=3, chi=1, C=2, label=0),
    "chi = 1 product states": dict(T=6, d=3, chi=1, C=2, label=2),
}


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", list(EDGES))
def test_edge_shapes(eng, name, cx):
    k = EDGES[name]
    rng = np.random.default_rng(5)
    models = [gaussian_chain(k["T"], k["d"], k["chi"], k["C"], k["label"], cx, rng, scale=0.5) for _ in range(1 if name.startswith("K = 1") else 2)]
    log_norm, blocks = R.normalised_ref(models)
    ov = mt.model_overlaps(models, engine=eng)
    worst_o, worst_n = deviation(ov, log_norm, blocks)
    print(f"{name}: {worst_o:.2e} {worst_n:.2e}")
    assert worst_o <= TOL and worst_n <= TOL
    if k["C"] == 1 and len(models) == 1:
        assert ov.overlap.shape == (1, 1) and abs(ov.overlap[0, 0] - 1.0) <= 1e-12
        assert np.array_equal(mt.class_overlaps(models[0], engine=eng), ov.fidelity)


def test_a_zero_class_slice(eng):
    models, log_norm, blocks = case("chi7_mid", False)
    p = R.CASES["chi7_mid"]["label"]
    dead = [t.copy() for t in models[0]]
    dead[p][..., 1] = 0.0
    ov = mt.model_overlaps([dead, models[1], models[2]], engine=eng)
    assert ov.log_norm[0][1] == -np.inf and np.all(np.isnan(ov.overlap[1, :])) and np.all(np.isnan(ov.overlap[:, 1]))
    keep = np.array([i for i in range(9) if i != 1])
    full = mt.model_overlaps(models, engine=eng)
    # nothing else disturbed (the power of two g is scaled by may differ, so the logarithms round differently: not the same bits)
    assert np.abs(ov.overlap[np.ix_(keep, keep)] - full.overlap[np.ix_(keep, keep)]).max() <= 1e-13
    assert np.abs(ov.log_norm[0][[0, 2]] - full.log_norm[0][[0, 2]]).max() <= 1e-13
    # a model that is zero altogether: its environments vanish, g = 0 and lg = -inf for its pairs
    gone = [np.zeros_like(t) for t in models[0]]
    g, lg, _ = OV.overlaps_raw(eng, [gone, models[1]], None, False)
    assert np.all(g[:2] == 0) and np.all(np.isneginf(lg[:2])) and np.isfinite(lg[2]) and not np.any(np.isnan(g))


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------------------
def test_abi_errors(eng):
    models, _, _ = case("chi7_mid", False)
    lib = eng.lib
    before = _raw_by_pair(eng, models, None, False)
    abi = [mt.engine.model_to_abi(m, None) for m in models]
    arr = (L.ImputeModel * 3)(*[a[0] for a in abi])
    g, lg = np.zeros((6, 3, 3)), np.zeros(6)
    gp, lp = g.ctypes.data_as(DP), lg.ctypes.data_as(DP)
    call = lambda m=arr, K=3, pairs=None, P=0, go=gp, lo=lp: lib.mpst_model_overlaps(eng.ctx, m, K, pairs, P, go, lo, None)
    assert call() == 0                                                         # seconds may be NULL
    assert call(m=None) == L.MPST_ERR_INVALID and call(go=None) == L.MPST_ERR_INVALID and call(lo=None) == L.MPST_ERR_INVALID
    assert lib.mpst_model_overlaps(None, arr, 3, None, 0, gp, lp, None) == L.MPST_ERR_INVALID
    assert call(K=0) == L.MPST_ERR_INVALID
    for bad in ([0, 3], [-1, 0]):
        t = np.array([bad], dtype=np.int32)
        assert call(pairs=t.ctypes.data_as(IP), P=1) == L.MPST_ERR_INVALID

    def with_field(k, **kw):
        a = (L.ImputeModel * 3)(*[x[0] for x in abi])
        for name, v in kw.items():
            setattr(a[k], name, v)
        return a

    assert call(m=with_field(1, T=9)) == L.MPST_ERR_INVALID
    assert call(m=with_field(2, d=5)) == L.MPST_ERR_INVALID
    assert call(m=with_field(1, label_site=4)) == L.MPST_ERR_INVALID
    assert call(m=with_field(2, dtype=1)) == L.MPST_ERR_INVALID
    assert call(m=with_field(0, compute=1)) == L.MPST_ERR_UNSUPPORTED
    assert call(m=with_field(0, C=17)) == L.MPST_ERR_UNSUPPORTED
    for field, value in (("chi", 129), ("d", 17)):
        chi = np.array([1] + [129 if field == "chi" else 4] * 9 + [1], dtype=np.int32)
        a = with_field(0, chi=chi.ctypes.data_as(IP)) if field == "chi" else (L.ImputeModel * 3)(*[with_field(0, d=17)[0]] * 3)
        assert call(m=a) == L.MPST_ERR_UNSUPPORTED, field
    chi = np.array([1] + [100] * 9 + [1], dtype=np.int32)                      # d chi = 1100 > 1024 with d = 11 on every model
    a = (L.ImputeModel * 3)(*[with_field(0, d=11, chi=chi.ctypes.data_as(IP))[0]] * 3)
    assert call(m=a) == L.MPST_ERR_UNSUPPORTED
    after = _raw_by_pair(eng, models, None, False)                             # a valid call right after the rejected ones: the same bits
    for q in before:
        assert np.array_equal(before[q][0], after[q][0]) and before[q][1] == after[q][1]
    # the Python layer refuses before any device work
    other = gaussian_chain(10, 6, 7, 3, 4, False, np.random.default_rng(0))
    with pytest.raises(ValueError):
        mt.model_overlaps([models[0], other], engine=eng)
    with pytest.raises(ValueError):
        mt.model_overlaps([models[0], [t.astype(np.complex128) for t in models[1]]], engine=eng)
    with pytest.raises(ValueError):
        mt.model_overlaps(models, pairs=[(0, 3)], engine=eng)
    half = mt.model_overlaps([[t.astype(np.float32) for t in models[0]]], engine=eng)        # fp32 models are upcast
    assert half.overlap.dtype == np.float64 and np.all(np.isfinite(half.overlap))
    only = mt.model_overlaps(models, pairs=[(0, 1)], engine=eng)               # pairs that were not asked for are NaN; the self pairs give the norms
    assert np.all(np.isnan(block(only, 0, 2))) and np.all(np.isnan(block(only, 1, 2))) and np.all(np.isfinite(block(only, 1, 0)))
    assert np.all(np.isfinite(block(only, 2, 2)))


# ---- end to end: a small Legendre fit --------------------------------------------------------------------------------------------------
def test_training_summary_end_to_end(eng):
    from oracle import ref_numpy as O
    from tests.test_gpu_split import _fit_data
    Xtr, ytr, Xte, yte = _fit_data()
    opts = mt.MPSOptions(encoding="legendre", d=4, chi_max=8, nsweeps=2, verbosity=-1)
    trained, info, te = mt.fitMPS(Xtr, ytr, Xte, yte, opts)
    out = io.StringIO()
    stats = mt.get_training_summary(trained, te, print_stats=True, io=out, engine=eng)
    log_norm, blocks = R.normalised_ref([trained.mps])
    norm = np.exp(log_norm[0])
    pred_train = np.argmax(np.abs(O.contract_mps(trained.mps, trained.train_data.phi)) / norm[None, :], axis=1)
    pred_test = np.argmax(np.abs(O.contract_mps(trained.mps, te.phi)) / norm[None, :], axis=1)
    ref = mt.training_stats(trained.train_data.label_index, pred_train, te.label_index, pred_test, 2)
    assert np.array_equal(stats["confmat"], ref["confmat"]) and stats["confmat"].sum() == len(Xte) and stats["confmat"].dtype.kind == "i"
    for key in ("train_acc", "test_acc", "test_balanced_acc", "precision", "recall", "specificity", "f1_score"):
        assert stats[key] == ref[key] or (np.isnan(stats[key]) and np.isnan(ref[key])), key
    assert np.abs(stats["overlapmat"] - np.abs(blocks[(0, 0)])).max() <= 1e-10
    text = out.getvalue()
    for word in ("Overlap Matrix", "Confusion Matrix", "|ψ0⟩", "⟨ψ1|", "Pred. |1⟩", "True |0⟩", "test_balanced_acc"):
        assert word in text, word
    # a raw matrix goes through the model's own preprocessing and gives the same predictions
    raw = mt.get_training_summary(trained, Xte[np.argsort(yte, kind="stable")], io=io.StringIO(), engine=eng, y_test=np.sort(yte))
    assert np.array_equal(raw["confmat"], stats["confmat"])
    table = mt.sweep_summary(info, io=io.StringIO())
    assert table.shape == (5, opts.nsweeps + 3)
