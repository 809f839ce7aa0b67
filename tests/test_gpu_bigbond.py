"""Bond tensors beyond 128 x 128: d*chi_max in (128, 1024] (row X1 of the round-1 verdict).  The reference's own
documented runs live here: chi_max=37, d=8 (docs/src/hyperparameters.md:65), chi_max=40, d=8 (:127), and BASELINE.json
configs[4] is chi_max=64, d=8.  Same tolerances as the small-bond parity tests; everything through the C ABI."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests.helpers import load_engine, make_problem, teacher_forced_segment, teacher_forced_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(engine_cls):
    e = engine_cls(0)
    yield e
    e.close()


@pytest.mark.parametrize("alg", [0, 2], ids=["blocked", "jacobi"])
@pytest.mark.parametrize("n", [130, 160, 296, 512, 1000])
def test_large_eigensolver_against_lapack(eng, n, alg):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((2 * n, n)) * (0.9 ** np.arange(n))
    G = A.T @ A
    lam, E, info = eng.selftest_eig(G, alg=alg)
    w, V = np.linalg.eigh(G)
    w, V = w[::-1], V[:, ::-1]
    K = min(n, 128)
    assert info == (-2 if alg == 2 else -3)        # -2: the multi-workgroup Jacobi fallback (no vendor solver is linked), -3: the hand-written blocked solver, both verified
    assert np.abs(lam[:K] - w[:K]).max() <= 1e-12 * w[0]
    Ek = E[:, :K]
    assert np.abs(Ek.T @ Ek - np.eye(K)).max() < 1e-12
    # eigenvector residual (sign / cluster-basis independent)
    assert np.abs(G @ Ek - Ek * lam[:K]).max() <= 1e-11 * w[0]


def test_blocked_eigensolver_hands_clusters_to_the_library(eng):
    """Exactly repeated kept eigenvalues: the twisted-factorisation vectors of a cluster are not orthogonal, the on-device
    verification must notice and the library solver must deliver."""
    rng = np.random.default_rng(5)
    n = 200
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam_true = np.concatenate([[5.0, 5.0, 5.0, 3.0, 3.0], 2.0 * 0.8 ** np.arange(n - 5)])
    G = (Q * lam_true) @ Q.T
    G = 0.5 * (G + G.T)
    lam, E, info = eng.selftest_eig(G)
    assert info in (-2, -3)
    K = 128
    assert np.abs(lam[:K] - np.sort(lam_true)[::-1][:K]).max() <= 1e-11 * 5.0
    Ek = E[:, :K]
    assert np.abs(Ek.T @ Ek - np.eye(K)).max() < 1e-10
    assert np.abs(G @ Ek - Ek * lam[:K]).max() <= 1e-10 * 5.0


CASES = [
    # N, T, d, chi_init, chi_max, C, loss, bbopt
    (64, 4, 8, 12, 20, 2, "KLD", "TSGO"),      # 160
    (48, 4, 6, 20, 30, 2, "MSE", "GD"),        # 180
    (40, 3, 12, 10, 14, 1, "KLD", "TSGO"),     # 168, d = 12 (hyperparameters.md:241)
    (96, 5, 8, 30, 37, 2, "KLD", "TSGO"),      # 296: chi_max = 37, d = 8 (hyperparameters.md:65)
]


def _bond_by_bond(eng, ds, W0, opts, T):
    """One sweep, every bond update compared with the restatement's on the same inputs; returns the oracle's final MPS."""
    load_engine(eng, ds, W0, opts)
    eng.build_caches()
    W = [t.copy() for t in W0]
    LE, RE = R.construct_caches(W, ds.phi, True)
    for going_left, order in ((True, range(T - 2, -1, -1)), (False, range(0, T - 1))):
        if not going_left:
            LE, RE = R.construct_caches(W, ds.phi, False)
        for lid in order:
            tr_o = {}
            R.bond_step(W, LE, RE, lid, ds, opts, going_left, tr_o)
            tr_g = eng.bond_step(lid, going_left)
            assert tr_g["chi"] == tr_o["chi"]
            assert abs(tr_g["loss"] - tr_o["loss"]) <= 1e-11 * max(1.0, abs(tr_o["loss"]))
            assert abs(tr_g["grad_norm"] - tr_o["grad_norm"]) <= 1e-11 * tr_o["grad_norm"]
            So = np.asarray(tr_o["S"])
            assert np.abs(np.asarray(tr_g["S"])[:len(So)] - So).max() <= 1e-9 * So[0]
            yo, yg = R.contract_mps(W, ds.phi), R.contract_mps(eng.get_mps(), ds.phi)
            assert np.abs(yg - yo).max() <= 1e-9 * np.abs(yo).max()
    return W


@pytest.mark.parametrize("case", CASES, ids=[f"dchi{c[2] * c[4]}" for c in CASES])
def test_big_bond_sweep_bond_by_bond(eng, case):
    N, T, d, chi0, chimax, C, loss, bbopt = case
    ds, W0 = make_problem(N, T, d, chi0, C, seed=N + d)
    opts = R.SweepOptions(nsweeps=1, chi_max=chimax, eta=0.05, loss_grad=loss, bbopt=bbopt)
    W = _bond_by_bond(eng, ds, W0, opts, T)
    mse, kld, acc, conf = eng.eval(0)
    mo, ko, ao, co = R.mse_loss_acc(W, ds, conf=True)
    assert abs(mse - mo) < 1e-9 and abs(kld - ko) < 1e-9 * max(1, abs(ko)) and acc == ao and np.array_equal(conf, co)
    # mpst_sweep + normalize! on the same problem (plain-stream path: the library call is not graph-captured)
    load_engine(eng, ds, W0, opts)
    eng.build_caches()
    eng.sweep()
    eng.normalize()
    Wo = [t.copy() for t in W0]
    R.sweep(Wo, ds, opts)
    Wo = R.normalize_mps(Wo)
    yo, yg = R.contract_mps(Wo, ds.phi), R.contract_mps(eng.get_mps(), ds.phi)
    assert np.abs(yg - yo).max() <= 1e-8 * np.abs(yo).max()
    assert abs(R.mps_norm(eng.get_mps()) - 1.0) < 1e-12


MANY = [
    # enough series for the 4-tiles-per-workgroup form of k_yhat_gen (from 1024 tiles of 16 series; the 2-tile form is what
    # test_config5_shape_chi64_d8_teacher_forced runs) and for k_grad workgroups that walk many chunks; three classes
    # whose sizes are no multiple of the tile group, so that groups straddle class boundaries
    (16550, 4, 9, 10, 15, 3, "KLD", "TSGO"),
    (16550, 4, 9, 10, 15, 3, "MSE", "GD"),
]


@pytest.mark.parametrize("case", MANY, ids=[f"N{c[0]}_{c[6]}" for c in MANY])
def test_big_bond_many_series(eng, case):
    """Every bond of one sweep, each update started from the C oracle's state (free-running trajectories drift apart:
    a 1e-9 difference in one bond's gradient - a sum with heavy cancellation over 16 k series - is amplified bond by
    bond)."""
    from oracle.c_oracle import COracle
    N, T, d, chi0, chimax, C, loss, bbopt = case
    ds, W0 = make_problem(N, T, d, chi0, C, seed=N + d)
    opts = R.SweepOptions(nsweeps=1, chi_max=chimax, eta=0.05, loss_grad=loss, bbopt=bbopt)
    load_engine(eng, ds, W0, opts)
    assert np.bincount(ds.label_index).tolist() == [5517, 5517, 5516]       # 345 tiles per class: 345 % 4 != 0
    co = COracle(W0, ds.phi, ds.label_index, ds.class_distribution, chimax, eta=0.05, loss=loss, bbopt=bbopt, rebuild_caches=False)
    co.build_caches(around_label=True)
    worst, flips = teacher_forced_sweep(eng, co, ds.phi, T, overlap_every=2)
    assert worst["loss"] < 1e-10 and worst["grad"] < 1e-8 and worst["S"] < 1e-9 and worst["overlap"] < 1e-8, worst
    assert flips <= 1
    assert eng.info()["large_bond"]


def _trendy(N, T, d, C):
    rng = np.random.default_rng(7)
    if C == 2:
        X1, _ = mt.trendy_sine(T, N // 2, period=(12.0, 15.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
        X2, _ = mt.trendy_sine(T, N - N // 2, period=(16.0, 19.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
        X = np.concatenate([X1, X2])
        y = np.concatenate([np.ones(N // 2, dtype=np.int64), 2 * np.ones(N - N // 2, dtype=np.int64)])
        keys = {1: 0, 2: 1}
    else:
        X, _ = mt.trendy_sine(T, N, period=(12.0, 19.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
        y = np.zeros(N, dtype=np.int64)
        keys = {0: 0}
    opts = mt.MPSOptions(d=d, encoding="Legendre", verbosity=-1)
    enc = mt.model_encoding(opts.encoding)
    Xs, _ = mt.transform_train_data(X, opts, enc.range)
    return mt.encode_dataset(X, Xs, y, enc, d, keys)


def test_documented_run_chi37_d8_teacher_forced(engine_cls):
    """The reference's logged classification run (docs/src/hyperparameters.md:65-74): noisy trendy sine, N=240 of 300,
    T=100, chi_max=37, d=8, two classes.  Teacher-forced against the C oracle where the sweep starts and over 12 bulk
    bonds of the forward half-sweep (d*chi = 296)."""
    from oracle.c_oracle import COracle
    N, T, d, chi, C = 240, 100, 8, 37, 2
    full = _trendy(N, T, d, C)
    W0 = mt.generate_startingMPS(4, T, d, C, 1234)
    mk = lambda W: COracle(W, full.phi, full.label_index, full.class_distribution, chi, eta=0.01, rebuild_caches=False)
    eng = engine_cls(0)
    try:
        eng.set_options(chi_max=chi, eta=0.01)
        eng.set_dataset(0, full.phi, full.label_index, C)
        for first, count in ((0, 10), (150, 12)):
            worst, flips = teacher_forced_segment(eng, mk, W0, full.phi, T, first, count)
            assert worst["loss"] < 1e-10 and worst["grad"] < 1e-8 and worst["S"] < 1e-9 and worst["overlap"] < 1e-8, (first, worst)
            assert flips <= 1
        chi_now, _ = eng.get_chi()
        assert chi_now.max() == chi
    finally:
        eng.close()


def test_config5_shape_chi64_d8_teacher_forced(engine_cls):
    """BASELINE.json configs[4]'s bond shape in real fp64: chi_max=64, d=8 (d*chi = 512), N=8192, one class (the
    imputation setting).  T is cut to 24 sites so that the single-threaded C oracle finishes in about a minute; the
    bond kernels see the full 512 x 512 bond tensor from the third site on."""
    from oracle.c_oracle import COracle
    N, T, d, chi, C = 8192, 24, 8, 64, 1
    full = _trendy(N, T, d, C)
    W0 = mt.generate_startingMPS(4, T, d, C, 1234)
    mk = lambda W: COracle(W, full.phi, full.label_index, full.class_distribution, chi, eta=0.01, rebuild_caches=False)
    eng = engine_cls(0)
    sub = slice(0, N, 64)
    try:
        eng.set_options(chi_max=chi, eta=0.01)
        eng.set_dataset(0, full.phi, full.label_index, C)
        for first, count in ((0, 3), (T - 1 + 8, 3)):
            worst, flips = teacher_forced_segment(eng, mk, W0, full.phi, T, first, count, sub=sub, overlap_every=1)
            assert worst["loss"] < 1e-10 and worst["grad"] < 1e-8 and worst["S"] < 1e-9 and worst["overlap"] < 1e-8, (first, worst)
            assert flips <= 1
        chi_now, _ = eng.get_chi()
        assert chi_now.max() == chi
    finally:
        eng.close()


def test_limits_are_reported(engine_cls):
    e = engine_cls(0)
    try:
        e.set_options(chi_max=140)
        phi = np.random.default_rng(0).uniform(-1, 1, (8, 4, 4))
        e.set_dataset(0, phi, np.zeros(8, dtype=int), 1)
        e.set_mps(mt.generate_startingMPS(2, 4, 4, 1, 0))
        with pytest.raises(mt.MPSTError, match="exceeds the engine's limits"):
            e.build_caches()
    finally:
        e.close()


def test_blocked_tridiagonalisation_is_deterministic(eng):
    """Regression: the Householder step kernel runs on many workgroups with no barrier between them inside a launch; the
    vector y of a step used to share one buffer with the previous step's (a fast workgroup overwrote what a slow one was
    still reading: 1 sweep in ~150 wrong).  Now double-buffered: 200 repetitions of a small sweep, bit-identical."""
    N, T, d, chi0, chimax, C = 40, 3, 12, 10, 14, 1
    ds, W0 = make_problem(N, T, d, chi0, C, seed=N + d)
    opts = R.SweepOptions(nsweeps=1, chi_max=chimax, eta=0.05, loss_grad="KLD", bbopt="TSGO")
    first = None
    for rep in range(200):
        load_engine(eng, ds, W0, opts)
        eng.build_caches()
        eng.sweep()
        W = eng.get_mps()
        if first is None:
            first = W
            Wo = [t.copy() for t in W0]
            R.sweep(Wo, ds, opts)
            yo, yg = R.contract_mps(Wo, ds.phi), R.contract_mps(W, ds.phi)
            assert np.abs(yg - yo).max() <= 1e-8 * np.abs(yo).max()
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, W)), rep
    info = eng.info()
    # the persistent tridiagonalisation carried every bond (it hands a bond back only when its workgroups cannot all
    # become resident), and nothing needed the library solver
    assert info["large_bond"] and info["persistent_tridiag_aborts"] == 0 and info["library_eig_fallbacks"] == 0


@pytest.mark.parametrize("dtype", ["float64", "complex128"])
def test_sweep_reads_the_verdict_once_and_redoes_a_failed_sweep(engine_cls, dtype):
    """Large bonds: mpst_sweep no longer synchronises with the host after every bond to read the eigensolver's verdict - it
    reads a sticky word once per sweep and, if any bond failed, redoes the sweep from a snapshot bond by bond (with the
    library fallback).  MPST_BIG_FORCE_FAIL=n marks the n-th solve of the training workspace as failed (the count restarts, and the variable is read
    again, whenever the workspace is rebuilt): the redone sweep, and the sweep after it, must give
    the bits of a context that reads the verdict after every bond (MPST_BIG_SYNC=1).  float64 goes through the real reduction on
    one XCD; complex128 (one class, complex order 160, subspace block 64) through the Hermitian reduction from both launchers,
    the complex subspace sequence and its Rayleigh-Ritz launch."""
    import os
    N, T, d, chi0, chimax = 96, 5, 8, 14, 20                # d*chi = 160 > 128
    if dtype == "float64":
        ds, W0 = make_problem(N, T, d, chi0, 2, seed=3)
    else:
        from oracle import ref_complex as RC
        ds, W0 = RC.make_problem(N, T, d, chi0, 1, seed=3, dtype=np.complex128)
    opts = R.SweepOptions(nsweeps=2, chi_max=chimax, eta=0.05, loss_grad="KLD", bbopt="TSGO")

    def run(env):
        old = {k: os.environ.get(k) for k in ("MPST_BIG_FORCE_FAIL", "MPST_BIG_SYNC")}
        for k in old:
            os.environ.pop(k, None)
        os.environ.update(env)
        e = engine_cls(0)
        try:
            load_engine(e, ds, W0, opts)
            e.build_caches()
            st = [e.sweep() for _ in range(2)]
            return e.get_mps(), e.info(), e.loss_trace() if hasattr(e, "loss_trace") else None, st
        finally:
            e.close()
            for k, val in old.items():
                os.environ.pop(k, None)
                if val is not None:
                    os.environ[k] = val

    W_sync, i_sync, _, _ = run({"MPST_BIG_SYNC": "1"})
    W_opt, i_opt, _, _ = run({})
    W_redo, i_redo, _, _ = run({"MPST_BIG_FORCE_FAIL": "3"})
    assert not i_sync["large_bond_verdict_per_sweep"] and i_opt["large_bond_verdict_per_sweep"]
    assert i_opt["large_bond_sweep_redos"] == 0 and i_redo["large_bond_sweep_redos"] == 1
    assert all(np.array_equal(a, b) for a, b in zip(W_sync, W_opt))
    assert all(np.array_equal(a, b) for a, b in zip(W_sync, W_redo))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_subspace_eigensolver_is_used_certified_and_agrees_with_lapack(dtype):
    """Large real bonds go through the randomised subspace solver first (csrc/mpst_eig_subspace.inl: GEMM half-steps through the bond
    matrix + a (C chi + 32)-dimensional Rayleigh-Ritz problem), its result is certified on the device against the Gram matrix and the
    exact Householder solver takes every bond the certificate rejects.  On structured data (the reference's noisy trendy sines,
    toy_data.jl:68-71) after the growth phase nearly every bond must be ACCEPTED, and accepted or not every bond must agree with the
    LAPACK-based restatement (decomposeBT, RealRealHighDimension.jl:146-203) to the usual tolerances: teacher forced, second sweep."""
    from oracle import ref_complex as RC
    from tests.test_gpu_typed import TOL, caches_around, two_site
    from tests.helpers import bond_of
    rng = np.random.default_rng(2)
    N, T, d, chi = 768, 10, 8, 24                      # n = d chi = 192 >= 2 (C chi + 32) = 160
    X, y = R.trendy_sine_dataset(N, T, rng)
    Xs, _ = R.transform_train_data(X)
    ds = R.encode_dataset(X, Xs, y, lambda x: R.legendre_encode(x, d), (-1, 1))
    W = R.random_mps(T, d, 4, 2, np.random.default_rng(7))
    opts = R.SweepOptions(chi_max=chi, eta=0.01)
    dt = np.dtype(dtype)
    eng = mt.SweepEngine(0)
    try:
        eng.set_options(chi_max=chi, eta=0.01)
        eng.set_dataset(0, ds.phi.astype(dt), ds.label_index, 2, dtype=dt)
        eng.set_mps([t.astype(dt) for t in W])
        eng.build_caches()
        eng.sweep()                                     # growth phase: the engine free-runs (rejections are expected here)
        i0 = eng.info()
        assert i0["large_bond"] and i0["subspace_attempted"] > 0
        W1 = [np.asarray(t).astype(np.float64) for t in eng.get_mps()]
        ds64 = R.EncodedSet(ds.phi.astype(dt).astype(np.float64), ds.label_index, ds.class_distribution)
        tol = TOL["f32" if dtype == "float32" else "f64"]
        worst = dict(loss=0.0, grad=0.0, S=0.0, bond=0.0)
        Wo = [t.copy() for t in W1]
        for q in range(2 * (T - 1)):
            lid, gl = bond_of(q, T)
            ls = lid + 1 if gl else lid
            eng.set_mps([t.astype(dt) for t in Wo], label_site=ls)
            eng.build_caches()
            LE, RE = caches_around(Wo, ds64.phi, ls)
            tr = {}
            RC.bond_step(Wo, LE, RE, lid, ds64, opts, gl, tr)
            got = eng.bond_step(lid, gl)
            assert got["chi"] == tr["chi"], (q, got["chi"], tr["chi"])
            worst["loss"] = max(worst["loss"], abs(got["loss"] - tr["loss"]) / max(1.0, abs(tr["loss"])))
            worst["grad"] = max(worst["grad"], abs(got["grad_norm"] - tr["grad_norm"]) / tr["grad_norm"])
            worst["S"] = max(worst["S"], np.abs(got["S"][:tr["chi"]] - tr["S"]).max() / tr["S"][0])
            Wg = eng.get_mps()
            a, b = two_site(Wg[lid], Wg[lid + 1]), two_site(Wo[lid], Wo[lid + 1])
            worst["bond"] = max(worst["bond"], np.abs(a - b).max() / np.abs(b).max())
        i1 = eng.info()
        att, acc = i1["subspace_attempted"] - i0["subspace_attempted"], i1["subspace_accepted"] - i0["subspace_accepted"]
        print(dtype, "second sweep: subspace attempted", att, "accepted", acc, worst)
        assert att >= 2 * (T - 1) - 6 and acc >= att - 3, (att, acc)      # the bonds next to the chain's ends are small (exact solver)
        assert i1["library_eig_fallbacks"] == 0
        for k in tol:
            # (||grad||: a sum of 768 fp32 products whose cancellation depends on the state the free-running first sweep left)
            assert worst[k] < (3.0 if (k == "grad" and dtype == "float32") else 1.0) * tol[k], (k, worst)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_subspace_eigensolver_complex_bonds(dtype):
    """The same for a complex model (Fourier encoding, one class - BASELINE configs[4]'s kind of fit): complex GEMM half-steps, Hermitian
    elimination, Rayleigh-Ritz through the native pair-mode chain; accepted bonds and handed-back bonds alike agree with the
    double-precision restatement of the legacy engine (oracle/ref_complex.py), teacher forced over the second sweep."""
    import bench
    from oracle import ref_complex as RC
    from tests.test_gpu_typed import TOL, caches_around, two_site
    from tests.helpers import bond_of
    N, T, d, chi = 512, 8, 8, 24                       # n = d chi = 192 complex columns, block 24 + 32 -> 64
    full = bench.typed_inputs(N, T, d, 1, True)
    dt = np.dtype(dtype)
    W = mt.generate_startingMPS(4, T, d, 1, 1234, np.complex128)
    opts = RC.SweepOptions(chi_max=chi, eta=0.01)
    phi = np.asarray(full.phi).astype(dt)
    eng = mt.SweepEngine(0)
    try:
        eng.set_options(chi_max=chi, eta=0.01)
        eng.set_dataset(0, phi, full.label_index, 1, dtype=dt)
        eng.set_mps([t.astype(dt) for t in W])
        eng.build_caches()
        eng.sweep()
        i0 = eng.info()
        assert i0["large_bond"] and i0["typed_kernels"] and i0["subspace_attempted"] > 0
        Wo = [np.asarray(t).astype(np.complex128) for t in eng.get_mps()]
        ds64 = RC.EncodedSet(phi.astype(np.complex128), np.asarray(full.label_index), np.asarray(full.class_distribution))
        tol = TOL["f32" if dtype == "complex64" else "f64"]
        worst = dict(loss=0.0, grad=0.0, S=0.0, bond=0.0)
        for q in range(2 * (T - 1)):
            lid, gl = bond_of(q, T)
            ls = lid + 1 if gl else lid
            eng.set_mps([t.astype(dt) for t in Wo], label_site=ls)
            eng.build_caches()
            LE, RE = caches_around(Wo, ds64.phi, ls)
            tr = {}
            RC.bond_step(Wo, LE, RE, lid, ds64, opts, gl, tr)
            got = eng.bond_step(lid, gl)
            assert got["chi"] == tr["chi"], (q, got["chi"], tr["chi"])
            worst["loss"] = max(worst["loss"], abs(got["loss"] - tr["loss"]) / max(1.0, abs(tr["loss"])))
            worst["grad"] = max(worst["grad"], abs(got["grad_norm"] - tr["grad_norm"]) / tr["grad_norm"])
            worst["S"] = max(worst["S"], np.abs(got["S"][:tr["chi"]] - tr["S"]).max() / tr["S"][0])
            Wg = eng.get_mps()
            a, b = two_site(Wg[lid], Wg[lid + 1]), two_site(Wo[lid], Wo[lid + 1])
            worst["bond"] = max(worst["bond"], np.abs(a - b).max() / np.abs(b).max())
        i1 = eng.info()
        att, acc = i1["subspace_attempted"] - i0["subspace_attempted"], i1["subspace_accepted"] - i0["subspace_accepted"]
        print(dtype, "second sweep: subspace attempted", att, "accepted", acc, worst)
        assert att >= 2 * (T - 1) - 6 and acc >= att - 4, (att, acc)
        assert i1["library_eig_fallbacks"] == 0
        for k in tol:
            assert worst[k] < tol[k], (k, worst)
    finally:
        eng.close()


# ---- every documented route of the large-bond eigensolver, one child process per setting (the switches are read once per process) ----
ROUTE_SETTINGS = [
    # id, complex problem, environment
    ("real-default", False, {}),
    ("real-no-xcd", False, {"MPST_BT_NO_XCD": "1"}),
    ("real-no-tail", False, {"MPST_BT_NO_TAIL": "1"}),
    ("real-no-subspace", False, {"MPST_NO_SUBSPACE": "1"}),
    ("complex-default", True, {}),
    ("complex-no-cnative", True, {"MPST_BT_NO_CNATIVE": "1"}),
    ("complex-counted", True, {"MPST_BT_C_XCD": "counted"}),
]
ROUTE_SWITCHES = sorted({k for _, _, env in ROUTE_SETTINGS for k in env})


def _route_problem(cx):
    if cx:
        from oracle import ref_complex as RC
        ds, W0 = RC.make_problem(96, 5, 8, 14, 1, seed=3, dtype=np.complex128)      # the complex shape of the verdict test above
        return ds, W0, R.SweepOptions(nsweeps=1, chi_max=20, eta=0.05, loss_grad="KLD", bbopt="TSGO")
    N, T, d, chi0, chimax, C, loss, bbopt = CASES[0]
    ds, W0 = make_problem(N, T, d, chi0, C, seed=N + d)
    return ds, W0, R.SweepOptions(nsweeps=1, chi_max=chimax, eta=0.05, loss_grad=loss, bbopt=bbopt)


def _route_child(cx, out):
    """Runs in the child: one sweep (and normalize for the real problem) under the child's environment -> MPS and info() in `out`."""
    ds, W0, opts = _route_problem(cx)
    eng = mt.SweepEngine(0)
    try:
        load_engine(eng, ds, W0, opts)
        eng.build_caches()
        eng.sweep()
        if not cx:
            eng.normalize()
        info = eng.info()
        W = eng.get_mps()
    finally:
        eng.close()
    np.savez(out, *W, info=np.array([info["large_bond"], info["library_eig_fallbacks"], info["subspace_attempted"],
                                     info["persistent_tridiag_aborts"], info["xcd_local_misplaced"]], dtype=np.int64))


def test_every_documented_route_of_the_large_bond_eigensolver(tmp_path):
    """Default, MPST_BT_NO_XCD, MPST_BT_NO_TAIL, MPST_NO_SUBSPACE on CASES[0] (real, d*chi = 160, two classes) and default,
    MPST_BT_NO_CNATIVE, MPST_BT_C_XCD=counted on a complex problem (one class, complex order 160): one sweep each in a child process
    of its own, one after the other, against the CPU restatement's sweep.  Real: overlaps after normalize within 1e-8 of the largest
    (the bound of test_big_bond_sweep_bond_by_bond at this shape).  Complex: overlaps within TOL["f64"]["bond"] = 1e-8 of the
    largest (gauge invariant, unlike the two-site tensors of a free-running chain).  Every setting's deviation is printed before it
    is asserted; profiles/eig_host_refactor.txt records what was measured."""
    import os
    import subprocess
    import sys
    from oracle import ref_complex as RC
    from tests.test_gpu_typed import TOL
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = {}
    for cx in (False, True):
        ds, W0, opts = _route_problem(cx)
        Wo = [t.copy() for t in W0]
        (RC if cx else R).sweep(Wo, ds, opts)
        ref[cx] = (ds, R.contract_mps(Wo if cx else R.normalize_mps(Wo), ds.phi))
    base = {k: v for k, v in os.environ.items() if k not in ROUTE_SWITCHES}
    base["PYTHONPATH"] = root + os.pathsep + os.environ.get("PYTHONPATH", "")
    for name, cx, env in ROUTE_SETTINGS:
        out = str(tmp_path / (name + ".npz"))
        code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_bigbond import _route_child; _route_child(%r, %r)" % (root, cx, out)
        run = subprocess.run([sys.executable, "-c", code], env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, (name, run.stderr[-2000:])
        with np.load(out) as z:
            W = [z["arr_%d" % j] for j in range(len(z.files) - 1)]
            large, fallbacks, attempted, aborts, misplaced = (int(x) for x in z["info"])
        ds, yo = ref[cx]
        dev = np.abs(R.contract_mps(W, ds.phi) - yo).max() / np.abs(yo).max()
        print(f"{name}: deviation {dev:.3e}, subspace_attempted {attempted}, persistent_tridiag_aborts {aborts}, xcd_local_misplaced {misplaced}")
        assert large and fallbacks == 0, (name, large, fallbacks)
        assert (attempted == 0) if "MPST_NO_SUBSPACE" in env else (attempted > 0), (name, attempted)
        assert dev <= (TOL["f64"]["bond"] if cx else 1e-8), (name, dev)
