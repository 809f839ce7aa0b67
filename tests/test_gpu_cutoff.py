"""Cutoff-limited bonds on every launch chain against the oracle.

Every other oracle comparison of the suite runs at cutoff = 1e-10 on uniform-random series, whose flat spectrum the relative-cutoff rule
(NDTensors truncate!, oracle/ref_numpy.py truncate_spectrum) never cuts: the kept dimension is min(chi_max, full rank), the same on every
bulk bond, and a multiple of 4 whenever chi_max is.  Here the cutoff is 1e-3 (1e-4, 1e-2): bond dimensions differ from site to site, are
mostly no multiple of the MFMA granule of 4, shrink from one half-sweep to the next and reach 1 - the regime of the extents rounded to 4
(KP, ZP in k_bond_tail), of the addresses clamped to cap - 1 and of the masks by live dimension.  tests/test_cutoff_inputs.py asserts, on
the CPU, that the cases below really are in that regime.

The pattern is tests/fuzz_sweep_oracle.py::one over TWO sweeps (the second starts from the ragged profile the first one left): per bond
set_mps(oracle state) + build_caches, one bond_step, compared with the oracle's bond_step from the same state; after each bond the updated
MPS as overlaps with every series.  Tolerances: tests/test_gpu_parity.py (fp64: loss 1e-11, ||grad|| 1e-10, S 1e-9 sigma_1, overlaps 1e-9)
and the TOL table of tests/test_gpu_typed.py.  The kept dimension is exact in fp64 / complex128: the smallest decision margin
(tests/helpers.py truncation_margin) of any case is 1e-5 of the threshold, the Gram route's error 1e-13 of it.  In float32 / complex64 a
flip by one state is excused on a bond whose margin lies below

    Delta = 2 tol_S sigma_1 sum_{i >= n-1} s_i / (cutoff sum s^2)

(the change of the discarded weight when every discarded value moves by the S tolerance), on at most a quarter of a case's bonds.

Every case asserts with info() that its route ran (an environment switch that resolves to the default chain fails the test)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_complex as RC
from oracle import ref_numpy as R
from tests.helpers import _env, bond_of, load_engine, make_problem, truncation_margin
from tests.test_gpu_typed import DT, TOL, caches_around, problem, two_site

pytestmark = pytest.mark.gpu

F64 = dict(loss=1e-11, grad=1e-10, S=1e-9, overlap=1e-9)         # tests/test_gpu_parity.py
PAIR = dict(loss=1e-11, grad=1e-8, S=1e-8)                       # second bond of a pair: its yhat comes from the first bond's tail launch
TOL_S_F32 = TOL["f32"]["S"]


def _case(id, route, N, T, d, chi, C, cutoff=1e-3, seed=0, env=None, flags=None, collapse=False, sweeps=2, unmet=(), **opts):
    """A Float64 case: make_problem(N, T, d, 4, C, seed, balanced=False), eta = 0.05 unless given.  ``env``: the switches that select the
    route; ``flags``: what info() must report; ``collapse``: the deliberately degenerate case (every bond ends at dimension 1); ``unmet``: the
    input conditions of tests/test_cutoff_inputs.py this shape cannot meet at any seed (each with its reason where the case is listed)."""
    o = dict(eta=0.05)
    o.update(opts)
    return SimpleNamespace(id=id, route=route, N=N, T=T, d=d, chi=chi, C=C, cutoff=cutoff, seed=seed, env=env or {}, flags=flags or {},
                           collapse=collapse, sweeps=sweeps, unmet=frozenset(unmet), opts=tuple(sorted(o.items())), dtype="float64", typed=False)


FOUR = dict(four_launch_chain=True, fused=True, tail_redos=0)
SIX = dict(four_launch_chain=False, fused=True)
HEAD = (531, 12, 4, 32, 2)      # 34 tile workgroups of the full-capacity d = 4 tail launch, the last tile holds 3 series
F64_CASES = [
    _case("four_N531", "four", *HEAD, seed=3, flags=FOUR),
    # (a finer cutoff on the same shape saturates at chi_max during the first forward half-sweep - final profile 4,16,32,...,32,8 at each of
    # 40 seeds: no bond below the cap in the second sweep, at most 10 of 44 bonds off the granule)
    _case("four_N531_1e-4", "four", *HEAD, cutoff=1e-4, seed=3, flags=FOUR, unmet=("quarter_unaligned", "below_cap_in_each_half_sweep")),
    # (one class, d = 6: the profile grows monotonically over both sweeps at each of 40 seeds)
    _case("four_d6_C1", "four", 120, 9, 6, 16, 1, seed=3, flags=FOUR, unmet=("shrinks",)),
    _case("four_d11", "four", 64, 8, 11, 11, 2, seed=3, flags=FOUR),
    _case("four_separately", "four", 200, 10, 4, 32, 3, seed=3, flags=FOUR, train_classes_separately=True),
    _case("six_N531", "six", *HEAD, seed=3, env=dict(MPST_CHAIN4=0), flags=SIX),
    _case("six_mse_tsgo", "six", 200, 10, 4, 32, 2, seed=3, flags=SIX, loss_grad="MSE", bbopt="TSGO"),
    _case("six_iters2", "six", 200, 10, 4, 32, 2, seed=3, flags=SIX, update_iters=2),
    _case("six_d2_chi64", "six", 150, 10, 2, 64, 2, seed=3, flags=SIX),
    # (MSE / GD at eta = 0.5: the second sweep takes every bond from 4 ... 12 down to 1 - Gram matrices of rank 1, the mindim branch, K0 < 4 -,
    # the third runs on the all-ones chain)
    _case("six_gd_collapse", "six", 200, 10, 4, 32, 2, seed=3, flags=SIX, collapse=True, sweeps=3, loss_grad="MSE", bbopt="GD", eta=0.5),
    _case("persistent_pair", "persistent", 300, 9, 4, 32, 2, seed=3, env=dict(MPST_B2=0), flags=dict(sliced_bond_gemms=False, fused=True)),
    _case("unfused_rescale", "unfused", 200, 10, 4, 32, 2, seed=3, flags=dict(fused=False, large_bond=False), rescale=(True, True)),
    _case("unfused_switch", "unfused", 200, 10, 4, 32, 2, seed=3, env=dict(MPST_NO_FUSED=1), flags=dict(fused=False, large_bond=False)),
    _case("large_bond", "large", 300, 9, 4, 40, 2, seed=3, flags=dict(large_bond=True)),
]
PAIR_CASES = [c for c in F64_CASES if c.id in ("four_N531", "four_d6_C1")]
FREE_CASE = F64_CASES[2]


def _typed(N, T, d, chi, C, cutoff, dtype):
    """An element-typed case: RC.make_problem with seed 11 (the seed is part of the case).  At this seed some of the six (shape, cutoff)
    pairs miss a condition of the ragged regime: TYPED_UNMET names them."""
    big = (2 if dtype.startswith("complex") else 1) * d * chi > 128      # complex Gram matrices arrive as embeddings of twice the dimension
    return SimpleNamespace(id=f"{dtype}_N{N}_chi{chi}_{cutoff:g}", route="typed", N=N, T=T, d=d, chi=chi, C=C, cutoff=cutoff, seed=11, env=dict(MPST_TYPED=1)
                           if dtype == "float64" else {}, flags=dict(typed_kernels=True, large_bond=big), collapse=False, sweeps=2, unmet=frozenset(TYPED_UNMET.get((N, cutoff, dtype.startswith("complex")), ())),
                           opts=(("eta", 0.05),), dtype=dtype, typed=True)


# (N, cutoff, complex) -> conditions.  Fourier states, seed 11: chi_max = 16 is reached on every bulk bond in the first forward half-sweep
# (7 of 32 bonds off the granule); cutoff 1e-2 on the d = 4 Fourier chain keeps 3 or 4 states everywhere (profile 3,4,4,4,4,4,4)
TYPED_UNMET = {(130, 1e-3, True): ("quarter_unaligned",), (96, 1e-2, True): ("distinct", "quarter_unaligned", "shrinks")}
TYPED_SHAPES = [(130, 9, 4, 16, 2), (100, 8, 3, 24, 3), (96, 8, 4, 40, 2)]       # the last: d chi_max = 160, the blocked solver in pair mode
TYPED_CASES = [_typed(*s, cutoff, dt) for dt in ("complex128", "float64", "complex64", "float32") for s in TYPED_SHAPES for cutoff in (1e-3, 1e-2)]
ALL_CASES = F64_CASES + TYPED_CASES
NSWEEPS = 2


def sweep_options(case):
    return R.SweepOptions(nsweeps=1, chi_max=case.chi, cutoff=case.cutoff, **dict(case.opts))


def case_problem(case):
    """(data set, starting MPS) in double precision - for float32 / complex64 rounded to that type first (tests/test_gpu_typed.py)."""
    if case.typed:
        return problem(case.N, case.T, case.d, min(4, case.chi), case.C, case.seed, DT[case.dtype])
    return make_problem(case.N, case.T, case.d, 4, case.C, seed=case.seed, balanced=False)


@functools.lru_cache(maxsize=8)
def _oracle_run(N, T, d, chi, C, cutoff, seed, opts, dtype, typed, sweeps):
    case = SimpleNamespace(N=N, T=T, d=d, chi=chi, C=C, cutoff=cutoff, seed=seed, opts=opts, dtype=dtype, typed=typed)
    ds, W0 = case_problem(case)
    so = sweep_options(case)
    W = [t.copy() for t in W0]
    recs = []
    for sweep in range(sweeps):
        LE = RE = None
        for q in range(2 * (T - 1)):
            lid, gl = bond_of(q, T)
            before = [t.copy() for t in W]
            tr = {}
            if typed:
                LE, RE = caches_around(W, ds.phi, lid + 1 if gl else lid)
                RC.bond_step(W, LE, RE, lid, ds, so, gl, tr)
                tr.pop("bt_new", None)
            else:
                if q in (0, T - 1):
                    LE, RE = R.construct_caches(W, ds.phi, gl)
                R.bond_step(W, LE, RE, lid, ds, so, gl, tr)
            margin, n = truncation_margin(tr["S_all"], chi, cutoff)
            assert n == tr["chi"]
            recs.append(dict(sweep=sweep, q=q, lid=lid, going_left=gl, W=before, tr=tr, margin=margin, full_rank=len(tr["S_all"]),
                             bond=two_site(W[lid], W[lid + 1]) if typed else None, y=None if typed else R.contract_mps(W, ds.phi)))
    for r in recs:
        for a in r["W"]:
            a.setflags(write=False)
    return ds, recs, W


def oracle_run(case):
    """The oracle's trajectory over the case's sweeps, computed once per problem and shared, never modified: (data set, one record per
    bond - the MPS before the bond, the oracle's trace with the full spectrum S_all, the decision margin, the updated model as overlaps
    (Float64 cases) or as the two-site tensor (typed cases) -, the final MPS)."""
    return _oracle_run(case.N, case.T, case.d, case.chi, case.C, case.cutoff, case.seed, case.opts, case.dtype, case.typed, case.sweeps)


def excusable(rec, cutoff, tol_s=TOL_S_F32):
    """Whether a flip of the kept dimension by one state is excused on this bond in float32 / complex64: the oracle's decision margin lies
    below Delta, the relative change of the discarded weight when every discarded value (and the last kept one) moves by tol_s sigma_1."""
    S = rec["tr"]["S_all"]
    n = rec["tr"]["chi"]
    delta = 2.0 * tol_s * S[0] * S[max(n - 1, 0):].sum() / (cutoff * np.sum(S ** 2))
    return rec["margin"] < delta


def _where(case, rec):
    W = rec["W"]
    lid = rec["lid"]
    return (f"{case.id}: sweep {rec['sweep']}, bond {rec['q']} (sites {lid},{lid + 1}, going {'left' if rec['going_left'] else 'right'}), dimensions "
            f"{W[lid].shape[0]} | {W[lid].shape[2]} | {W[lid + 1].shape[2]}, oracle keeps {rec['tr']['chi']} of {rec['full_rank']}")


def _engine(case, ds, W, hint=None):
    eng = mt.SweepEngine(0)
    if hint:
        eng.set_batch_hint(hint)
    if case.typed:
        dt = DT[case.dtype]
        o = sweep_options(case)
        eng.set_options(chi_max=o.chi_max, eta=o.eta, cutoff=o.cutoff)
        eng.set_dataset(0, ds.phi.astype(dt), ds.label_index, case.C)
        eng.set_mps([t.astype(dt) for t in W])
    else:
        load_engine(eng, ds, W, sweep_options(case))
    eng.build_caches()
    return eng


def _check_flags(case, info):
    for k, v in case.flags.items():
        assert info[k] == v, (case.id, k, info)


def _dev(worst, key, value):
    worst[key] = max(worst[key], float(value))


# ---- Float64: every chain, bond by bond ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", F64_CASES, ids=[c.id for c in F64_CASES])
def test_cutoff_limited_bonds_against_the_oracle(case):
    """Two teacher-forced sweeps of a Float64 case on the route its id names; kept dimension exact, no flip allowance.  Then the
    consumers of the ragged model the oracle ends with: eval and classify against summary.jl's restatement."""
    ds, recs, W_end = oracle_run(case)
    worst = dict(loss=0.0, grad=0.0, S=0.0, overlap=0.0)
    with _env(**case.env):
        eng = _engine(case, ds, recs[0]["W"])
        try:
            _check_flags(case, eng.info())
            for rec in recs:
                eng.set_mps(rec["W"])
                eng.build_caches()
                got, ref = eng.bond_step(rec["lid"], rec["going_left"]), rec["tr"]
                assert got["chi"] == ref["chi"], (_where(case, rec), "engine keeps", got["chi"], "margin", rec["margin"])
                n = ref["chi"]
                _dev(worst, "loss", abs(got["loss"] - ref["loss"]) / max(1.0, abs(ref["loss"])))
                _dev(worst, "grad", abs(got["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"])
                _dev(worst, "S", np.abs(got["S"][:n] - ref["S"]).max() / ref["S"][0])
                yg = R.contract_mps(eng.get_mps(), ds.phi)
                _dev(worst, "overlap", np.abs(yg - rec["y"]).max() / np.abs(rec["y"]).max())
                for k in F64:
                    assert worst[k] <= F64[k], (_where(case, rec), k, worst)
            info = eng.info()
            _check_flags(case, info)
            print(f"{case.id}: worst deviations {worst}, smallest margin {min(r['margin'] for r in recs):.2e}, subspace attempted / accepted "
                  f"{info['subspace_attempted']} / {info['subspace_accepted']}, final profile {[t.shape[2] for t in W_end[:-1]]}")
            # the ragged model's consumers
            eng.set_mps(W_end)
            eng.build_caches()
            mse, kld, acc, conf = eng.eval(0)
            mo, ko, ao, co = R.mse_loss_acc(W_end, ds, conf=True)
            assert abs(mse - mo) <= 1e-9 * max(1.0, abs(mo)) and abs(kld - ko) <= 1e-9 * max(1.0, abs(ko)), (mse, mo, kld, ko)
            assert acc == ao and np.array_equal(conf, co)
            pred, yh = eng.classify(0, return_overlaps=True)
            yo = R.contract_mps(W_end, ds.phi)
            assert np.abs(yh - yo).max() <= 1e-9 * np.abs(yo).max()
            assert np.array_equal(pred, R.classify(W_end, ds.phi))
        finally:
            eng.close()


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c.id for c in PAIR_CASES])
def test_second_bond_of_a_pair_consumes_the_tail_launch_overlaps(case):
    """The four-launch chain hands k_bond_tail's overlaps from one bond to the next.  From the oracle's state: TWO consecutive bonds of
    the same half-sweep with no set_mps between (the grouping of test_gpu_chain4.py's four-against-six test), the oracle advanced by
    the same two; the SECOND bond's loss, ||grad||, spectrum and kept dimension against the oracle's second bond - its yhat came from the
    first bond's tail launch, across a bond whose dimension had just changed."""
    ds, recs, _ = oracle_run(case)
    T, nb = case.T, case.T - 1
    worst = dict(loss=0.0, grad=0.0, S=0.0)
    npairs = 0
    with _env(**case.env):
        eng = _engine(case, ds, recs[0]["W"])
        try:
            _check_flags(case, eng.info())
            for sweep in range(NSWEEPS):
                q = 0
                while q + 1 < 2 * nb:
                    if (q < nb) != (q + 1 < nb):         # the turn: the next bond belongs to the other half-sweep
                        q += 1
                        continue
                    first, second = recs[sweep * 2 * nb + q], recs[sweep * 2 * nb + q + 1]
                    eng.set_mps(first["W"])
                    eng.build_caches()
                    a = eng.bond_step(first["lid"], first["going_left"])
                    assert a["chi"] == first["tr"]["chi"], _where(case, first)
                    got, ref = eng.bond_step(second["lid"], second["going_left"]), second["tr"]
                    assert got["chi"] == ref["chi"], (_where(case, second), "engine keeps", got["chi"])
                    n = ref["chi"]
                    _dev(worst, "loss", abs(got["loss"] - ref["loss"]) / max(1.0, abs(ref["loss"])))
                    _dev(worst, "grad", abs(got["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"])
                    _dev(worst, "S", np.abs(got["S"][:n] - ref["S"]).max() / ref["S"][0])
                    for k in PAIR:
                        assert worst[k] <= PAIR[k], (_where(case, second), k, worst)
                    npairs += 1
                    q += 2
            _check_flags(case, eng.info())
        finally:
            eng.close()
    print(f"{case.id}: {npairs} pairs, worst deviations of the second bond {worst}")
    assert npairs == NSWEEPS * 2 * (nb // 2)


# ---- element types ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TYPED_CASES, ids=[c.id for c in TYPED_CASES])
def test_cutoff_limited_bonds_in_every_element_type(case):
    """Two teacher-forced sweeps through the element-typed kernels (d chi_max = 160: the blocked solver, whose pair rule - one
    eigenvalue pair of the complex embedding per state - has a spectrum to cut here).  complex128 / float64: kept dimension exact.
    complex64 / float32: a flip by one state where the margin lies below Delta (module docstring), on at most a quarter of the bonds."""
    ds, recs, _ = oracle_run(case)
    dt = DT[case.dtype]
    f32 = case.dtype in ("float32", "complex64")
    tol = TOL["f32" if f32 else "f64"]
    worst = dict(loss=0.0, grad=0.0, S=0.0, bond=0.0)
    excused = 0
    with _env(**case.env):
        eng = _engine(case, ds, recs[0]["W"])
        try:
            _check_flags(case, eng.info())
            for rec in recs:
                lid, gl = rec["lid"], rec["going_left"]
                eng.set_mps([t.astype(dt) for t in rec["W"]], label_site=lid + 1 if gl else lid)
                eng.build_caches()
                got, ref = eng.bond_step(lid, gl), rec["tr"]
                nk = min(got["chi"], ref["chi"])
                _dev(worst, "loss", abs(got["loss"] - ref["loss"]) / max(1.0, abs(ref["loss"])))
                _dev(worst, "grad", abs(got["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"])
                _dev(worst, "S", np.abs(got["S"][:nk] - ref["S"][:nk]).max() / ref["S"][0])
                if got["chi"] != ref["chi"]:
                    assert f32, (_where(case, rec), "engine keeps", got["chi"], "margin", rec["margin"])
                    assert abs(got["chi"] - ref["chi"]) == 1 and excusable(rec, case.cutoff), (_where(case, rec), "engine keeps", got["chi"],
                                                                                                "margin", rec["margin"])
                    excused += 1
                else:
                    Wg = eng.get_mps()
                    a = two_site(Wg[lid], Wg[lid + 1])
                    _dev(worst, "bond", np.abs(a - rec["bond"]).max() / np.abs(rec["bond"]).max())
                for k in tol:
                    assert worst[k] < tol[k], (_where(case, rec), k, worst)
            info = eng.info()
            _check_flags(case, info)
        finally:
            eng.close()
    print(f"{case.id}: worst deviations {worst}, excused flips {excused} of {len(recs)} bonds, smallest margin {min(r['margin'] for r in recs):.2e}, "
          f"subspace attempted / accepted {info['subspace_attempted']} / {info['subspace_accepted']}")
    assert 4 * excused <= len(recs), (case.id, excused)


# ---- free running and batched -------------------------------------------------------------------------------------------------------------

def test_free_running_graph_sweeps_keep_the_profile_of_the_oracle():
    """Two eng.sweep() calls (graph replay, bond k + 1's tensor formed inside bond k's last launch) against the same bonds taken one by
    one with bond_step on a second engine: identical bits.  get_chi() after each sweep is the oracle's free-running profile, and the
    KLD agrees with the oracle's to 1e-9 (test_gpu_chain4.py's free-running bound)."""
    case = FREE_CASE
    ds, recs, W_end = oracle_run(case)           # the oracle's trajectory IS free running: every record starts where the last one ended
    T, nb2 = case.T, 2 * (case.T - 1)
    W0 = recs[0]["W"]
    a, b = _engine(case, ds, W0), _engine(case, ds, W0)
    try:
        _check_flags(case, a.info())
        for sweep in range(NSWEEPS):
            a.sweep()
            for q in range(nb2):
                b.bond_step(*bond_of(q, T))
            Wa, Wb = a.get_mps(), b.get_mps()
            assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(Wa, Wb)), sweep
            W_after = recs[(sweep + 1) * nb2]["W"] if sweep + 1 < NSWEEPS else W_end
            want = [1] + [t.shape[2] for t in W_after]
            assert a.get_chi()[0].tolist() == want, (sweep, a.get_chi()[0].tolist(), want)
        assert a.info()["graph"] and a.info()["tail_redos"] == 0
        _, kld, _, _ = a.eval(0)
        _, ko, _ = R.mse_loss_acc(W_end, ds)
        yo, yg = R.contract_mps(W_end, ds.phi), R.contract_mps(a.get_mps(), ds.phi)
        print(f"{case.id} free running: KLD {kld:.12f} (oracle {ko:.12f}), overlaps differ by {np.abs(yo - yg).max() / np.abs(yo).max():.2e}")
        assert abs(kld - ko) < 1e-9 * max(1.0, abs(ko)), (kld, ko)
    finally:
        a.close()
        b.close()


BATCH_SHAPE = (200, 10, 4, 32, 2)
BATCH_CUTOFFS = [1e-3] * 7 + [1e-10] * 3


def test_batched_sweeps_of_cutoff_limited_fits_are_bit_identical():
    """Ten fits of one shape (seven at cutoff 1e-3, three at 1e-10; different data and starting MPS) advanced by mpst_sweep_batch (the
    _b / _bm kernels) give the bits of ten solo sweeps, three sweeps long, through profiles that are no multiples of 4: with the
    six-launch chain's oracle comparison above, the batched kernels are covered in this regime too."""
    N, T, d, chi, C = BATCH_SHAPE
    K = len(BATCH_CUTOFFS)
    probs = [make_problem(N, T, d, 4, C, seed=200 + k, balanced=False) for k in range(K)]

    def fresh(k):
        e = mt.SweepEngine(0)
        e.set_batch_hint(K)
        e.set_options(chi_max=chi, eta=0.05, cutoff=BATCH_CUTOFFS[k])
        e.set_dataset(0, probs[k][0].phi, probs[k][0].label_index, C)
        e.set_mps(probs[k][1])
        e.build_caches()
        return e

    solo, bat = [fresh(k) for k in range(K)], [fresh(k) for k in range(K)]
    try:
        dims = set()
        for sweep in range(3):
            for e in solo:
                e.sweep()
            st = mt.sweep_batch(bat)
            assert len(st) == K and all(s["eig_fallbacks"] == 0 for s in st)
            for k, (x, y) in enumerate(zip(solo, bat)):
                assert np.array_equal(x.get_chi()[0], y.get_chi()[0]), (sweep, k)
                assert all(np.array_equal(ta, tb) for ta, tb in zip(x.get_mps(), y.get_mps())), (sweep, k)
                assert x.eval(0)[:3] == y.eval(0)[:3]
                dims |= set(y.get_chi()[0].tolist())
        info = bat[0].info()
        assert info["fused"] and not info["four_launch_chain"], info
        print(f"batched: bond dimensions seen {sorted(dims)}")
        assert any(n % 4 for n in dims if n > 1), dims
    finally:
        for e in solo + bat:
            e.close()


# ---- consumers of a ragged model ----------------------------------------------------------------------------------------------------------

def test_imputation_marginals_and_entanglement_on_a_ragged_model():
    """The model the oracle ends with on (531, 12, 4, 32, 2) - profile 4,12,32,...,32,25,8 instead of random_mps's constant bulk - through
    mpst_impute_model_run (median and mode, both orders; oracle/impute_numpy.py), mpst_marginal_model (tests/marginal_ref.py) and
    mpst_entanglement (tests/analysis_ref.py), each against the restatement and at the tolerance its own tests use."""
    from oracle import impute_numpy as IN
    from tests import marginal_ref as MR
    from tests.test_gpu_analysis import _check_spectra, _model
    from tests.test_gpu_impute_model import _check
    from tests.test_gpu_marginal import F64_TOL
    case = F64_CASES[0]
    ds, _, W = oracle_run(case)
    profile = [t.shape[2] for t in W[:-1]]
    assert len(set(profile)) >= 4 and any(n % 4 for n in profile), profile
    rng = np.random.default_rng(17)
    rows = np.sort(rng.choice(case.N, 14, replace=False))
    phi, y = ds.phi[rows], np.asarray(ds.label_index[rows], dtype=np.int32)
    m = (rng.uniform(size=(len(rows), case.T)) < 0.4).astype(np.uint8)
    m[0], m[1] = 1, 0
    ngrid = 401
    xs = -1.0 + (2.0 / (ngrid - 1)) * np.arange(ngrid)
    grid_phi = R.legendre_encode(xs, case.d)
    eng = mt.SweepEngine(0)
    try:
        classes = IN.expand_label_index(W)
        for o, order in enumerate(("forwards", "backwards")):
            x_med, e_med, _ = eng.impute_model(W, phi, y, m, xs, grid_phi, 0, True, order=o)
            x_mode, _, _ = eng.impute_model(W, phi, y, m, xs, grid_phi, 1, False, order=o)
            _check(W, xs, grid_phi, phi, y, m, x_med, e_med, "median", order, classes=classes)
            _check(W, xs, grid_phi, phi, y, m, x_mode, None, "mode", order, classes=classes)
        mask = m.astype(bool)
        got, _ = eng.marginal_model(W, phi, mask)
        ref = MR.log_marginals_ref(W, phi, mask)
        assert np.all(np.isfinite(ref)) and np.abs(got - ref).max() <= F64_TOL, np.abs(got - ref).max()
        _check_spectra(_model(W), eng)
    finally:
        eng.close()
