"""The cache rebuilds of a sweep (rebuild_caches: the reference's two construct_caches calls) beside the eigensolver: the side workgroups
of every bond's k_eig_trivec launch rebuild one environment row of a site that is already final, and a walk of two steps closes each
half-sweep (default), against the two full walks (MPST_REBUILD_SIDE=0) and against no rebuild at all.  A rebuilt row is the row that is
there already, bit for bit, so the three must agree in every bit - and the device's own count of the rows rebuilt beside the eigensolver,
2 max(0, T - 3) per sweep, is what shows that the path ran."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests.helpers import _env, bond_of, make_problem

pytestmark = pytest.mark.gpu

# (N, T, d, chi, C): tiles with fewer than 16 series, 3 hidden steps per half; extents that are no multiples of 4; kr_at's clamp and
# bonds of 3; 17 tiles, full 32-wide bonds, the single hidden step is the chain end (prev = 1); nothing hidden, the closing walk does
# everything (T = 3, T = 2); bond dimensions still growing along the chain, 9 hidden steps per half
SHAPES = [(40, 6, 4, 8, 2), (33, 5, 3, 5, 2), (32, 5, 11, 3, 2), (272, 4, 4, 32, 2), (40, 3, 4, 8, 2), (40, 2, 4, 8, 2), (48, 12, 4, 6, 2)]


def _hidden(T):
    return 2 * max(0, T - 3)


def _fresh(ds, W, chi, eta=0.05, options=None, cutoff=1e-10, label_site=None, **env):
    with _env(**env):
        eng = mt.SweepEngine(0)
        eng.set_options(chi_max=chi, eta=eta, cutoff=cutoff, **(options or {}))
        eng.set_dataset(0, ds.phi, ds.label_index, len(ds.class_distribution))
        if label_site is None:
            eng.set_mps(W)
        else:
            eng.set_mps(W, label_site=label_site)
        eng.build_caches()
        eng.info()            # resolves the chain while the environment is set
    return eng


def _same_mps(Wa, Wb):
    assert len(Wa) == len(Wb)
    for j, (a, b) in enumerate(zip(Wa, Wb)):
        assert a.shape == b.shape and np.array_equal(a, b), j


_two_sweeps_old = {}


def _start(shape):
    """The problem and the state two free-running sweeps (no rebuilds) leave: computed once per shape."""
    if shape not in _two_sweeps_old:
        N, T, d, chi, C = shape
        ds, W = make_problem(N, T, d, 4, C, seed=7 + N)
        eng = _fresh(ds, W, chi)
        try:
            eng.sweep()
            eng.sweep()
            W1, (_, ls) = eng.get_mps(), eng.get_chi()
            assert eng.info()["tail_redos"] == 0
        finally:
            eng.close()
        _two_sweeps_old[shape] = (ds, W1, ls)
    return _two_sweeps_old[shape]


def _run(shape, rebuild, side):
    """Two sweeps from the two-sweeps-old state, then one half-sweep bond by bond.  side: None = default (hidden path), 0 = MPST_REBUILD_SIDE=0."""
    N, T, d, chi, C = shape
    ds, W1, ls = _start(shape)
    on = rebuild and side is None
    eng = _fresh(ds, W1, chi, options={"rebuild_caches": rebuild}, label_site=ls, MPST_REBUILD_SIDE=side)
    try:
        info = eng.info()
        assert info["four_launch_chain"] and info["tail_side_workgroups"], info
        assert info["rebuild_side"] == on, (rebuild, side, info)
        for _ in range(2):
            eng.sweep()
            info = eng.info()
            assert info["rebuild_side_steps"] == (_hidden(T) if on else 0), (rebuild, side, info)
            assert info["tail_redos"] == 0, info
        W2 = eng.get_mps()
        steps = [eng.bond_step(*bond_of(q, T)) for q in range(T - 1)]
        W3 = eng.get_mps()
        assert eng.info()["tail_redos"] == 0
    finally:
        eng.close()
    return W2, W3, steps


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rebuilds_beside_the_eigensolver_leave_the_bits_of_the_full_walks(shape):
    T = shape[1]
    hid = _run(shape, True, None)
    full = _run(shape, True, 0)
    none = _run(shape, False, None)
    for other in (full, none):
        _same_mps(hid[0], other[0])
        _same_mps(hid[1], other[1])
        assert len(hid[2]) == len(other[2]) == T - 1
        for q, (a, b) in enumerate(zip(hid[2], other[2])):
            assert a["chi"] == b["chi"], (q, a["chi"], b["chi"])
            assert a["loss"] == b["loss"], (q, a["loss"], b["loss"])
            assert a["grad_norm"] == b["grad_norm"], (q, a["grad_norm"], b["grad_norm"])
            assert a["S"].shape == b["S"].shape and np.array_equal(a["S"], b["S"]), q


@pytest.mark.parametrize("switch", ["MPST_REBUILD_SIDE", "MPST_TAIL_PRE", "MPST_CHAIN4"])
def test_the_switches_that_turn_the_hidden_rebuild_off(switch):
    """Each of the three keeps the full walks: the flag is off and no row is counted; without any of them the flag is on and every sweep
    counts 2 (T - 3) rows."""
    shape = (40, 6, 4, 8, 2)
    N, T, d, chi, C = shape
    ds, W1, ls = _start(shape)
    for val in (None, 0):
        eng = _fresh(ds, W1, chi, options={"rebuild_caches": True}, label_site=ls, **{switch: val})
        try:
            assert eng.info()["rebuild_side"] == (val is None), (switch, val, eng.info())
            eng.sweep()
            info = eng.info()
            assert info["rebuild_side_steps"] == (_hidden(T) if val is None else 0), (switch, val, info)
            assert info["tail_redos"] == 0
        finally:
            eng.close()


@pytest.mark.parametrize("n_fail", [2, 7])
def test_failed_tail_verification_is_recovered_with_hidden_rebuilds(n_fail):
    """MPST_TAIL_FORCE_REDO with rebuild_caches and the hidden path on: tail launch 2 of 10 (backward half-sweep) or 7 (forward half) reports
    a failed verification.  The side workgroups of the launches after it skip their step (the sites are not final), the rest of the sweep
    runs on the six-launch chain with the full walks: one redo, one fallback, the bond dimensions of an undisturbed sweep, overlaps to 1e-7
    of the largest (the bound of test_failed_tail_verification_is_recovered_with_side_workgroups), fewer than 2 (T - 3) rows counted."""
    N, T = 40, 6
    ds, W = make_problem(N, T, 4, 4, 2, seed=7 + N)
    ref = _fresh(ds, W, 8, options={"rebuild_caches": True})
    bad = _fresh(ds, W, 8, options={"rebuild_caches": True}, MPST_TAIL_FORCE_REDO=n_fail)
    try:
        assert ref.info()["rebuild_side"] and bad.info()["rebuild_side"]
        ref.sweep()
        st = bad.sweep()
        assert ref.info()["tail_redos"] == 0 and ref.info()["rebuild_side_steps"] == _hidden(T)
        assert bad.info()["tail_redos"] == 1, bad.info()
        assert st["eig_fallbacks"] == 1
        print(f"forced failure at tail launch {n_fail}: {bad.info()['rebuild_side_steps']} rows rebuilt beside the eigensolver")
        assert bad.info()["rebuild_side_steps"] < _hidden(T), bad.info()
        assert np.array_equal(ref.get_chi()[0], bad.get_chi()[0])
        ya, yb = R.contract_mps(ref.get_mps(), ds.phi), R.contract_mps(bad.get_mps(), ds.phi)
        dev = np.abs(ya - yb).max() / np.abs(ya).max()
        print(f"forced failure at tail launch {n_fail}: overlaps differ by {dev:.3e} of the largest")
        assert dev < 1e-7, (n_fail, dev)
    finally:
        bad.close()
        ref.close()


def test_closing_walks_start_mid_chain_with_the_bits_of_the_per_site_launches():
    """build_caches, then a sweep with the reference's rebuilds: the hidden steps and the two-step closing walks (k_env_walk started
    mid-chain, prev read from memory) against one k_env launch per site (MPST_ENV_WALK=0, which also keeps every rebuild out of the
    eigensolver's launch) - the comparison of test_env_walk_builds_the_caches_of_the_per_site_launches, through the closing walks."""
    N, T, d, chi, C = 48, 12, 4, 6, 2
    ds, W = make_problem(N, T, d, 4, C, seed=7 + N)
    res = {}
    for walk in (0, None):
        with _env(MPST_ENV_WALK=walk):
            eng = _fresh(ds, W, chi, options={"rebuild_caches": True})
            try:
                assert eng.info()["rebuild_side"] == (walk is None)
                eng.sweep()
                assert eng.info()["rebuild_side_steps"] == (_hidden(T) if walk is None else 0)
                res[walk] = (eng.get_mps(), eng.eval(0)[:3])
            finally:
                eng.close()
    _same_mps(res[0][0], res[None][0])
    assert res[0][1] == res[None][1]
