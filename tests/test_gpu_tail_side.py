"""The side workgroups of k_eig_trivec (four-launch chain): the part of k_bond_tail that needs no eigenvector - the dense S tile of
every 16-series tile and the next bond's overlap product P = O bt_new - is formed by extra workgroups of the eigensolver's launch and
read back by the tail (default), against the tail forming both itself (MPST_TAIL_PRE=0).  Every floating-point operation keeps its
operands and its order, so the two paths must agree bit for bit; the recovery path of a failed tail verification and the bonds that
do not chain into a next one (side workgroups that form the S tile only) are covered too."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests.helpers import _env, bond_of, make_problem

pytestmark = pytest.mark.gpu


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


def _check_path(eng, pre):
    info = eng.info()
    assert info["four_launch_chain"], info
    assert info["tail_side_workgroups"] == (pre is None), (pre, info)


def _same_mps(Wa, Wb):
    assert len(Wa) == len(Wb)
    for j, (a, b) in enumerate(zip(Wa, Wb)):
        assert a.shape == b.shape and np.array_equal(a, b), j


def _two_stages(ds, W, T, chi, pre):
    """Two free-running sweeps without cache rebuilds, two more with them (a fresh context on the state the first two left, created while
    the switch is set: a context reads it when its workspace is built), then one half-sweep bond by bond.  Returns what to compare."""
    eng = _fresh(ds, W, chi, MPST_TAIL_PRE=pre)
    try:
        _check_path(eng, pre)
        eng.sweep()
        eng.sweep()
        W1, (_, ls) = eng.get_mps(), eng.get_chi()
        assert eng.info()["tail_redos"] == 0
    finally:
        eng.close()
    eng = _fresh(ds, W1, chi, options={"rebuild_caches": True}, label_site=ls, MPST_TAIL_PRE=pre)
    try:
        _check_path(eng, pre)
        eng.sweep()
        eng.sweep()
        W2 = eng.get_mps()
        steps = [eng.bond_step(*bond_of(q, T)) for q in range(T - 1)]
        W3 = eng.get_mps()
        info = eng.info()
        assert info["four_launch_chain"] and info["tail_redos"] == 0, info
    finally:
        eng.close()
    return W1, W2, W3, steps


# tiles with fewer than 16 series, a tile boundary at the class boundary, chain ends with bond dimension 1;
# contraction extents that are no multiples of 4 and d * chi no multiple of 16 (zero padding of P's columns and of the S tile);
# kr_at's clamp (d >= 11 with a bond of 3: tests/test_gpu_chain4.py), now exercised in the side workgroup;
# 17 tiles with full 32-wide bonds
@pytest.mark.parametrize("N,T,d,chi,C", [(40, 6, 4, 8, 2), (33, 5, 3, 5, 2), (32, 5, 11, 3, 2), (272, 4, 4, 32, 2)])
def test_side_workgroups_leave_the_bits_of_the_in_tail_path(N, T, d, chi, C):
    ds, W = make_problem(N, T, d, 4, C, seed=7 + N)
    old = _two_stages(ds, W, T, chi, 0)
    new = _two_stages(ds, W, T, chi, None)
    for Wa, Wb in zip(old[:3], new[:3]):
        _same_mps(Wa, Wb)
    assert len(old[3]) == len(new[3]) == T - 1
    for q, (a, b) in enumerate(zip(old[3], new[3])):
        assert a["chi"] == b["chi"], (q, a["chi"], b["chi"])
        assert a["loss"] == b["loss"], (q, a["loss"], b["loss"])
        assert a["grad_norm"] == b["grad_norm"], (q, a["grad_norm"], b["grad_norm"])
        assert a["S"].shape == b["S"].shape and np.array_equal(a["S"], b["S"]), q


@pytest.mark.parametrize("n_fail", [2, 7])
def test_failed_tail_verification_is_recovered_with_side_workgroups(n_fail):
    """MPST_TAIL_FORCE_REDO (tests/test_gpu_chain4.py) with the side workgroups on: tail launch 2 of 10 (backward half-sweep) or 7
    (forward half) reports a failed verification; the sweep, finished on the six-launch chain, equals an undisturbed one as the recovery
    tests of the in-tail path demand - bond dimensions, one redo, one fallback, overlaps to 1e-7 of the largest, equal accuracy."""
    N, T = 40, 6
    ds, W = make_problem(N, T, 4, 4, 2, seed=7 + N)
    ref = _fresh(ds, W, 8)
    bad = _fresh(ds, W, 8, MPST_TAIL_FORCE_REDO=n_fail)
    try:
        _check_path(ref, None)
        _check_path(bad, None)
        ref.sweep()
        st = bad.sweep()
        assert ref.info()["tail_redos"] == 0
        assert bad.info()["tail_redos"] == 1, bad.info()
        assert st["eig_fallbacks"] == 1
        assert np.array_equal(ref.get_chi()[0], bad.get_chi()[0])
        ya, yb = R.contract_mps(ref.get_mps(), ds.phi), R.contract_mps(bad.get_mps(), ds.phi)
        dev = np.abs(ya - yb).max() / np.abs(ya).max()
        print(f"forced failure at tail launch {n_fail}: overlaps differ by {dev:.3e} of the largest")
        assert dev < 1e-7, (n_fail, dev)
        assert ref.eval(0)[2] == bad.eval(0)[2]
    finally:
        bad.close()
        ref.close()


def test_unchained_bonds_take_the_s_tile_alone_from_the_side_workgroups():
    """T = 4 with the reference's cache rebuilds: the bond before the mid-sweep rebuild and the last bond of the sweep chain into no next
    one (want_next = 0) - their side workgroups form the S tile only and the tail reads no overlap product.  Bit-identical to the in-tail path."""
    N, T, chi = 40, 4, 8
    ds, W = make_problem(N, T, 4, 4, 2, seed=3)
    res = {}
    for pre in (0, None):
        eng = _fresh(ds, W, chi, options={"rebuild_caches": True}, MPST_TAIL_PRE=pre)
        try:
            _check_path(eng, pre)
            eng.sweep()
            eng.sweep()
            res[pre] = (eng.get_mps(), eng.eval(0)[:3])
            assert eng.info()["tail_redos"] == 0
        finally:
            eng.close()
    _same_mps(res[0][0], res[None][0])
    assert res[0][1] == res[None][1]
