"""The operand schedule of the bond kernels: k_gram_upd requests its operands in half batches, every load unconditional from a clamped
address and the lane predicate on the value (gram_upd_body), and the back-split hosts of k_bond_tail drop what lies beyond their operand
when it is consumed (tail_split_request / tail_split_job).  None of it changes an arithmetic operation or its order, so: the shapes at
which k_gram_upd goes through later batches and half-masked ones against the NumPy oracle, the back-split hosts with partial tiles
against the six-launch chain, and the bits of whole sweeps against those of the build before the change (tests/golden)."""
import functools
import os

import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests.helpers import _env, bond_matrix, bond_of, load_engine, make_problem

pytestmark = pytest.mark.gpu

# (a directory of its own: test_oracle.py and test_gpu_golden.py take every tests/golden/*.npz for a sweep fixture of the oracle's format)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bond_roundtrips", "parent.npz")


T = 8


@functools.lru_cache(maxsize=None)
def _oracle_half_sweeps(N, d, chi, C):
    """The oracle's backward and forward half-sweep, once per shape: the state every bond starts from and what the oracle's update of it
    reports (shared by the two chains' cases, not modified by them)."""
    ds, W0 = make_problem(N, T, d, chi, C, seed=17 + N)
    opts = R.SweepOptions(nsweeps=1, chi_max=chi, eta=0.05)
    W = [t.copy() for t in W0]
    LE, RE = R.construct_caches(W, ds.phi, True)
    states, traces = [], []
    for q in range(2 * (T - 1)):
        lid, going_left = bond_of(q, T)
        if q == T - 1:
            LE, RE = R.construct_caches(W, ds.phi, False)
        states.append([t.copy() for t in W])
        tro = {}
        R.bond_step(W, LE, RE, lid, ds, opts, going_left, tro)
        traces.append(tro)
    return ds, W0, opts, states, traces


# T = 8, chi_max = 32, d = 4: the bond in the middle has X = Y = 128.  Going right the classes are batches of their own (C = 3, 5: three and
# five of them, a wave's 32 k a half batch each, the other half zero-operand steps); going left K = C X = 384, 640: a wave's 96 k are
# one batch and a half, its 160 k two and a half.  C = 2 with (d, chi) = (3, 11), (4, 20): X, Y = 33, 80 - no multiples of 16, dead lanes
# in both panels, clamped rows and columns.
@pytest.mark.parametrize("chain4", [None, 0])
@pytest.mark.parametrize("N,d,chi,C", [(96, 4, 32, 3), (160, 4, 32, 5), (64, 3, 11, 2), (64, 4, 20, 2)])
def test_later_batches_of_gram_upd_agree_with_the_oracle(N, d, chi, C, chain4):
    """Every bond_step of a backward and a forward half-sweep against the NumPy oracle's, each from the oracle's state (one update from a
    common state is well conditioned): loss to 1e-9, gradient norm and singular values to 1e-8 (the bounds of
    test_gpu_chain4.py::test_free_running_sweeps_of_both_chains_agree_with_the_oracle for the KLD and for the overlaps), the same kept
    dimension; on both launch chains."""
    ds, W0, opts, states, traces = _oracle_half_sweeps(N, d, chi, C)
    with _env(MPST_CHAIN4=chain4):
        eng = mt.SweepEngine(0)
        load_engine(eng, ds, W0, opts)
        eng.build_caches()
        assert eng.info()["four_launch_chain"] == (chain4 is None)
    try:
        worst = {"loss": 0.0, "grad": 0.0, "S": 0.0}
        for q, (W, tro) in enumerate(zip(states, traces)):
            eng.set_mps(W)
            eng.build_caches()
            tr = eng.bond_step(*bond_of(q, T))
            assert tr["chi"] == tro["chi"], (q, tr["chi"], tro["chi"])
            worst["loss"] = max(worst["loss"], abs(tr["loss"] - tro["loss"]) / max(1.0, abs(tro["loss"])))
            worst["grad"] = max(worst["grad"], abs(tr["grad_norm"] - tro["grad_norm"]) / tro["grad_norm"])
            worst["S"] = max(worst["S"], np.abs(tr["S"][:tr["chi"]] - tro["S"]).max() / tro["S"][0])
        print(f"N={N} d={d} chi={chi} C={C} chain4={chain4}: worst relative deviations {worst}")
        assert worst["loss"] < 1e-9 and worst["grad"] < 1e-8 and worst["S"] < 1e-8, worst
    finally:
        eng.close()


def _fresh(ds, W, chi, C, **env):
    with _env(**env):
        eng = mt.SweepEngine(0)
        eng.set_options(chi_max=chi, eta=0.05, cutoff=1e-10)
        eng.set_dataset(0, ds.phi, ds.label_index, C)
        eng.set_mps(W)
        eng.build_caches()
        eng.info()            # resolves the chain while the environment is set
    return eng


def test_back_split_hosts_with_partial_tiles_store_the_sites_of_the_six_launch_chain():
    """d = 3, chi = 11, C = 3: X, Y up to 33 - three tiles of 16 of which the last holds one row - and a host takes two tiles, so hosts
    have tiles of a class c >= C and tiles cut by the matrix.  Every bond of a sweep by both chains from the six-launch chain's state: the
    two site tensors each stores, compared as the two-site tensor they make (the eigenvectors' signs are the chain's own), and the overlaps
    with the data, to 1e-8 of the largest (test_gpu_chain4.py::_four_against_six)."""
    N, d, chi, C = 96, 3, 11, 3
    ds, W = make_problem(N, T, d, chi, C, seed=11 + N)
    e6 = _fresh(ds, W, chi, C, MPST_CHAIN4=0)
    e4 = _fresh(ds, W, chi, C, MPST_CHAIN4=None)
    try:
        assert not e6.info()["four_launch_chain"] and e4.info()["four_launch_chain"]
        worst = 0.0
        for q in range(2 * (T - 1)):
            lid, gl = bond_of(q, T)
            e4.set_mps(e6.get_mps())
            e4.build_caches()
            a = e6.bond_step(lid, gl)
            b = e4.bond_step(lid, gl)
            assert a["chi"] == b["chi"], (q, a["chi"], b["chi"])
            Wa, Wb = e6.get_mps(), e4.get_mps()
            ma, mb = bond_matrix(Wa[lid], Wa[lid + 1]), bond_matrix(Wb[lid], Wb[lid + 1])
            worst = max(worst, np.abs(ma - mb).max() / np.abs(ma).max())
            ya, yb = R.contract_mps(Wa, ds.phi), R.contract_mps(Wb, ds.phi)
            worst = max(worst, np.abs(ya - yb).max() / np.abs(ya).max())
        print(f"four launches against six, stored sites: worst relative deviation {worst:.3e}")
        assert worst < 1e-8, worst
        assert e4.info()["tail_redos"] == 0
    finally:
        e6.close()
        e4.close()


def _two_sweeps(N, T, d, chi, C):
    ds, W = make_problem(N, T, d, chi, C, seed=3 + N)
    eng = mt.SweepEngine(0)
    try:
        eng.set_options(chi_max=chi, eta=0.05, rebuild_caches=True)
        eng.set_dataset(0, ds.phi, ds.label_index, C)
        eng.set_mps(W)
        eng.build_caches()
        eng.sweep()
        eng.sweep()
        info = eng.info()
        assert info["graph"] and info["four_launch_chain"], info
        return eng.get_mps()
    finally:
        eng.close()


@pytest.mark.parametrize("N,T,d,chi,C", [(96, 8, 4, 32, 3), (64, 8, 3, 11, 2), (128, 10, 4, 32, 2)])
def test_two_sweeps_leave_the_bits_of_the_build_before_the_change(N, T, d, chi, C):
    """The site tensors after two sweeps (cache rebuilds on, replayed from the graph) equal, element for element, those the build of the
    commit before this change left on the same GPU model (tests/golden/bond_roundtrips/parent.npz; the commit and the compiler are in
    the file's meta_* entries)."""
    gold = np.load(GOLDEN)
    Wg = _two_sweeps(N, T, d, chi, C)
    for j, w in enumerate(Wg):
        ref = gold[f"N{N}_T{T}_d{d}_chi{chi}_C{C}/site_{j}"]
        assert w.shape == ref.shape, (j, w.shape, ref.shape)
        assert np.array_equal(w, ref), (j, float(np.abs(w - ref).max()))
