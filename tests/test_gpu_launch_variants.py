"""Every row of the two lists of headline-kernel instantiations (csrc/mpst_bond_plan.h: YHAT_S_LIST, GRAD_S_LIST), each at the smallest
shape that reaches it, through the three host paths that launch it: mpst_sweep (a replayed graph), mpst_sweep_batch (the batched
launchers) and mpst_bond_step (plain stream) - identical bits - and one sweep against the NumPy oracle.  C = 2, KLD / TSGO,
eta 0.05, cutoff 1e-10.  Rows reached (k_yhat_s <LM, D4, V2> / k_grad_s <AW2, D2, FS, KC, NW>; the batched fits run 4 waves at d = 4,
the oracle comparison runs an engine without a batch hint: 8 waves, four launches per bond):
    d = 4,  capacity 12:  <2,true,true>    / <1,1,25,256,4> and <1,1,25,256,8>
    d = 4,  capacity 11:  <2,true,false>   (an odd capacity: no 16-byte row loads)
    d = 3,  capacity 10:  <2,false,false>  / <2,1,0,256,8>
    d = 5,  capacity 6:                      <1,1,0,256,8>
    d = 11, capacity 4:                      <1,2,0,256,8>      (chi_max 3; the starting MPS has bonds of 4)
    d = 2,  capacity 40:  <4,false,false>
Of the 8-wave d = 4 row <1,1,25,256,8> only the solo kernel runs (the oracle case's engine): a context that is advanced in batches has
a batch hint and with it 4 waves at d = 4, so no case launches k_grad_s_b of that row.
Every case prints the SHA-256 of its final MPS: a change of the host path that is meant to move nothing is checked by comparing
these between two builds."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

import mpstime_jl_amd as mt
from oracle import ref_numpy as R
from tests.helpers import bond_of, load_engine, make_problem

pytestmark = pytest.mark.gpu

C = 2
SHAPES = [(96, 5, 4, 12), (96, 5, 4, 11), (96, 5, 3, 10), (96, 5, 5, 6), (64, 5, 11, 3), (96, 5, 2, 40)]


def _engine(ds, W, chi, hint=None):
    eng = mt.SweepEngine(0)
    if hint:
        eng.set_batch_hint(hint)      # the gradient's shares and waves belong to the context: solo and batched sweeps agree bit for bit
    load_engine(eng, ds, W, R.SweepOptions(nsweeps=1, chi_max=chi, eta=0.05, cutoff=1e-10))
    eng.build_caches()
    return eng


@contextlib.contextmanager
def _env(**kv):
    """Environment variables for the engines created inside (the library reads them when a context resolves its launch chain)."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _state(eng):
    return eng.get_mps(), eng.get_chi()


def _same(a, b):
    (Wa, (chia, lsa)), (Wb, (chib, lsb)) = a, b
    return np.array_equal(chia, chib) and lsa == lsb and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(Wa, Wb))


def _digest(W):
    h = hashlib.sha256()
    for t in W:
        h.update(np.ascontiguousarray(t).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("N,T,d,chi", SHAPES)
def test_sweep_batch_and_bond_steps_give_the_same_bits(N, T, d, chi):
    probs = [make_problem(N, T, d, 4, C, seed=seed) for seed in (7, 8)]          # the second fit of the batch: another seed
    solo = [_engine(ds, W, chi, hint=2) for ds, W in probs]
    bat = [_engine(ds, W, chi, hint=2) for ds, W in probs]
    step = _engine(*probs[0], chi, hint=2)
    try:
        info = solo[0].info()
        assert info["fused"] and info["sliced_bond_gemms"] and not info["four_launch_chain"], info
        assert info["cap"] == max(chi, 4)
        for sweep in range(2):
            for e in solo:
                e.sweep()
            st = mt.sweep_batch(bat)
            assert all(s["eig_fallbacks"] == 0 for s in st)
            for q in range(2 * (T - 1)):
                step.bond_step(*bond_of(q, T))
            a = _state(solo[0])
            for k in (0, 1):
                assert _same(_state(solo[k]), _state(bat[k])), (sweep, k, "sweep against sweep_batch")
            assert _same(a, _state(step)), (sweep, "sweep against bond steps")
        print(f"final MPS (N={N}, T={T}, d={d}, chi_max={chi}): chi {a[1][0].tolist()}, sha256 {_digest(a[0])}")
    finally:
        for e in solo + bat + [step]:
            e.close()


@pytest.mark.parametrize("N,T,d,chi", SHAPES)
def test_one_sweep_agrees_with_the_oracle(N, T, d, chi):
    """The bounds of test_free_running_sweeps_of_both_chains_agree_with_the_oracle: KLD to 1e-9 (relative), overlaps to 1e-8 of the
    largest; the engine has no batch hint: the four-launch chain up to a capacity of 32."""
    ds, W0 = make_problem(N, T, d, 4, C, seed=7)
    Wo = [t.copy() for t in W0]
    R.sweep(Wo, ds, R.SweepOptions(nsweeps=1, chi_max=chi, eta=0.05, cutoff=1e-10))
    _, ko, _ = R.mse_loss_acc(Wo, ds)
    yo = R.contract_mps(Wo, ds.phi)
    eng = _engine(ds, W0, chi)
    try:
        assert eng.info()["four_launch_chain"] == (chi <= 32)          # the tail holds at most 32 kept vectors: six launches beyond
        st = eng.sweep()
        _, kld, _, _ = eng.eval(0)
        W = eng.get_mps()
    finally:
        eng.close()
    dev = np.abs(yo - R.contract_mps(W, ds.phi)).max() / np.abs(yo).max()
    print(f"(N={N}, T={T}, d={d}, chi_max={chi}): KLD {kld:.15g} oracle {ko:.15g} (relative {abs(kld - ko) / max(1.0, abs(ko)):.3e}), "
          f"overlaps differ by {dev:.3e} of the largest, eig_fallbacks {st['eig_fallbacks']}, sha256 {_digest(W)}")
    assert abs(kld - ko) < 1e-9 * max(1.0, abs(ko)), (kld, ko)
    assert dev < 1e-8, dev


def test_persistent_pair_sweep_equals_bond_steps():
    """MPST_B2=0: the persistent pair k_bond_fused + k_fused_reduce in place of the sliced one (which the context otherwise picks
    below about 8000 series), at (96, 5, 4, 8): one sweep against its bond steps, identical bits."""
    N, T, d, chi = 96, 5, 4, 8
    ds, W = make_problem(N, T, d, 4, C, seed=7)
    with _env(MPST_B2=0):
        engs = [_engine(ds, W, chi) for _ in range(2)]
        infos = [e.info() for e in engs]            # resolves the chain while the environment is set
    try:
        assert all(i["fused"] and not i["sliced_bond_gemms"] for i in infos), infos
        engs[0].sweep()
        for q in range(2 * (T - 1)):
            engs[1].bond_step(*bond_of(q, T))
        a, b = _state(engs[0]), _state(engs[1])
        print(f"final MPS (MPST_B2=0, N={N}, T={T}, d={d}, chi_max={chi}): chi {a[1][0].tolist()}, sha256 {_digest(a[0])}")
        assert _same(a, b)
    finally:
        for e in engs:
            e.close()
