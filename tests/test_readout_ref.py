"""The long-double read-out reference (tests/readout_ref.py) against the float64 oracle (oracle/ref_numpy.py: contract_mps,
mse_loss_acc, classify) on small chains with the label on the first, a middle and the last site, real and complex - the condition
that makes the device bounds of tests/test_gpu_readout.py (1e-11 of the largest overlap and looser) meaningful."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import readout_ref as RR
from tests.marginal_ref import random_states

CHAINS = [([1, 3, 2, 1], 3, 2, 31), ([1, 2, 5, 7, 3, 1], 3, 3, 45), ([1, 4, 9, 16, 6, 2, 1], 4, 2, 23)]     # dims, d, C, N


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("chain", CHAINS, ids=["T3", "T5", "T6"])
def test_long_double_against_the_float64_oracle(chain, where, cx):
    """Measured: 4e-16 ... 1.1e-15 of the largest overlap; held to 1e-13.  The losses of a series are held to that bound carried
    through their derivatives: |d kld| = 2 |dy| / |y_label|, |d mse| <= sum_c |y_c - e_c| |dy|."""
    dims, d, C, N = chain
    T = len(dims) - 1
    p = {"first": 0, "middle": T // 2, "last": T - 1}[where]
    rng = np.random.default_rng(100 * T + 10 * p + cx)
    W = RR.ragged_chain(dims, d, C, p, cx, rng)
    phi = random_states(N, T, d, cx, rng)
    labels = np.sort(np.arange(N) % C)
    ref = RR.readout_ref(W, phi, labels)
    assert ref["y"].dtype == (np.clongdouble if cx else np.longdouble)
    y64 = R.contract_mps(W, phi)
    ymax = float(np.abs(ref["y"]).max())
    delta = 1e-13 * ymax
    err = float(np.abs(y64 - ref["y"]).max())
    print(f"T = {T}, label on {p}, {'complex' if cx else 'real'}: overlaps {err / ymax:.2e} of the largest, which is {ymax:.3f}")
    assert 0.01 < ymax < 10.0                     # the scaling of ragged_chain: overlaps of order 0.1
    assert err <= delta
    ds = R.EncodedSet(phi, labels, np.bincount(labels, minlength=C))
    mse, kld, acc, conf = R.mse_loss_acc(W, ds, conf=True)
    rows = np.arange(N)
    onehot = np.zeros((N, C))
    onehot[rows, labels] = 1.0
    mse_bound = float(np.mean(np.sum(np.abs(y64 - onehot), axis=1))) * delta + 1e-15 * abs(mse)
    kld_bound = float(np.mean(2.0 / np.abs(y64[rows, labels]))) * delta + 1e-15 * abs(kld)
    assert abs(mse - float(ref["mse_mean"])) <= mse_bound and abs(kld - float(ref["kld_mean"])) <= kld_bound
    assert float(ref["gap"].min()) > 1e-10        # no prediction hangs on the float64 oracle's rounding
    assert acc == ref["acc"] and np.array_equal(conf, ref["conf"])
    assert np.array_equal(R.classify(W, phi), ref["pred"])
    assert ref["conf"].sum() == N and np.array_equal(ref["conf"].sum(axis=1), np.bincount(labels, minlength=C))


def test_one_class_has_gap_one():
    rng = np.random.default_rng(5)
    W = RR.ragged_chain([1, 3, 3, 1], 2, 1, 1, False, rng)
    ref = RR.readout_ref(W, random_states(7, 3, 2, False, rng), np.zeros(7, dtype=np.int64))
    assert np.array_equal(ref["gap"], np.ones(7)) and ref["acc"] == 1.0 and ref["conf"].tolist() == [[7]]


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_power_of_two_scale_is_exact(cx):
    """The same seed with and without ``scale``: every overlap changes by exactly the product of the factors, in float64 as in long
    double; the predictions and the gaps do not change at all."""
    dims, d, C, p = [1, 2, 4, 4, 2, 1], 3, 2, 2
    scale = [4.0, 0.25, 0.5, 8.0, 0.125]
    W0 = RR.ragged_chain(dims, d, C, p, cx, np.random.default_rng(9))
    W1 = RR.ragged_chain(dims, d, C, p, cx, np.random.default_rng(9), scale=scale)
    phi = random_states(19, 5, d, cx, np.random.default_rng(10))
    f = float(np.prod(scale))
    assert np.array_equal(R.contract_mps(W1, phi), R.contract_mps(W0, phi) * f)
    labels = np.sort(np.arange(19) % C)
    a, b = RR.readout_ref(W0, phi, labels), RR.readout_ref(W1, phi, labels)
    assert np.array_equal(b["y"], a["y"] * f) and np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["gap"], b["gap"])
    with pytest.raises(AssertionError, match="powers of two"):
        RR.ragged_chain(dims, d, C, p, cx, np.random.default_rng(9), scale=[3.0] * 5)
