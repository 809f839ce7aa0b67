"""Host side of the multi-trajectory imputation (impute_ITS(...; num_trajectories), src/Imputation/MPS_methods.jl:304-347): the NumPy
restatement of the device generator (tests/philox_ref.py) against the published known-answer vectors of Philox4x32-10, the 53-bit
mapping, argument validation of the Python surface and the layout of the host-drawn uniform numbers.  No GPU."""
import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import imputation as IM
from tests import philox_ref as P


def _hex(words):
    return [f"{int(w):08x}" for w in words]


def test_philox4x32_10_known_answers():
    """The known-answer vectors of the Random123 distribution (kat_vectors, "philox4x32 10"): all-zero and all-ones counter and key,
    and the digits of pi."""
    assert _hex(P.philox4x32_10([0, 0, 0, 0], [0, 0])) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _hex(P.philox4x32_10([f, f, f, f], [f, f])) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _hex(P.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_philox_is_vectorised_over_counters():
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 2, 3, 4]], dtype=np.uint64)
    out = P.philox4x32_10(ctr, [5, 6])
    for r in range(3):
        assert np.array_equal(out[r], P.philox4x32_10(ctr[r], [5, 6]))


def test_uniform_mapping_is_53_bits_in_the_unit_interval():
    u = P.uniforms(seed=12345, row_id=[0, 7, 2 ** 40 + 3], K=3, T=5, trials=2)
    assert u.shape == (3, 3, 5, 2) and u.dtype == np.float64
    assert np.all(u >= 0.0) and np.all(u < 1.0)
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))             # multiples of 2^-53: every value exact
    assert len(np.unique(u)) == u.size
    # one draw by hand: counter (row low, row high, trajectory, site | trial << 20), key (seed low, seed high)
    row, k, j, t, seed = 2 ** 40 + 3, 2, 4, 1, 12345
    w = P.philox4x32_10([row & 0xFFFFFFFF, row >> 32, k, j | (t << 20)], [seed & 0xFFFFFFFF, seed >> 32])
    assert u[2, k, j, t] == ((int(w[0]) >> 5) * 2 ** 26 + (int(w[1]) >> 6)) / 2.0 ** 53
    # keyed by the row id, not by the position; another seed is another stream
    assert np.array_equal(P.uniforms(12345, [7], 3, 5, 2)[0], u[1])
    assert not np.any(P.uniforms(12346, [0, 7, 2 ** 40 + 3], 3, 5, 2) == u)
    # the upper word of a 64-bit seed is part of the key
    assert not np.any(P.uniforms(12345 + 2 ** 32, [0], 3, 5, 2) == u[:1])


def test_uniforms_look_uniform():
    u = P.uniforms(1, np.arange(50), 8, 25, 1).ravel()
    assert abs(u.mean() - 0.5) < 0.01 and abs(u.var() - 1.0 / 12.0) < 0.005
    ecdf = np.arange(1, u.size + 1) / u.size
    assert np.abs(np.sort(u) - ecdf).max() < np.sqrt(np.log(2 / 0.001) / (2 * u.size)) + 1.0 / u.size         # 99.9 % DKW


def test_host_drawn_uniforms_layout():
    """(N, K, T, trials): chain (i, k) reads the block u[i, k] as a single-trajectory call reads u[i]; K None keeps today's (N, T,
    trials) and today's stream."""
    a = IM._draw_uniforms(np.random.default_rng(3), 4, 6, 2, K=5)
    assert a.shape == (4, 5, 6, 2) and a.flags["C_CONTIGUOUS"] and a.dtype == np.float64
    assert np.array_equal(a, np.random.default_rng(3).uniform(0.0, 1.0, (4, 5, 6, 2)))
    b = IM._draw_uniforms(np.random.default_rng(3), 4, 6, 2)
    assert b.shape == (4, 6, 2) and np.array_equal(b, np.random.default_rng(3).uniform(0.0, 1.0, (4, 6, 2)))
    assert np.all(a >= 0.0) and np.all(a < 1.0)


class _NoEngine:
    """Stands where the engine would: validation has to fail before it is touched."""

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached")


def _dummy_problem():
    X = np.zeros((3, 6))
    return IM.ImputationProblem([], X, np.zeros(3), X, np.zeros(3), None, None, {0.0: 0})


@pytest.mark.parametrize("method", ["median", "mode", "mean"])
def test_trajectories_need_the_sampling_method(method):
    with pytest.raises(ValueError, match="num_trajectories"):
        mt.impute_dataset(_dummy_problem(), np.ones((3, 6), dtype=bool), method, num_trajectories=4, engine=_NoEngine())


@pytest.mark.parametrize("K", [0, -3])
def test_fewer_than_one_trajectory_is_refused(K):
    with pytest.raises(ValueError, match="at least 1"):
        mt.impute_dataset(_dummy_problem(), np.ones((3, 6), dtype=bool), "ITS", num_trajectories=K, engine=_NoEngine())


def test_rseed_without_trajectories_is_refused():
    with pytest.raises(ValueError, match="rseed"):
        mt.impute_dataset(_dummy_problem(), np.ones((3, 6), dtype=bool), "ITS", rseed=1, engine=_NoEngine())


def test_engine_argument_checks():
    T = mt.SweepEngine._traj_args
    with pytest.raises(ValueError, match="at least 1"):
        T(2, 3, 2, 1, None, 0, 1, None)
    with pytest.raises(ValueError, match="sampling"):
        T(2, 3, 0, 1, None, 4, 1, None)
    with pytest.raises(ValueError, match="seed"):
        T(2, 3, 2, 1, None, 4, None, None)
    with pytest.raises(AssertionError):
        T(2, 3, 4, 5, np.zeros((2, 4, 3)), 4, None, None)                    # u must be (N, K, T, max_trials)
    K, u, seed, rid = T(2, 3, 4, 5, np.zeros((2, 4, 3, 5)), 4, None, [10, 11])
    assert K == 4 and u.shape == (2, 4, 3, 5) and seed == 0 and rid.dtype == np.int64
    assert T(2, 3, 2, 1, None, 1, 2 ** 64 - 1, None)[2] == -1                  # the 64 bits of the seed cross the ABI as an int64


def test_new_symbols_are_bound():
    for name in ("mpst_impute_traj", "mpst_impute_model_traj"):
        assert name in mt._lib.SYMBOLS and len(mt._lib.SYMBOLS[name][1]) == 14
        assert hasattr(mt._lib.load(), name)
