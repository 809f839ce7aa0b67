"""The NumPy restatement of the model overlaps (tests/overlap_ref.py) against itself: the walk against the dense states, and float64
against long double at every shape the device is tested at - the condition that makes the device tolerance of 1e-10 meaningful."""
import numpy as np
import pytest

from tests import overlap_ref as R
from tests.marginal_ref import gaussian_chain


def test_walk_against_the_dense_states():
    """T = 5, d = 4, complex, chi 6 / 9, C 3 / 2 (measured: 5.7e-16 relative)"""
    rng = np.random.default_rng(77)
    A, B = gaussian_chain(5, 4, 6, 3, 2, True, rng, scale=0.3), gaussian_chain(5, 4, 9, 2, 2, True, rng, scale=0.3)
    worst = 0.0
    for X, Y in ((A, A), (A, B), (B, A), (B, B)):
        g, lg = R.overlap_ref(X, Y)
        ref = R.overlap_brute(X, Y)
        assert g.shape == ref.shape
        worst = max(worst, float(np.abs(g * np.exp(lg) - ref).max() / np.abs(ref).max()))
    print(f"walk against dense states: {worst:.2e}")
    assert worst <= 1e-13
    g_ab, lg_ab = R.overlap_ref(A, B)
    g_ba, lg_ba = R.overlap_ref(B, A)
    assert np.abs(g_ba * np.exp(lg_ba) - (g_ab * np.exp(lg_ab)).conj().T).max() <= 1e-13 * np.abs(g_ab * np.exp(lg_ab)).max()


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_against_long_double(name, cx):
    """Largest deviations measured: 9.7e-13 of a normalised overlap (complex, T = 1000), 4.9e-13 of a ln norm; both held to 1e-11."""
    models = R.case_models(name, cx)
    n64, b64 = R.normalised_ref(models)
    nld, bld = R.normalised_ref(models, dtype=np.longdouble)
    worst_n = max(float(np.abs(x - y).max()) for x, y in zip(n64, nld))
    worst_o = max(float(np.abs(b64[q] - bld[q]).max()) for q in b64)
    print(f"{name}-{'complex' if cx else 'real'}: normalised overlap {worst_o:.2e}, ln norm {worst_n:.2e}")
    assert worst_o <= 1e-11 and worst_n <= 1e-11


def test_zero_states_and_embedding():
    rng = np.random.default_rng(3)
    A = gaussian_chain(6, 3, 4, 2, 3, False, rng)
    dead = [t.copy() for t in A]
    dead[3][..., 0] = 0.0
    log_norm, blocks = R.normalised_ref([dead])
    assert log_norm[0][0] == -np.inf and np.isfinite(log_norm[0][1])
    assert np.all(np.isnan(blocks[(0, 0)][0])) and np.all(np.isnan(blocks[(0, 0)][:, 0])) and abs(blocks[(0, 0)][1, 1] - 1.0) <= 1e-14
    gone = [np.zeros_like(t) for t in A]
    g, lg = R.overlap_ref(gone, A)
    assert np.all(g == 0) and lg == -np.inf
    # eps = 0 embeds exactly: the larger chain is the same state
    B = R.embed(A, 7, 0.0, rng)
    assert max(t.shape[2] for t in B) == 7
    _, blocks = R.normalised_ref([A, B], [(0, 1)])
    assert np.abs(np.abs(np.diagonal(blocks[(0, 1)])) - 1.0).max() <= 1e-13
