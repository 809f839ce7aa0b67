"""NumPy restatement of the segment marginals (mpst_segment_marginals): ``log_marginals_ref`` of tests/marginal_ref.py - the density
recursion per (instance, class), the code the marginal likelihoods are pinned to - over the complement masks, set everywhere but on the
sites a .. a+w-1, for every start a and width w <= max_width inside the series (or the (a, w) pairs asked for)."""
import numpy as np

from tests import marginal_ref as MR


def complement_mask(N, T, a, w):
    m = np.ones((N, T), dtype=bool)
    m[:, a:a + w] = False
    return m


def all_segments(T, max_width):
    return [(a, w) for a in range(T) for w in range(1, max_width + 1) if a + w <= T]


def segment_log_marginals_ref(W, phi, max_width, segments=None):
    """(N, T, max_width, C) ln l_c(i; a, w) at [i, a, w - 1, c]; NaN where a + w > T and, with ``segments`` (a list of (a, w) pairs),
    at every segment that is not listed"""
    N, T = phi.shape[:2]
    Cn = W[MR.label_site_of(W)].shape[3]
    out = np.full((N, T, max_width, Cn), np.nan)
    for a, w in (all_segments(T, max_width) if segments is None else segments):
        assert 0 <= a and 1 <= w <= max_width and a + w <= T
        out[:, a, w - 1] = MR.log_marginals_ref(W, phi, complement_mask(N, T, a, w))
    return out
