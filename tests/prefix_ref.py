"""NumPy restatement of the prefix marginals (mpst_prefix_marginals): ``log_marginals_ref`` of tests/marginal_ref.py - the density
recursion per (instance, class), the code the marginal likelihoods are pinned to - stacked over the suffix masks
``mask[:, t:] = True``, t = 0 .. T (or the prefix lengths asked for)."""
import numpy as np

from tests import marginal_ref as MR


def suffix_mask(N, T, t):
    m = np.zeros((N, T), dtype=bool)
    m[:, t:] = True
    return m


def prefix_log_marginals_ref(W, phi, lengths=None):
    """(N, len(lengths), C) ln l_c(i; t) for t in ``lengths`` (None: 0 .. T)"""
    N, T = phi.shape[:2]
    ts = range(T + 1) if lengths is None else lengths
    return np.stack([MR.log_marginals_ref(W, phi, suffix_mask(N, T, t)) for t in ts], axis=1)
