"""NumPy restatement of the rolling-origin forecasts (mpst_rolling_forecasts): ``marginal_conditionals_ref`` of tests/margcond_ref.py -
the code the marginal site conditionals are pinned to - on the suffix mask ``mask[:, t:] = True`` of every origin t (or of the origins
asked for), read at the sites t .. t+H-1.  ``suffix_conditionals`` is that call made of its own pieces (``density_walks``, ``rho_site``,
``grid_density``, ``site_cond_ref._finish``) for the sites that are read only - a chain of a thousand sites would finish a thousand
sites per origin for eight - and tests/test_rolling_host.py holds it to the whole call bit for bit.  For a series under the class
mixture (``lab = -1``) the rho of the per-class walks with ``scaled=False`` are summed and finished the same way.  On a long chain the
unscaled walks leave the range of fp64; ``weighted`` states the same sum from the scaled walks: every class's rho at trace one times
its prefix likelihood (the trace of the unscaled rho), from ``marginal_ref.log_marginals_ref``.  TEST INFRASTRUCTURE ONLY."""
from dataclasses import dataclass

import numpy as np

from oracle import impute_numpy as I
from tests import margcond_ref as M
from tests import marginal_ref as MR
from tests import site_cond_ref as S
from tests.prefix_ref import suffix_mask


@dataclass
class RollingRef:
    nll: np.ndarray             # (N, T, H), entry [i, t, h - 1]; NaN beyond the chain and at origins that were not restated
    pit: np.ndarray
    median: np.ndarray
    err: np.ndarray
    mean: np.ndarray
    quantiles: np.ndarray       # (N, T, H, nq)
    rho: np.ndarray             # (N, T, H, d, d); a labelled row: as the scaled walks left it; a mixture row: the class sum
    excused: np.ndarray         # (N, T, H) bool: a selection margin of the triple is at most 1e-9
    done: np.ndarray            # (T, H) bool: the triple was restated


def suffix_rho(cm, enc, t, sites, scaled=True):
    """rho_u of marginal_conditionals_ref for the suffix mask of t, u in ``sites``"""
    miss = np.arange(len(cm)) >= t
    L, R = M.density_walks(cm, enc, miss, scaled)
    return [M.rho_site(L[u], cm[u], R[u]) for u in sites]


def _finish(out, i, t, h, rho, phi_u, x_u, xs, g, levels):
    """the part of marginal_conditionals_ref after rho, into the triple (i, t, h)"""
    sc = S._empty(np.array([[x_u]]), len(xs), len(levels))
    p = M.grid_density(rho, g)
    pobs = float((np.conj(phi_u) @ rho @ phi_u).real)
    S._finish(sc, 0, 0, xs, p, pobs, x_u, levels)
    out.nll[i, t, h] = sc.nll[0, 0] if pobs > 0.0 else np.inf
    out.pit[i, t, h], out.median[i, t, h], out.err[i, t, h] = sc.pit[0, 0], sc.median[0, 0], sc.err[0, 0]
    out.mean[i, t, h] = I.cumul_trapz_even(xs, xs * p)[-1] / I.cumul_trapz_even(xs, p)[-1]
    out.quantiles[i, t, h], out.rho[i, t, h] = sc.quantiles[0, 0], rho
    margin = min([sc.med_margin[0, 0], sc.err_margin[0, 0]] + sc.lev_margin[0, 0].tolist())
    out.excused[i, t, h] = margin <= 1e-9


def mixture_rho(W, enc, t, sites, weighted=False):
    """sum_c rho_c of the sites on the suffix mask of t, every class at its stored scale (``weighted``: up to one factor for all)"""
    Cn = W[MR.label_site_of(W)].shape[3]
    if not weighted:
        per = [suffix_rho(MR.class_slice(W, c), enc, t, sites, scaled=False) for c in range(Cn)]
        return [sum(per[c][k] for c in range(Cn)) for k in range(len(sites))]
    lp = MR.log_marginals_ref(W, enc[None], suffix_mask(1, len(W), t))[0]           # (C,): ln tr of the unscaled rho_c
    w = np.exp(lp - lp.max())
    per = [suffix_rho(MR.class_slice(W, c), enc, t, sites, scaled=True) for c in range(Cn)]
    return [sum(w[c] * per[c][k] / np.trace(per[c][k]).real for c in range(Cn)) for k in range(len(sites))]


def rolling_forecasts_ref(W, phi, lab, x, xs, grid_phi, H, levels, origins=None, weighted=False):
    N, T = x.shape
    d, nq = W[0].shape[1], len(levels)
    lab = np.asarray(lab)
    nan = lambda *s: np.full(s, np.nan)
    out = RollingRef(nan(N, T, H), nan(N, T, H), nan(N, T, H), nan(N, T, H), nan(N, T, H), nan(N, T, H, nq),
                     np.zeros((N, T, H, d, d), dtype=np.result_type(W[0].dtype, phi.dtype)), np.zeros((N, T, H), dtype=bool),
                     np.zeros((T, H), dtype=bool))
    slices = {c: MR.class_slice(W, c) for c in set(int(c) for c in lab if c >= 0)}
    for t in (range(T) if origins is None else origins):
        sites = [t + h for h in range(H) if t + h < T]
        out.done[t, :len(sites)] = True
        for i in range(N):
            rhos = suffix_rho(slices[int(lab[i])], phi[i], t, sites) if lab[i] >= 0 else mixture_rho(W, phi[i], t, sites, weighted)
            for h, u in enumerate(sites):
                _finish(out, i, t, h, rhos[h], phi[i, u], x[i, u], xs, grid_phi[u] if grid_phi.ndim == 3 else grid_phi, levels)
    return out
