"""NumPy restatement of the marginal site conditionals (mpst_marginal_conditionals): for a series with missing sites and EVERY site t
the distribution of x_t given the known values of the other sites, the missing ones summed over their physical index (Born rule).

    L_{t-1}, R_{t+1}   the density recursion of tests/marginal_ref._step from the two ends of the chain (trace one at every site
                       with ``scaled``),
    rho_t[s, s'] = sum L_{t-1}[a, a'] W_t[a, s, b] conj(W_t[a', s', b']) R_{t+1}[b, b'],
    p_k = max(Re(g_k^H rho_t g_k), 0),  cdf / Z / F and the selections as in tests/site_cond_ref.py,  mean = trapezoid(x p) / Z,
    nll = -ln(phi_t^H rho_t phi_t / Z),  pit = F(x_t)   wherever x[i][t] is finite, NaN elsewhere.

``dense_rho`` is rho_t from the full d^T amplitude tensor (tiny chains only).  TEST INFRASTRUCTURE ONLY (checker of
tests/test_margcond_host.py and tests/test_gpu_margcond.py)."""
from dataclasses import dataclass

import numpy as np

from oracle import impute_numpy as I
from tests import site_cond_ref as S
from tests.marginal_ref import class_slice, label_site_of


def _step(E, A, phi_j, missing):
    """tests/marginal_ref._step with matrix products (bond dimensions of 72 in the GPU test): E' = sum_s A[:, s, :]^T E conj(A[:, s, :])
    at a missing site, M^T E conj(M) with M = sum_s conj(phi_j[s]) A[:, s, :] at a known one"""
    if missing:
        return sum(A[:, s, :].T @ E @ np.conj(A[:, s, :]) for s in range(A.shape[1]))
    M = np.einsum("s,asb->ab", np.conj(phi_j), A)
    return M.T @ E @ np.conj(M)


@dataclass
class MargCondRef:
    sc: S.SiteCondRef           # F, nll, pit, median, err, quantiles and the selection margins
    mean: np.ndarray            # (N, T)
    rho: np.ndarray             # (N, T, d, d), as the walks left it (trace one up to the site's own factor with ``scaled``)
    excused: np.ndarray         # (N, T) bool: a selection margin of the pair is at most 1e-9


def density_walks(cm, enc, miss, scaled=True):
    """(L, R): L[t] = L_{t-1} over the left bond of site t, R[t] = R_{t+1} over its right bond; enc[j] is not read where miss[j]."""
    T = len(cm)
    norm = (lambda E: E / np.trace(E).real) if scaled else (lambda E: E)
    L = [np.ones((1, 1), dtype=cm[0].dtype)]
    for j in range(T - 1):
        L.append(norm(_step(L[-1], cm[j], None if miss[j] else enc[j], miss[j])))
    R = [np.ones((1, 1), dtype=cm[0].dtype)]
    for j in range(T - 1, 0, -1):
        R.append(norm(_step(R[-1], cm[j].transpose(2, 1, 0), None if miss[j] else enc[j], miss[j])))
    return L, R[::-1]


def rho_site(L, Wt, R):
    LW = np.einsum("ac,asb->csb", L, Wt)                        # sum_a L[a, a'] W[a, s, b]
    CR = np.einsum("ctd,bd->ctb", np.conj(Wt), R)               # sum_b' conj(W[a', s', b']) R[b, b']
    return np.einsum("csb,ctb->st", LW, CR)


def grid_density(rho, g):
    return np.maximum(np.einsum("ks,st,kt->k", np.conj(g), rho, g).real, 0.0)


def dense_rho(cm, enc, miss, t):
    """rho_t from the amplitude tensor psi[s_1 ... s_T]: the known sites but t projected on conj(phi), the missing ones kept and summed."""
    psi = cm[0][0]
    for w in cm[1:]:
        psi = np.tensordot(psi, w, axes=([psi.ndim - 1], [0]))
    psi = psi[..., 0]
    ax, at = 0, None
    for j in range(len(cm)):
        if j == t:
            at = ax
            ax += 1
        elif miss[j]:
            ax += 1
        else:
            psi = np.tensordot(psi, np.conj(enc[j]), axes=([ax], [0]))
    psi = np.moveaxis(psi, at, 0).reshape(psi.shape[at], -1)
    return psi @ np.conj(psi.T)


def marginal_conditionals_ref(W, phi, lab, miss, x, xs, grid_phi, levels=(), scaled=True):
    """``x`` (N, T): NaN where no value is supplied (nll and pit are then NaN; phi[i][t] is not read there if the site is missing)."""
    N, T = x.shape
    d = W[0].shape[1]
    sc = S._empty(x, len(xs), len(levels))
    mean = np.zeros((N, T))
    rho = np.zeros((N, T, d, d), dtype=np.result_type(W[0].dtype, phi.dtype))
    slices = {c: class_slice(W, c) for c in set(int(c) for c in lab)}
    for i in range(N):
        cm = slices[int(lab[i])]
        L, R = density_walks(cm, phi[i], miss[i], scaled)
        for t in range(T):
            r = rho_site(L[t], cm[t], R[t])
            rho[i, t] = r
            g = grid_phi[t] if grid_phi.ndim == 3 else grid_phi
            p = grid_density(r, g)
            pobs = float((np.conj(phi[i, t]) @ r @ phi[i, t]).real) if np.isfinite(x[i, t]) else np.nan
            S._finish(sc, i, t, xs, p, pobs, x[i, t], levels)
            if np.isfinite(x[i, t]) and not pobs > 0.0:
                sc.nll[i, t] = np.inf
            mean[i, t] = I.cumul_trapz_even(xs, xs * p)[-1] / I.cumul_trapz_even(xs, p)[-1]
    margin = np.minimum(sc.med_margin, sc.err_margin)
    if len(levels):
        margin = np.minimum(margin, sc.lev_margin.min(axis=2))
    return MargCondRef(sc, mean, rho, margin <= 1e-9)


def make_masks(N, T, rng):
    """The patterns of the GPU test, one per row and then scattered 30 %: nothing missing, everything missing, the first and the last
    site, a run of adjacent sites, a single site; rows beyond the fifth (and both rows of a two-row case) are scattered or a run."""
    miss = rng.uniform(size=(N, T)) < 0.3
    run = np.zeros(T, dtype=bool)
    run[T // 3:max(T // 3 + 1, 2 * T // 3)] = True
    if N == 2:
        miss[1] = run
        miss[1, 0] = miss[1, T - 1] = True
        return miss
    pats = [np.zeros(T, dtype=bool), np.ones(T, dtype=bool), np.arange(T) % max(T - 1, 1) == 0, run, np.arange(T) == T // 2]
    for r, p in enumerate(pats[:N]):
        miss[r] = p
    return miss


def full_bond_chain(T, d, chi, C, label_site, cx, rng):
    """Gaussian site tensors whose inner bonds all have dimension chi (the bonds next to the ends d): a bond of 72 on a chain of six
    sites, which tests/marginal_ref.gaussian_chain caps at d^3 = 64.  Scaled so that the densities stay near one."""
    dims = [1] + [chi if min(j, T - j) >= 2 else min(chi, d ** min(j, T - j)) for j in range(1, T)] + [1]
    W = []
    for j in range(T):
        shape = (dims[j], d, dims[j + 1]) + ((C,) if j == label_site else ())
        t = rng.standard_normal(shape)
        if cx:
            t = t + 1j * rng.standard_normal(shape)
        W.append(t / np.sqrt(dims[j] * d))
    return W


def make_case(T, d, chi, C, N, seed, cx=False, label_site=None, ngrid=201, long_chain=False, per_site=False, full_bonds=False):
    """(W, phi, lab, miss, x_in, xs, grid_phi, x_true): a case of tests/site_cond_ref.make_case with masks.  Every second row supplies
    the true value at its missing sites (held-out scores); on the other rows x_in is NaN there and phi is poisoned with NaN - the
    call must not read it."""
    W, phi, lab, x, xs, grid_phi = S.make_case(T, d, chi, C, N, seed, cx=cx, label_site=label_site, ngrid=ngrid, long_chain=long_chain)
    rng = np.random.default_rng(seed + 7919)
    if full_bonds:
        W = full_bond_chain(T, d, chi, C, label_site_of(W), cx, rng)
    miss = make_masks(N, T, rng)
    if per_site:        # one table per site: the shared one, each site's states rotated by its own sign / phase pattern
        sg = np.where(rng.uniform(size=(T, 1, d)) < 0.5, -1.0, 1.0)
        grid_phi = grid_phi[None] * sg
        phi = phi * sg[:, 0][None]
    held = miss & (np.arange(N)[:, None] % 2 == 0)
    x_in = np.where(miss & ~held, np.nan, x)
    phi = np.array(phi)
    phi[miss & ~held] = np.nan
    return W, phi, lab, miss, x_in, xs, grid_phi, x
