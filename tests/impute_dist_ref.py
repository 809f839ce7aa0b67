"""NumPy restatement of the reference's get_rdms_with_med / impute_med_and_get_cdf! (src/Imputation/MPS_methods.jl:350-466, with get_cdf,
src/Imputation/sampling_utils.jl:205-241) from the pieces of oracle/impute_numpy.py: the median imputer, and for every missing site the
normalised cumulative trapezoid its median was read from, plus argmin_k |cdf_k - q| for given levels.  TEST INFRASTRUCTURE ONLY (checker
of tests/test_impute_dist_host.py and tests/test_gpu_impute_dist.py); pinned against the brute-force conditional densities there."""
import numpy as np

from oracle import impute_numpy as I


def impute_med_and_cdfs(class_mps, enc, imputation_sites, xs, grid_phi, order="forwards", levels=()):
    """Returns (median, wmad, cdfs, level_idx, states), each indexed by the RANK of the missing site in ascending site order whatever the
    imputation order (cdfs[i] by position in the conditioned MPS, MPS_methods.jl:413): median (n,), wmad (n,), cdfs (n, ngrid),
    level_idx (n, nq) grid indices, states (n, d) the state the chain was conditioned on (the median's, unnormalised)."""
    sites = sorted(int(j) for j in imputation_sites)
    cond = I.precondition(class_mps, enc, sites)
    n = len(cond)
    if order == "forwards":
        t = I._right_orthogonalize(cond)
        idxs = list(range(n))
        A = t[0][0]
    else:
        t = I._left_orthogonalize(cond)
        idxs = list(range(n - 1, -1, -1))
        A = t[-1][:, :, 0].T
    med, wm = np.zeros(n), np.zeros(n)
    cdfs = np.zeros((n, len(xs)))
    lidx = np.zeros((n, len(levels)), dtype=np.int64)
    states = np.zeros((n, grid_phi.shape[1]), dtype=grid_phi.dtype)
    for ii, i in enumerate(idxs):
        p = I.probs_from_rdm(A, grid_phi)
        cdf = I.cumul_trapz_even(xs, p)
        Z = cdf[-1]
        cdf = cdf / Z
        k = int(np.argmin(np.abs(cdf - 0.5)))
        med[i] = xs[k]
        wm[i] = I.weighted_median(np.abs(xs - xs[k]), p / Z)
        cdfs[i] = cdf
        states[i] = grid_phi[k]
        for l, q in enumerate(levels):
            lidx[i, l] = int(np.argmin(np.abs(cdf - q)))
        if ii != n - 1:
            Am = np.conj(grid_phi[k] / np.sqrt(Z)) @ A
            nxt = t[idxs[ii + 1]]
            A = np.einsum("a,asb->sb", Am, nxt) if order == "forwards" else np.einsum("asb,b->sa", nxt, Am)
            A = A / np.max(np.abs(A))
    return med, wm, cdfs, lidx, states
