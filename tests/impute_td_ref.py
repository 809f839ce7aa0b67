"""impute_at! (src/Imputation/MPS_methods.jl:103-177) with one grid table PER SITE, as the reference runs it for a time-dependent
encoding (x_guess_range.xvals_enc[j], imputation.jl:92-99; MPS_methods.jl:124-157 index it with the site).  The loop of
oracle.impute_numpy.impute_at with `grid_phi[imputation_sites[i]]` at the i-th conditioned site; preconditioning, the
orthogonalisation, the cumulative trapezoid, the weighted median and the density are the oracle's own functions."""
import numpy as np

from oracle import impute_numpy as I


def impute_at(cond, sites, xs, grid_phi, method="median", order="forwards", get_wmad=True, u=None, rejection_threshold=None,
              max_trials=10, return_cdfs=False):
    """``sites``: the chain positions of the conditioned tensors ``cond`` (ascending); ``grid_phi`` (T, ngrid, d).  Methods: median,
    mode, quantile (``u[k]`` for the k-th conditioned site in the order of the sweep; with ``rejection_threshold`` up to max_trials
    numbers each).  Returns (x, err) per conditioned site - and the list of normalised cdfs in ascending site order with return_cdfs."""
    n = len(cond)
    if order == "forwards":
        t = I._right_orthogonalize(cond)
        idxs = list(range(n))
        A = t[0][0]
    else:
        t = I._left_orthogonalize(cond)
        idxs = list(range(n - 1, -1, -1))
        A = t[-1][:, :, 0].T
    xout, eout, cdfs = np.zeros(n), np.zeros(n), [None] * n
    for ii, i in enumerate(idxs):
        gp = grid_phi[sites[i]]                                  # this site's table
        p = I.probs_from_rdm(A, gp)
        if method == "mode":
            k = int(np.argmax(p))
            ms, xk, err = gp[k], xs[k], 0.0
        else:
            cdf = I.cumul_trapz_even(xs, p)
            Z = cdf[-1]
            cdf = cdf / Z
            cdfs[i] = cdf
            pn = p / Z
            if method == "median":
                k = int(np.argmin(np.abs(cdf - 0.5)))
                err = I.weighted_median(np.abs(xs - xs[k]), pn) if get_wmad else 0.0
            elif rejection_threshold is None:
                k = int(np.argmin(np.abs(cdf - float(np.ravel(u[ii])[0]))))
                err = 0.0
            else:
                km = int(np.argmin(np.abs(cdf - 0.5)))
                err = I.weighted_median(np.abs(xs - xs[km]), pn)
                k = km
                for trial in range(max_trials):
                    k = int(np.argmin(np.abs(cdf - float(u[ii][trial]))))
                    if abs(xs[k] - xs[km]) < rejection_threshold * err:
                        break
            ms, xk = gp[k] / np.sqrt(Z), xs[k]
        xout[i], eout[i] = xk, err
        if ii != n - 1:
            Am = np.conj(ms) @ A
            nxt = t[idxs[ii + 1]]
            A = np.einsum("a,asb->sb", Am, nxt) if order == "forwards" else np.einsum("asb,b->sa", nxt, Am)
            A = A / np.max(np.abs(A))
    return (xout, eout, cdfs) if return_cdfs else (xout, eout)


def impute(class_mps, enc, imputation_sites, xs, grid_phi, method="median", order="forwards", get_wmad=True, u=None, **kw):
    """oracle.impute_numpy.impute with a per-site table grid_phi (T, ngrid, d)."""
    imp = sorted(int(j) for j in imputation_sites)
    return impute_at(I.precondition(class_mps, enc, imp), imp, xs, grid_phi, method, order, get_wmad, u, **kw)
