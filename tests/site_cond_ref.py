"""NumPy restatement of the leave-one-out site conditionals (mpst_site_conditionals): for a complete series and every site t the
distribution of x_t given all the other values, from the pieces of oracle/impute_numpy.py - ``brute_force_conditional`` with
exactly one unknown site (density-matrix environments, the reference's |rho phi|^2), ``cumul_trapz_even`` and ``weighted_median``.
The density at the observed value comes from a second ``brute_force_conditional`` call on the one-row "grid" phi[i][t], so that
numerator and Z carry the same constant factor.  TEST INFRASTRUCTURE ONLY (checker of tests/test_site_cond_host.py and
tests/test_gpu_site_cond.py).

``brute_force_conditional`` does not rescale, so a chain of a thousand sites underflows in it; ``scaled_site_conditionals`` is the
definition itself (two vector walks, every site divided by its largest magnitude) and tests/test_site_cond_host.py pins it against
the brute-force form on the short chains."""
from dataclasses import dataclass

import numpy as np

import mpstime_jl_amd as mt
from oracle import impute_numpy as I
from tests.marginal_ref import class_slice, gaussian_chain, label_site_of, normalised_chain


@dataclass
class SiteCondRef:
    x: np.ndarray           # (N, T)
    F: np.ndarray           # (N, T, ngrid) normalised cdf
    nll: np.ndarray         # (N, T)
    pit: np.ndarray         # (N, T)
    med_idx: np.ndarray     # (N, T) grid index of the median
    median: np.ndarray      # (N, T)
    err: np.ndarray         # (N, T) WMAD
    lev_idx: np.ndarray     # (N, T, nq)
    quantiles: np.ndarray   # (N, T, nq)
    med_margin: np.ndarray  # (N, T) gap between the best and second-best |F - 0.5|
    lev_margin: np.ndarray  # (N, T, nq) ... |F - q|
    err_margin: np.ndarray  # (N, T) distance of the WMAD's cumulative weight (and of the largest single weight) from one half

    def margins_ok(self, tol=1e-9):
        return bool(self.med_margin.min() > tol and self.err_margin.min() > tol and (self.lev_margin.size == 0 or self.lev_margin.min() > tol))


def selection_margin(F, q):
    dd = np.sort(np.abs(F - q))[:2]
    return float(dd[1] - dd[0])


def wmad_margin(xs, k, w):
    """How far weighted_median(|xs - xs[k]|, w) is from deciding otherwise: the smallest distance of a cumulative weight (in its
    order) and of the largest single weight from half the total, relative to the total."""
    v = np.abs(xs - xs[k])
    tot = w.sum()
    cw = np.cumsum(w[np.argsort(v, kind="stable")])
    return float(min(np.abs(cw - 0.5 * tot).min(), abs(w.max() - 0.5 * tot)) / tot)


def pit_at(xs, F, x):
    """F at x, linear between the neighbouring grid values; 0 below the grid, 1 above (F[0] = 0, F[-1] = 1)."""
    return float(np.interp(x, xs, F))


def _finish(out, i, t, xs, p, pobs, x, levels):
    cdf = I.cumul_trapz_even(xs, p)
    Z = cdf[-1]
    F = cdf / Z
    k = int(np.argmin(np.abs(F - 0.5)))
    out.F[i, t] = F
    out.med_idx[i, t], out.median[i, t] = k, xs[k]
    out.err[i, t] = I.weighted_median(np.abs(xs - xs[k]), p / Z)
    out.med_margin[i, t] = selection_margin(F, 0.5)
    out.err_margin[i, t] = wmad_margin(xs, k, p / Z)
    for l, q in enumerate(levels):
        kl = int(np.argmin(np.abs(F - q)))
        out.lev_idx[i, t, l], out.quantiles[i, t, l] = kl, xs[kl]
        out.lev_margin[i, t, l] = selection_margin(F, q)
    with np.errstate(divide="ignore"):
        out.nll[i, t] = -np.log(pobs / Z)
    out.pit[i, t] = pit_at(xs, F, x)


def _empty(x, ngrid, nq):
    N, T = x.shape
    z = lambda *s, dt=np.float64: np.zeros(s, dtype=dt)
    return SiteCondRef(np.array(x, dtype=np.float64), z(N, T, ngrid), z(N, T), z(N, T), z(N, T, dt=np.int64), z(N, T), z(N, T), z(N, T, nq, dt=np.int64),
                       z(N, T, nq), z(N, T), z(N, T, nq), z(N, T))


def site_conditionals_ref(W, phi, lab, x, xs, grid_phi, levels=()):
    """The definition per (series, site) through brute_force_conditional.  ``W``: site tensors with the label site (Dl, d, Dr, C)
    anywhere; ``phi`` (N, T, d); ``lab`` (N,) class indices; ``x`` (N, T); ``grid_phi`` (ngrid, d) or (T, ngrid, d)."""
    N, T = x.shape
    out = _empty(x, len(xs), len(levels))
    slices = {c: class_slice(W, c) for c in set(int(c) for c in lab)}
    for i in range(N):
        cm = slices[int(lab[i])]
        for t in range(T):
            known = np.ones(T, dtype=bool)
            known[t] = False
            g = grid_phi[t] if grid_phi.ndim == 3 else grid_phi
            p = I.brute_force_conditional(cm, phi[i], known, t, {}, g)
            pobs = I.brute_force_conditional(cm, phi[i], known, t, {}, phi[i, t][None])[0]
            _finish(out, i, t, xs, p, pobs, x[i, t], levels)
    return out


def amplitudes(cm, enc, return_scales=False):
    """a_t of the definition for every t: l_j = l_{j-1} M_j and r_j = M_j r_{j+1}, each divided by its largest magnitude.
    ``return_scales``: also ln of the factor every a_t was divided by on the way (the scales of l_{t-1} and r_{t+1})."""
    T = len(cm)
    M = [np.einsum("asb,s->ab", cm[j], np.conj(enc[j])) for j in range(T)]
    l, ll = [np.ones(1)], [0.0]
    for j in range(T):
        v = l[-1] @ M[j]
        l.append(v / np.abs(v).max())
        ll.append(ll[-1] + np.log(np.abs(v).max()))
    r, lr = [np.ones(1)], [0.0]
    for j in range(T - 1, -1, -1):
        v = M[j] @ r[-1]
        r.append(v / np.abs(v).max())
        lr.append(lr[-1] + np.log(np.abs(v).max()))
    r, lr = r[::-1], lr[::-1]
    a = [np.einsum("a,asb,b->s", l[t], cm[t], r[t + 1]) for t in range(T)]
    return (a, [ll[t] + lr[t + 1] for t in range(T)]) if return_scales else a


def scaled_site_conditionals(W, phi, lab, x, xs, grid_phi, levels=()):
    """The same outputs from the definition as stated (vector walks, rescaled at every site): for chains whose unscaled environments
    leave the range of fp64."""
    N, T = x.shape
    out = _empty(x, len(xs), len(levels))
    slices = {c: class_slice(W, c) for c in set(int(c) for c in lab)}
    for i in range(N):
        a = amplitudes(slices[int(lab[i])], phi[i])
        for t in range(T):
            g = grid_phi[t] if grid_phi.ndim == 3 else grid_phi
            p = np.abs(np.conj(g) @ a[t]) ** 2
            pobs = float(np.abs(np.conj(phi[i, t]) @ a[t]) ** 2)
            _finish(out, i, t, xs, p, pobs, x[i, t], levels)
    return out


def make_case(T, d, chi, C, N, seed, cx=False, label_site=None, ngrid=201, long_chain=False):
    """(W, phi, lab, x, xs, grid_phi) of a test case: Gaussian site tensors (a QR-normalised chain with the label on the last site for
    ``long_chain``), Legendre states on [-1, 1] for real models and Fourier states for complex ones, values inside (-0.95, 0.95)."""
    rng = np.random.default_rng(seed)
    if long_chain:
        W = normalised_chain(T, d, chi, C, rng, cx)
    else:
        W = gaussian_chain(T, d, chi, C, T - 1 if label_site is None else label_site, cx, rng)
    enc = mt.model_encoding("Fourier" if cx else "Legendre_No_Norm")
    xs = np.linspace(-1.0, 1.0, ngrid)
    grid_phi = np.asarray(enc.encode(xs, d))
    x = rng.uniform(-0.95, 0.95, (N, T))
    phi = np.asarray(enc.encode(x.ravel(), d)).reshape(N, T, d)
    lab = (np.arange(N) % C).astype(np.int32)
    assert label_site_of(W) == (T - 1 if label_site is None or long_chain else label_site)
    return W, phi, lab, x, xs, grid_phi
