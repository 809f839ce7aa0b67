"""NumPy restatement of the pair analysis (mpst_pair_analysis) in two forms.

``brute_force`` builds the dense d^T state of every class MPS and reads rho_i and rho_ij off it by reshaping: no gauge and no
recursion.  ``transfer`` is the recursion the device runs - right-canonical tensors, the left densities L_i, the carried blocks
E^{ss'} - written as matrix products, for shapes the dense state cannot reach.  Both return (mi, mean, cov): (C, T, T), (C, T),
(C, T, T) arrays (mean and cov None without an observable), with the single-site entropies on the diagonal of mi and the variances
on the diagonal of cov.

Site tensors are (Dl, d, Dr); the label site of a model is (Dl, d, Dr, C).  O is None, (d, d) or (T, d, d), real symmetric."""
from __future__ import annotations

import numpy as np

from tests import analysis_ref as A


def chain_model(chi, d, C, label=None, seed=0):
    """Random site tensors with the bond dimensions chi[0..T] (chi[0] = chi[T] = 1); the label index on site ``label`` (default: last)."""
    rng = np.random.default_rng(seed)
    T = len(chi) - 1
    label = T - 1 if label is None else label
    return [rng.standard_normal((chi[j], d, chi[j + 1]) + ((C,) if j == label else ())) for j in range(T)]


def ghz_model(T, C=1):
    """(|00..0> + |11..1>) / sqrt 2 with d = 2 and bonds of 2 (every class the same state)."""
    W = []
    for j in range(T):
        Dl, Dr = (1 if j == 0 else 2), (1 if j == T - 1 else 2)
        a = np.zeros((Dl, 2, Dr))
        for s in range(2):
            a[0 if j == 0 else s, s, 0 if j == T - 1 else s] = 1.0
        W.append(a)
    W[-1] = np.repeat(W[-1][..., None], C, axis=3)
    return W


def entropy(rho):
    """The entropy rule: with lam the eigenvalues of (rho + rho^T) / 2, -sum over lam > 0 of lam ln lam; NaN stays NaN."""
    rho = np.asarray(rho)
    if not np.all(np.isfinite(rho)):
        return np.nan
    lam = np.linalg.eigvalsh(0.5 * (rho + rho.T))
    lam = lam[lam > 0.0]
    return float(-(lam * np.log(lam)).sum())


def _site_obs(O, T, d):
    if O is None:
        return None
    O = np.asarray(O, dtype=np.float64)
    return np.broadcast_to(O, (T, d, d)) if O.ndim == 2 else O


def _assemble(T, S1, Sij, rho1, craw, O):
    mi = np.zeros((T, T))
    for i in range(T):
        mi[i, i] = S1[i]
        for j in range(i + 1, T):
            mi[i, j] = mi[j, i] = S1[i] + S1[j] - Sij[i, j]
    if O is None:
        return mi, None, None
    mean = np.array([np.sum(rho1[i] * O[i]) for i in range(T)])
    cov = np.zeros((T, T))
    for i in range(T):
        cov[i, i] = np.sum(rho1[i] * (O[i] @ O[i])) - mean[i] ** 2
        for j in range(i + 1, T):
            cov[i, j] = cov[j, i] = craw[i, j] - mean[i] * mean[j]
    return mi, mean, cov


def _stack(per_class):
    mi = np.stack([r[0] for r in per_class])
    if per_class[0][1] is None:
        return mi, None, None
    return mi, np.stack([r[1] for r in per_class]), np.stack([r[2] for r in per_class])


def dense_state(m: A.MPS):
    psi = np.ones((1, 1))
    for a in m.t:
        psi = np.tensordot(psi, a, axes=(psi.ndim - 1, 0))
    return psi.reshape(psi.shape[1:-1])


def brute_force(W, O=None):
    """From the dense state of every class MPS (A.expand_label_index: the label slice, normalised)."""
    out = []
    for m in A.expand_label_index(W):
        T, d = len(m), m.t[0].shape[1]
        Os = _site_obs(O, T, d)
        with np.errstate(invalid="ignore", divide="ignore"):
            psi = dense_state(m)
        rho1, S1 = [], np.zeros(T)
        Sij, craw = np.zeros((T, T)), np.zeros((T, T))
        for i in range(T):
            M = np.moveaxis(psi, i, 0).reshape(d, -1)
            rho1.append(M @ M.T)
            S1[i] = entropy(rho1[i])
            for j in range(i + 1, T):
                M2 = np.moveaxis(psi, (i, j), (0, 1)).reshape(d * d, -1)
                rho = M2 @ M2.T                                     # [(s, t), (s', t')]
                Sij[i, j] = entropy(rho)
                if Os is not None:
                    craw[i, j] = np.sum(rho * np.kron(Os[i], Os[j]))
        out.append(_assemble(T, S1, Sij, rho1, craw, Os))
    return _stack(out)


def transfer(W, O=None):
    """The recursion of the device as matrix products.  With B_j right-canonical and L_i the left density at bond i:
    E_i^{ss'} = B_i^sT L_i B_i^s',  rho_ij[(s,t),(s',t')] = <B_j^t, E^{ss'} B_j^t'>_F,  E^{ss'} <- sum_t B_j^tT E^{ss'} B_j^t."""
    out = []
    for m in A.expand_label_index(W):
        m = m.copy()
        m.orthogonalize(0)
        B = m.t
        T, d = len(B), B[0].shape[1]
        Os = _site_obs(O, T, d)
        rho1, S1 = [], np.zeros(T)
        Sij, craw = np.zeros((T, T)), np.zeros((T, T))
        L = np.ones((1, 1))
        for i in range(T):
            Dl, _, Dr = B[i].shape
            Bm = B[i].reshape(Dl, d * Dr)
            E = (Bm.T @ (L @ Bm)).reshape(d, Dr, d, Dr).transpose(0, 2, 1, 3)       # [s, s', a, b]
            rho1.append(np.trace(E, axis1=2, axis2=3))
            S1[i] = entropy(rho1[i])
            L = np.einsum("ssab->ab", E)
            for j in range(i + 1, T):
                Bj = B[j]                                                           # [a, t, c]
                Y = np.tensordot(E, Bj, axes=(3, 0))                                # [s, s', a, t', c]
                rho = np.tensordot(Y, Bj, axes=((2, 4), (0, 2)))                    # [s, s', t', t]
                rho = rho.transpose(0, 3, 1, 2).reshape(d * d, d * d)               # [(s, t), (s', t')]
                Sij[i, j] = entropy(rho)
                if Os is not None:
                    craw[i, j] = np.sum(rho * np.kron(Os[i], Os[j]))
                if j + 1 < T:
                    E = np.tensordot(Y, Bj, axes=((2, 3), (0, 1))).transpose(0, 1, 3, 2)    # [s, s', c', c]: B^tT Y^t
        out.append(_assemble(T, S1, Sij, rho1, craw, Os))
    return _stack(out)
