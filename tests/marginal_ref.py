"""NumPy restatement of the marginal likelihoods (mpst_marginal_model): per (instance, class) the density recursion from the
left end of the chain, rescaled by its trace at every site with the logarithms of the traces accumulated - real or complex
models, the label site anywhere.

    l_c(i) = sum over s_j, j missing, of | < (x)_{j known} phi[i][j] (x)_{j missing} e_{s_j} | W_c > |^2

with W_c the label slice of the model as stored; a known site is projected with conj(phi) (contract_mps), a missing one is summed
over its physical index.  ``dense_log_marginal`` is the same number from the full d^T amplitude tensor (tiny chains only) and
``naive_log_marginal`` the unscaled product in np.longdouble, whose exponent range keeps a thousand sites in range."""
import numpy as np


def normalised_chain(T, d, chi, C, rng, cx=False):
    """A random MPS of unit norm with the label on the last site, for chains of any length: every site but the last is the Q
    factor of a Gaussian tensor (left-orthonormal, the R factor is dropped instead of being carried along, which overflows
    fp64 near T = 400), the last one a Gaussian tensor of unit Frobenius norm."""
    dims = [1] + [int(min(chi, d ** min(j, T - j, 30))) for j in range(1, T)] + [1]
    W = []
    for j in range(T):
        shape = (dims[j], d, dims[j + 1]) + ((C,) if j == T - 1 else ())
        t = rng.standard_normal(shape)
        if cx:
            t = t + 1j * rng.standard_normal(shape)
        if j < T - 1:
            q = np.linalg.qr(t.reshape(dims[j] * d, dims[j + 1]))[0]
            assert q.shape[1] == dims[j + 1]
            t = q.reshape(shape)
        else:
            t = t / np.linalg.norm(t)
        W.append(t)
    return W


def gaussian_chain(T, d, chi, C, label_site, cx, rng, scale=1.0):
    """Gaussian site tensors (Dl, d, Dr), the label site (Dl, d, Dr, C) anywhere; bond dimensions capped by d^j at the ends."""
    dims = [1] + [min(chi, d ** min(j, T - j)) for j in range(1, T)] + [1]
    W = []
    for j in range(T):
        shape = (dims[j], d, dims[j + 1]) + ((C,) if j == label_site else ())
        t = rng.standard_normal(shape)
        if cx:
            t = t + 1j * rng.standard_normal(shape)
        W.append(scale * t)
    return W


def random_states(N, T, d, cx, rng):
    phi = rng.standard_normal((N, T, d))
    if cx:
        phi = phi + 1j * rng.standard_normal((N, T, d))
    return phi / np.linalg.norm(phi, axis=2, keepdims=True)


def label_site_of(W):
    ls = [j for j, t in enumerate(W) if t.ndim == 4]
    assert len(ls) == 1
    return ls[0]


def class_slice(W, c):
    return [t[..., c] if t.ndim == 4 else t for t in W]


def _step(E, A, phi_j, missing):
    """E'_{cd} = sum_s sum_ab A[a,s,c] E[a,b] conj(A[b,s,d]) (missing) or the same with s projected on conj(phi_j) (known)"""
    if missing:
        return np.einsum("ab,asc,bsd->cd", E, A, np.conj(A))
    M = np.einsum("s,asb->ab", np.conj(phi_j), A)
    return M.T @ E @ np.conj(M)


def log_marginals_ref(W, phi, missing=None):
    """(N, C) ln l_c(i); -inf where a trace vanishes.  phi (N, T, d) is not read where missing (N, T) is set."""
    T, N = len(W), phi.shape[0]
    C = W[label_site_of(W)].shape[3]
    miss = np.zeros((N, T), dtype=bool) if missing is None else np.asarray(missing).astype(bool)
    out = np.zeros((N, C))
    for c in range(C):
        Wc = class_slice(W, c)
        for i in range(N):
            E = np.ones((1, 1), dtype=Wc[0].dtype)
            lg = 0.0
            for j in range(T):
                E = _step(E, Wc[j], None if miss[i, j] else phi[i, j], miss[i, j])
                tr = float(np.trace(E).real)
                if not tr > 0.0:
                    lg = -np.inf
                    break
                lg += np.log(tr)
                E = E / tr
            out[i, c] = lg
    return out


def dense_log_marginal(W, phi_i, missing_i, c):
    """ln l_c of one instance from the full amplitude tensor psi[s_1 ... s_T] (d^T numbers): project, square, sum."""
    Wc = class_slice(W, c)
    psi = Wc[0][0]                                            # (d, D)
    for t in Wc[1:]:
        psi = np.tensordot(psi, t, axes=([psi.ndim - 1], [0]))
    psi = psi[..., 0]                                         # (d,) * T
    ax = 0
    for j in range(len(Wc)):
        if missing_i[j]:
            ax += 1
        else:
            psi = np.tensordot(psi, np.conj(phi_i[j]), axes=([ax], [0]))
    l = float(np.sum(np.abs(psi) ** 2))
    return np.log(l) if l > 0.0 else -np.inf


def naive_log_marginal(W, phi_i, missing_i, c):
    """ln l_c of one instance from the UNSCALED recursion in np.longdouble (complex: np.clongdouble)."""
    Wc = class_slice(W, c)
    cx = any(np.iscomplexobj(t) for t in Wc) or np.iscomplexobj(phi_i)
    dt = np.clongdouble if cx else np.longdouble
    E = np.ones((1, 1), dtype=dt)
    for j, t in enumerate(Wc):
        E = _step(E, t.astype(dt), None if missing_i[j] else phi_i[j].astype(dt), missing_i[j])
    return float(np.log(E[0, 0].real))
