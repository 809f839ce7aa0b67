"""NumPy restatement of the model overlaps (mpst_model_overlaps): for two chains A, B with the label at site p,

    L_0 = [1],  L_{j+1}[ra, rb] = sum_{la, lb, s} conj(A_j[la, s, ra]) L_j[la, lb] B_j[lb, s, rb]      (j < p),
    R the same from the right end down to p + 1,
    G[c, c'] = sum L[la, lb] conj(A_p[la, s, ra, c]) B_p[lb, s, rb, c'] R[ra, rb] = <psi_{a,c} | psi_{b,c'}>,

with L and R divided by their Frobenius norm at every site and the logarithms of the norms accumulated: G = g exp(lg).  The same walk
runs in np.longdouble (``dtype=np.longdouble``), ``overlap_brute`` contracts every class slice to its dense state and calls np.vdot
(tiny chains only), and ``embed`` makes a noisy copy of a chain in larger bonds."""
import numpy as np

from tests.marginal_ref import class_slice, label_site_of


def _is_complex(*chains):
    return any(np.iscomplexobj(t) for W in chains for t in W)


def overlap_ref(A, B, dtype=np.float64):
    """(g (Ca, Cb), lg): G = g exp(lg), conjugate on A.  dtype: np.float64 or np.longdouble (complex chains: their complex type).
    A zero environment gives (zeros, -inf)."""
    T, p = len(A), label_site_of(A)
    assert len(B) == T and label_site_of(B) == p
    cx = _is_complex(A, B)
    dt = {np.float64: np.complex128, np.longdouble: np.clongdouble}[dtype] if cx else dtype
    A, B = [np.asarray(t).astype(dt) for t in A], [np.asarray(t).astype(dt) for t in B]
    lg = dtype(0.0)
    zero = (np.zeros((A[p].shape[3], B[p].shape[3]), dtype=dt), -np.inf)

    def scaled(E):
        n = np.sqrt(np.sum(np.abs(E) ** 2))
        return (E / n, np.log(n)) if n > 0 else (None, None)

    L = np.ones((1, 1), dtype=dt)
    for j in range(p):
        X = np.tensordot(L, B[j], axes=(1, 0))                                  # (la, s, rb)
        L, s = scaled(np.tensordot(np.conj(A[j]), X, axes=([0, 1], [0, 1])))    # (ra, rb)
        if L is None:
            return zero
        lg += s
    R = np.ones((1, 1), dtype=dt)
    for j in range(T - 1, p, -1):
        X = np.tensordot(B[j], R, axes=(2, 1))                                  # (lb, s, ra)
        R, s = scaled(np.tensordot(np.conj(A[j]), X, axes=([1, 2], [1, 2])))    # (la, lb)
        if R is None:
            return zero
        lg += s
    X = np.tensordot(L, B[p], axes=(1, 0))                                      # (la, s, rb, c')
    X = np.tensordot(X, R, axes=(2, 1))                                         # (la, s, c', ra)
    G = np.tensordot(np.conj(A[p]), X, axes=([0, 1, 2], [0, 1, 3]))             # (c, c')
    return G, lg


def normalised_ref(models, pairs=None, dtype=np.float64):
    """(log_norm: K arrays ln ||psi_{k,c}||, {(a, b): normalised block G_ab / (||.|| ||.||)}) of the pairs asked for (None: every a <= b),
    formed in the log domain.  Zero states have log_norm -inf and NaN rows."""
    K = len(models)
    pairs = [(a, b) for a in range(K) for b in range(a, K)] if pairs is None else [tuple(q) for q in pairs]
    log_norm = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for W in models:
            g, lg = overlap_ref(W, W, dtype)
            log_norm.append(0.5 * (np.log(np.abs(np.diagonal(g).real)) + lg))
        blocks = {}
        for a, b in pairs:
            g, lg = overlap_ref(models[a], models[b], dtype)
            mag = np.abs(g)
            val = np.where(mag > 0, g / np.where(mag > 0, mag, 1), 0) * np.exp(np.log(mag) + lg - log_norm[a][:, None] - log_norm[b][None, :])
            val = np.where(mag > 0, val, 0)
            blocks[(a, b)] = np.where(np.isneginf(log_norm[a])[:, None] | np.isneginf(log_norm[b])[None, :], np.nan, val)
    return log_norm, blocks


def dense_state(W, c):
    """psi[s_1 ... s_T] of class slice c (d^T numbers)."""
    Wc = class_slice(W, c)
    psi = Wc[0][0]
    for t in Wc[1:]:
        psi = np.tensordot(psi, t, axes=([psi.ndim - 1], [0]))
    return psi[..., 0]


def overlap_brute(A, B):
    """G (Ca, Cb) from the dense states: np.vdot conjugates its first argument."""
    Ca, Cb = A[label_site_of(A)].shape[3], B[label_site_of(B)].shape[3]
    sa, sb = [dense_state(A, c) for c in range(Ca)], [dense_state(B, c) for c in range(Cb)]
    return np.array([[np.vdot(x, y) for y in sb] for x in sa])


def embed(W, chi2, eps, rng):
    """The chain W zero-padded into bonds min(chi2, d^j, d^(T-j)) (at least its own), with eps * mean|t| * Gaussian noise added to every
    element of every padded tensor (mean|t| of the tensor before padding; complex chains: complex noise of unit variance, real and imaginary parts alike)."""
    T, d = len(W), W[0].shape[1]
    dims = [1] + [max(W[j].shape[0], min(chi2, d ** min(j, T - j))) for j in range(1, T)] + [1]
    out = []
    for j, t in enumerate(W):
        shape = (dims[j], d, dims[j + 1]) + t.shape[3:]
        big = np.zeros(shape, dtype=t.dtype)
        big[:t.shape[0], :, :t.shape[2]] = t
        noise = rng.standard_normal(shape)
        if np.iscomplexobj(t):
            noise = (noise + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
        out.append(big + eps * np.abs(t).mean() * noise)
    return out


# The device cases (tests/test_gpu_overlap.py) and the float64-against-long-double check of this restatement (tests/test_overlap_ref.py):
# chi / chi2, T, d, C, label site, eps, and why
CASES = {
    "chi12_last": dict(chi=12, chi2=12, T=10, d=6, C=3, label=9, eps=0.3),       # not a tile multiple; left walk only
    "chi7_mid": dict(chi=7, chi2=12, T=10, d=6, C=3, label=5, eps=0.3),          # below one tile, rectangular L, both walks
    "chi12_first": dict(chi=12, chi2=20, T=10, d=5, C=3, label=0, eps=0.2),      # right walk only; d not a multiple of 4
    "chi40_scratch": dict(chi=40, chi2=72, T=6, d=6, C=2, label=3, eps=0.2),     # beyond the LDS path: global scratch
    "long_last": dict(chi=8, chi2=8, T=1000, d=3, C=2, label=999, eps=0.02),     # the scale accumulator
    "long_mid": dict(chi=8, chi2=8, T=1000, d=3, C=2, label=500, eps=0.02),
}


def case_models(name, cx):
    """[a, b, c] of a case: a Gaussian chain at chi, its noisy embedding at chi2, an independent chain at chi2."""
    from tests.marginal_ref import gaussian_chain
    k = CASES[name]
    rng = np.random.default_rng([sorted(CASES).index(name), int(cx), 5])
    a = gaussian_chain(k["T"], k["d"], k["chi"], k["C"], k["label"], cx, rng, scale=1.0 / np.sqrt(k["d"] * k["chi"]))
    b = embed(a, k["chi2"], k["eps"], rng)
    c = gaussian_chain(k["T"], k["d"], k["chi2"], k["C"], k["label"], cx, rng, scale=1.0 / np.sqrt(k["d"] * k["chi2"]))
    return [a, b, c]
