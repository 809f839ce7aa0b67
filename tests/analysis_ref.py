"""NumPy restatement of the reference's analysis module (src/Analysis/analyse.jl), function for function: the yardstick
of the device's bipartite_spectrum / single_site_spectrum / see_variation.  It works as the reference does - an MPS with an
orthogonality centre that orthogonalize! moves by QR, an SVD per cut for the BEE, eigh + rho_correct per one-site RDM,
precondition + normalize! for every (instance, k) - not as the device does.

Site tensors are (Dl, d, Dr); the label site of a trained model is (Dl, d, Dr, C)."""
from __future__ import annotations

import numpy as np

EIGTOL = float(np.sqrt(np.finfo(np.float64).eps))      # sqrt(eps())


class DomainError(ValueError):
    pass


class MPS:
    """Site tensors plus the ITensors orthogonality limits: sites < llim are left-orthonormal, sites > rlim right-orthonormal."""

    def __init__(self, tensors):
        self.t = [np.array(a, dtype=np.float64) for a in tensors]
        self.llim, self.rlim = -1, len(self.t)

    def __len__(self):
        return len(self.t)

    def copy(self):
        m = MPS(self.t)
        m.llim, m.rlim = self.llim, self.rlim
        return m

    def orthogonalize(self, j):
        """orthogonalize!(mps, j): QR left of j, LQ right of j, only where the current limits require it."""
        while self.llim < j - 1:
            i = self.llim + 1
            Dl, d, Dr = self.t[i].shape
            q, r = np.linalg.qr(self.t[i].reshape(Dl * d, Dr))
            self.t[i] = q.reshape(Dl, d, q.shape[1])
            self.t[i + 1] = np.einsum("ab,bsr->asr", r, self.t[i + 1])
            self.llim = i
        while self.rlim > j + 1:
            i = self.rlim - 1
            Dl, d, Dr = self.t[i].shape
            q, r = np.linalg.qr(self.t[i].reshape(Dl, d * Dr).T)
            self.t[i] = q.T.reshape(q.shape[1], d, Dr)
            self.t[i - 1] = np.einsum("lsa,ba->lsb", self.t[i - 1], r)
            self.rlim = i
        self.llim, self.rlim = min(self.llim, j - 1), max(self.rlim, j + 1)

    def norm(self):
        E = np.ones((1, 1))
        for a in self.t:
            E = np.einsum("ab,asr,bst->rt", E, a, a)
        return float(np.sqrt(E[0, 0]))

    def normalize(self):
        """normalize!: the whole state scaled to norm 1.  The norm is read off an orthogonality centre (as ITensors' lognorm
        does): a transfer-matrix contraction in a badly conditioned gauge would lose digits."""
        if self.rlim - self.llim != 2:
            self.orthogonalize(0)
        c = self.llim + 1
        self.t[c] = self.t[c] / np.linalg.norm(self.t[c])
        return self


def label_site(W):
    ls = [j for j, a in enumerate(W) if np.ndim(a) == 4]
    assert len(ls) == 1
    return ls[0]


def expand_label_index(W):
    """utils.jl:356-370: one normalised MPS per class (the label index fixed by a one-hot vector)."""
    pos = label_site(W)
    out = []
    for c in range(W[pos].shape[3]):
        t = [np.asarray(a, dtype=np.float64) for a in W]
        t[pos] = t[pos][..., c]
        out.append(MPS(t).normalize())
    return out


def von_neumann_entropy(mps: MPS, logfn=np.log):
    """analyse.jl:20-45."""
    if logfn not in (np.log, np.log2, np.log10):
        raise ValueError("logfn must be one of: log, log2, or log10")
    mps = mps.copy()
    N = len(mps)
    entropy = np.zeros(N)
    for i in range(N):
        mps.orthogonalize(i)
        a = mps.t[i]
        Dl, d, Dr = a.shape
        if i == 0:
            S = np.linalg.svd(a.reshape(d, Dr), compute_uv=False)            # svd(mps[1], siteind(1))
        elif i == N - 1:
            S = np.linalg.svd(a.reshape(Dl, d).T, compute_uv=False)          # svd(mps[N], siteind(N)): bond N-1 again
        else:
            S = np.linalg.svd(a.reshape(Dl * d, Dr), compute_uv=False)       # svd(mps[i], (link(i-1), site(i)))
        SvN = 0.0
        for s in S:
            p = s * s
            if p > 1e-12:
                SvN += -p * logfn(p)
        entropy[i] = SvN
    return entropy


def bipartite_spectrum(W, logfn=np.log):
    """analyse.jl:47-64."""
    if logfn not in (np.log, np.log2, np.log10):
        raise ValueError("logfn must be one of: log, log2, or log10")
    return [von_neumann_entropy(m, logfn) for m in expand_label_index(W)]


def rho_correct(rho, eigentol=EIGTOL):
    """analyse.jl:69-91."""
    eigvals, eigvecs = np.linalg.eigh(rho)
    if not np.any(eigvals < 0):
        return rho
    oot = eigvals[eigvals < -eigentol]
    if oot.size:
        raise DomainError(f"RDM contains large negative eigenvalues outside of the tolerance {eigentol}: λ = {oot}")
    clamped = np.clip(eigvals, eigentol, np.inf)
    rc = eigvecs @ np.diag(clamped) @ eigvecs.T
    if not abs(np.trace(rc) - 1.0) <= 0.01:
        raise DomainError(f"Tr(ρ_corrected) > 1.0! ({np.trace(rc)})")
    return rc


def one_site_rdm(mps: MPS, site: int, mins=None):
    """analyse.jl:102-109 (mps is moved in place, as orthogonalize! does).  ``mins``: a list that collects the smallest
    |eigenvalue| of every raw RDM - where it is within rounding of zero, whether rho_correct clamps depends on its sign."""
    mps.orthogonalize(site)
    a = mps.t[site]
    rho = np.einsum("lsr,ltr->st", a, a)
    if mins is not None:
        mins.append(float(np.min(np.abs(np.linalg.eigvalsh(rho)))) if np.all(np.isfinite(rho)) else np.nan)
    return rho_correct(rho)


def entropy_of(rho):
    """-tr(rho log rho) on the eigenvalues; an exact 0 contributes 0 (the reference's matrix log would give NaN)."""
    lam = np.linalg.eigvalsh(rho)
    return float(-sum(l * np.log(l) for l in lam if l > 0.0)) if not np.isnan(lam).any() else np.nan


def single_site_entropy(mps: MPS, mins=None):
    """analyse.jl:111-120."""
    mps = mps.copy()
    return np.array([entropy_of(one_site_rdm(mps, i, mins)) for i in range(len(mps))])


def single_site_spectrum(W, mins=None):
    """analyse.jl:122-138.  ``mins``: a list that receives one array of smallest |eigenvalue| per class."""
    out = []
    for m in expand_label_index(W):
        mm = []
        out.append(single_site_entropy(m, mm))
        if mins is not None:
            mins.append(np.array(mm))
    return out


def precondition(mps: MPS, phi, k):
    """Imputation/MPS_methods.jl:42-99 with the known sites 0..k-1: their projections contracted into site k."""
    v = np.ones(1)
    for i in range(k):
        v = v @ np.einsum("lsr,s->lr", mps.t[i], phi[i])
    first = np.einsum("l,lsr->sr", v, mps.t[k])[None]
    return MPS([first] + [a.copy() for a in mps.t[k + 1:]])


def see_variation_encoded(class_mps: MPS, phi, return_mins=False):
    """analyse.jl:168-194 on encoded series phi (n, T, d): out[i, k, site] (and, with ``return_mins``, the smallest
    |eigenvalue| of every raw RDM in the same layout, +inf where nothing was computed)."""
    T = len(class_mps)
    bm = []
    base = single_site_entropy(class_mps, bm)
    out = np.zeros((phi.shape[0], T, T))
    mins = np.full((phi.shape[0], T, T), np.inf)
    for i in range(phi.shape[0]):
        out[i, 0] = base
        mins[i, 0] = bm
        for k in range(1, T):
            c = precondition(class_mps, phi[i], k)
            with np.errstate(invalid="ignore", divide="ignore"):
                c.normalize()
            if not np.all(np.isfinite(c.t[0])):
                out[i, k, k:] = np.nan
                continue
            mm = []
            out[i, k, k:] = single_site_entropy(c, mm)
            mins[i, k, k:] = mm
    return (out, mins) if return_mins else out


def tolerance(mins, d, atol):
    """Where the smallest eigenvalue of the restatement's RDM is within 1e-13 of zero, the clamp branch of rho_correct depends
    on the sign of rounding noise (a clamped eigenvalue adds about 2.7e-7 to the entropy): allow d * 3e-7 there."""
    return np.where(np.asarray(mins) < 1e-13, d * 3e-7, atol)
