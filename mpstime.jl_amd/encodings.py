"""Host-side input producers of the sweep: preprocessing and encodings.

Mirrors src/utils.jl:161-295 (RobustSigmoid + MinMax) and src/Encodings (encode_dataset,
Encodings/encodings.jl:33-156; bases, Encodings/bases.jl).  These run once per fit on the
host in the reference as well.  Encodings whose basis differs from site to site (Encodings/splitbases.jl,
basis_structs.jl) are fitted once by ``fit_encoding`` and applied through the encoder it returns; so are the Sahand-Legendre
bases (``sahand_legendre``), fitted to a kernel density estimate of the training values, and the projected bases
(``legendre(project=True)``, ``fourier(project=True)``), which pick every site's members of the closed-form family from such an estimate.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from .options import MPSOptions, encoding_info


# ---------------------------------------------------------------------------------------
# containers (src/Structs/structs.jl:12-33)
# ---------------------------------------------------------------------------------------
@dataclass
class EncodedTimeSeriesSet:
    """timeseries (as one array), original_data, class_distribution - structs.jl:27-33.
    ``phi[i, t, :]`` is PState i's pstate[t]; ``labels``/``label_index`` are PState.label /
    PState.label_index (0-based here)."""

    phi: np.ndarray
    labels: np.ndarray
    label_index: np.ndarray
    original_data: np.ndarray
    class_distribution: np.ndarray

    def __len__(self):
        return 0 if self.phi.ndim != 3 else self.phi.shape[0]

    @staticmethod
    def empty():
        return EncodedTimeSeriesSet(np.zeros((0, 0, 0)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                    np.zeros((0, 0)), np.zeros(0, dtype=np.int64))

    def isempty(self):
        return len(self) == 0


# ---------------------------------------------------------------------------------------
# bases (src/Encodings/bases.jl)
# ---------------------------------------------------------------------------------------
def _legendre_table(x, d):
    """P_0..P_{d-1} by Bonnet recursion, scaled to sqrt((2k+1)/2) P_k - LegendrePolynomials'
    Pl(x, k; norm=Val(:normalized)) as used at bases.jl:77-79."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape + (d,))
    p0 = np.ones_like(x)
    out[..., 0] = p0
    if d > 1:
        p1 = x.copy()
        out[..., 1] = p1
        for k in range(1, d - 1):
            p2 = ((2 * k + 1) * x * p1 - k * p0) / (k + 1)
            out[..., k + 1] = p2
            p0, p1 = p1, p2
    out *= np.sqrt((2.0 * np.arange(d) + 1.0) / 2.0)
    return out


def legendre_encode(x, d, norm=True):
    """bases.jl:81-92.  norm=True divides by sqrt(Pl(1,d;normalized)*d) (:86-89)."""
    ls = _legendre_table(x, d)
    if norm:
        ls = ls / math.sqrt(math.sqrt((2 * d + 1) / 2.0) * d)
    return ls


def legendre_encode_no_norm(x, d):
    """bases.jl:108."""
    return legendre_encode(x, d, norm=False)


def get_fourier_freqs(d):
    """bases.jl:27-34: 0, 1, -1, 2, -2, ... truncated to d terms."""
    hb = math.ceil((d - 1.0) / 2.0)
    fr = [0]
    for i in range(1, hb + 1):
        fr += [i, -i]
    return fr[:d]


def fourier_encode(x, d):
    """bases.jl:23-42: cispi(k x)/sqrt(d)."""
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(get_fourier_freqs(d), dtype=np.float64)
    return np.exp(1j * np.pi * x[..., None] * k) / math.sqrt(d)


def angle_encode(x, d=2, periods=0.25):
    """Stoudenmire angle encoding, bases.jl:7-21 (d must be 2)."""
    if d != 2:
        raise ValueError("Stoudenmire Angle encoding only supports d = 2!")
    x = np.asarray(x, dtype=np.float64)
    s1 = np.exp(1j * np.pi * 1.5 * x) * np.cos(np.pi * 2 * periods * x)
    s2 = np.exp(-1j * np.pi * 1.5 * x) * np.sin(np.pi * 2 * periods * x)
    return np.stack([s1, s2], axis=-1)


def sahand_encode(x, d):
    """bases.jl:45-68."""
    if d % 2:
        raise ValueError("Sahand encoding only supports even dimension")
    x = np.asarray(x, dtype=np.float64)
    dx = 2.0 / d
    out = np.zeros(x.shape + (d,), dtype=np.complex128)
    for i in range(1, d + 1):
        interval = math.ceil(i / 2)
        startx = (interval - 1) * dx
        inside = (startx <= x) & (x <= interval * dx)
        if i % 2:
            s = np.exp(1j * np.pi * 1.5 * x / dx) * np.cos(np.pi * 0.5 * (x - startx) / dx)
        else:
            s = np.exp(-1j * np.pi * 1.5 * x / dx) * np.sin(np.pi * 0.5 * (x - startx) / dx)
        out[..., i - 1] = np.where(inside, s, 0.0)
    return out


def uniform_encode(x, d):
    """bases.jl:2-4."""
    x = np.asarray(x, dtype=np.float64)
    return np.full(x.shape + (d,), 1.0 / d)


def no_init(X_norm=None, y=None, opts=None, range=None):
    """no_init (bases.jl): a closed-form basis has no arguments to fit."""
    return []


@dataclass(frozen=True)
class Encoding:
    """Basis / SplitBasis (src/Encodings/basis_structs.jl:49-92): name, complex flag, input range, encode and - for bases
    that are fitted to the training data or differ from site to site - init and the two flags.

    ``encode(x, d, *init_args)`` takes an array of values of any shape and returns shape + (d,); a time-dependent basis is
    called as ``encode(x, d, ti, *init_args)`` with ``ti`` the site COUNTED FROM 0 (the reference's ``j`` of encode_TS,
    encodings.jl:18-24, counts from 1).  ``init(X_norm, y, opts=opts)`` returns ``init_args``; X_norm is the (N, T)
    training matrix in the encoding's range, rows = series (the reference passes its transpose)."""

    name: str
    iscomplex: bool
    range: tuple
    encode: object = None
    istimedependent: bool = False
    isdatadriven: bool = False
    init: object = None                 # None: no_init
    splitmethod: object = None          # SplitBasis only
    aux_enc: object = None              # SplitBasis only


_CLOSED_FORM = ("Legendre_No_Norm", "Legendre_Norm", "Fourier", "Stoudenmire", "Sahand", "Uniform")


# ---------------------------------------------------------------------------------------
# split bases (src/Encodings/splitbases.jl)
# ---------------------------------------------------------------------------------------
def get_nbins_safely(opts) -> int:
    """splitbases.jl:2-9."""
    if opts.d % opts.aux_basis_dim != 0:
        raise ValueError(f"The auxilliary basis dimension ({opts.aux_basis_dim}) must evenly divide the total feature "
                         f"dimension ({opts.d})")
    return opts.d // opts.aux_basis_dim


def unif_split(data, nbins, a, b):
    """splitbases.jl:51-54: ``collect(a:dx:b)`` with dx = (b - a) / nbins.  Julia builds a float range from the
    rationals behind its end points (twice-precision arithmetic), so edge i is the double nearest to a + i (b - a) / nbins
    and the last one is b: restated with exact fractions."""
    fa, fb = Fraction(float(a)), Fraction(float(b))
    return np.array([float(fa + (fb - fa) * i / nbins) for i in range(nbins + 1)])


def hist_split(samples, nbins, a, b):
    """splitbases.jl:56-92.  A vector: the bin edges that put round(npts / nbins) of the sorted samples inside [a, b]
    into every bin; a matrix (N, T): one edge list per time point, (T, nbins + 1)."""
    samples = np.asarray(samples, dtype=np.float64)
    if samples.ndim == 2:                                                      # :90-92 (columns here: rows = series)
        return np.stack([hist_split(samples[:, t], nbins, a, b) for t in range(samples.shape[1])])
    npts = len(samples)
    bin_pts = int(round(npts / nbins))                                         # round half to even, as Julia's
    if bin_pts == 0:
        warnings.warn("Less than one data point per bin! Putting the extra bins at x=1 and hoping for the best")
        bin_pts = 1
    bins = np.full(nbins + 1, float(a))
    ds = np.sort(samples[(a <= samples) & (samples <= b)])                     # :69
    # every bin_pts-th sorted sample (1-based i, i < npts) closes a bin until nbins - 1 interior edges are set (:70-80)
    take = [i for i in range(bin_pts, len(ds) + 1, bin_pts) if i < npts][:nbins - 1]
    for j, i in enumerate(take, start=1):
        if i >= len(ds):                                                       # ds[i+1] of :77 is past the end
            raise IndexError(f"hist_split: sample {i + 1} of {len(ds)} inside [{a}, {b}]")
        bins[j] = (ds[i - 1] + ds[i]) / 2
    if len(take) + 2 <= nbins:                                                 # :81-84 (j <= nbins)
        bins[bins == a] = b
        bins[0] = a
    bins[-1] = b
    return bins


def rect(x, lbound=0.5, rbound=0.5):
    """splitbases.jl:96-108, elementwise: lbound at -0.5, rbound at 0.5, 1 inside, 0 outside (and for NaN)."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x == -0.5, lbound, np.where(x == 0.5, rbound, np.where((-0.5 <= x) & (x <= 0.5), 1.0, 0.0)))


def _project(x, aux_dim, aux_encoder, bins, iscomplex, norm=True):
    """project_onto_bins(x, aux_dim, aux_encoder, bins) (splitbases.jl:113-132) for an array of values: the auxiliary
    encoder is evaluated in the selected bin(s) only, at a + scale (x - bins[i]) / dx."""
    x = np.asarray(x, dtype=np.float64)
    bins = np.asarray(bins, dtype=np.float64)
    widths = np.diff(bins)
    a, b = bins[0], bins[-1]
    scale = b - a
    nb = len(widths)
    out = np.zeros(x.shape + (nb * aux_dim,), dtype=np.complex128 if iscomplex else np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):                       # an empty bin (dx = 0) selects nothing
        for i in range(nb):
            dx = widths[i]
            y = 1.0 if norm else 1.0 / dx
            x_prop = scale * (x - bins[i]) / dx
            select = y * rect(x_prop / scale - 0.5, 1.0 if i == 0 else 0.5, 1.0 if i == nb - 1 else 0.5)
            hit = select != 0
            if hit.any():
                out[hit, i * aux_dim:(i + 1) * aux_dim] = select[hit][:, None] * aux_encoder(a + x_prop[hit], i)
    return out


def project_onto_bins(x, d, aux_enc_args, split_args, norm=True):
    """splitbases.jl:135-142: the time-independent form, one edge list for all sites."""
    bins, aux_dim, aux_enc = split_args
    return _project(x, aux_dim, lambda xx, i: aux_enc.encode(xx, aux_dim, *aux_enc_args[i]), bins, aux_enc.iscomplex, norm)


def project_onto_bins_td(x, d, ti, all_aux_enc_args, split_args, norm=True):
    """splitbases.jl:144-163: the time-dependent form; ``ti`` (from 0) picks the site's edge list when there is one per site.
    (The auxiliary basis is never time-dependent here: the SplitBasis constructor refuses it.)"""
    all_bins, aux_dim, aux_enc = split_args
    bins = all_bins[ti] if np.ndim(all_bins) == 2 else all_bins
    return _project(x, aux_dim, lambda xx, i: aux_enc.encode(xx, aux_dim, *all_aux_enc_args[i]), bins, aux_enc.iscomplex, norm)


def split_init(X_norm, y, opts, range=None):
    """splitbases.jl:12-48: [aux_enc_args, [bins, aux_dim, aux_enc]]."""
    enc = opts_encoding(opts)
    nbins = get_nbins_safely(opts)
    a, b = enc.range if range is None else range
    bins = enc.splitmethod(np.asarray(X_norm, dtype=np.float64), nbins, a, b)
    aux = enc.aux_enc
    if aux.aux_enc is not None:
        raise NotImplementedError("nested split bases are not implemented")
    enc_arg = [] if aux.init is None else aux.init(X_norm, y, opts=opts.set(d=opts.aux_basis_dim))       # :30, :42
    return [[enc_arg] * nbins, [bins, int(opts.aux_basis_dim), aux]]


def SplitBasis(name, init, splitmethod, aux_enc, encode, iscomplex, istimedependent, isdatadriven, range) -> Encoding:
    """The SplitBasis constructor's consistency checks (basis_structs.jl:75-91), same texts."""
    if aux_enc.iscomplex != iscomplex:
        raise ValueError("The SplitBasis and its auxilliary basis must agree on whether they are complex!")
    if tuple(aux_enc.range) != tuple(range):
        raise ValueError("The SplitBasis and its auxilliary basis must agree on the normalised timeseries range!")
    if aux_enc.isdatadriven or aux_enc.istimedependent:
        raise ValueError("Splitting up a data-driven encoding is not yet supported, sorry")
    if aux_enc.aux_enc is not None:
        raise NotImplementedError("nested split bases are not implemented")
    return Encoding(name, iscomplex, tuple(range), encode, istimedependent, isdatadriven, init, splitmethod, aux_enc)


def _aux(enc_or_name) -> Encoding:
    return enc_or_name if isinstance(enc_or_name, Encoding) else model_encoding(enc_or_name)


def histogram_split(enc_or_name="uniform") -> Encoding:
    """histogram_split (basis_structs.jl:247-260, :278): per-site bins holding equal shares of the training values."""
    aux = _aux(enc_or_name)
    return SplitBasis(f"Hist Split {aux.name}", split_init, hist_split, aux, project_onto_bins_td, aux.iscomplex, True, True, aux.range)


def uniform_split(enc_or_name="uniform") -> Encoding:
    """uniform_split (basis_structs.jl:262-276, :279): equal-width bins, time-independent over a closed-form basis."""
    aux = _aux(enc_or_name)
    return SplitBasis(f"Unif Split {aux.name}", split_init, unif_split, aux, project_onto_bins, aux.iscomplex, aux.istimedependent,
                      aux.isdatadriven, aux.range)


def function_basis(fn, is_complex, range, is_time_dependent=False, is_data_driven=False, init=None, name="Custom") -> Encoding:
    """function_basis (basis_structs.jl:235-244).  ``fn(x, d, *init_args)`` - or, with ``is_time_dependent``,
    ``fn(x, d, ti, *init_args)`` - takes ONE value and returns its d coefficients.  ``ti`` counts sites from 0 here; the
    reference passes Julia's 1-based index, so a function ported from Julia uses ``ti + 1`` where it used ``ti``."""
    dt = np.complex128 if is_complex else np.float64

    def encode(x, d, *args):
        x = np.asarray(x, dtype=np.float64)
        out = np.empty((x.size, d), dtype=dt)
        for k, v in enumerate(x.ravel().tolist()):
            out[k] = fn(v, d, *args)
        return out.reshape(x.shape + (d,))

    return Encoding(name, bool(is_complex), tuple(range), encode, bool(is_time_dependent), bool(is_data_driven), init)


# ---------------------------------------------------------------------------------------
# Sahand-Legendre bases (bases.jl:111-129, :158-206, :269-342): polynomials orthonormalised under the square root of a kernel
# density estimate of the training values - one estimate per site (time dependent) or one for all values
# ---------------------------------------------------------------------------------------
KDE_NPOINTS = 2048


@dataclass
class UnivariateKDE:
    """KernelDensity.jl's default univariate estimate (Normal kernel) as ``kde_pdf`` needs it: the grid starts at ``lo`` with spacing
    ``step``, ``h`` is the bandwidth, ``coef`` the K + 2 coefficients of the quadratic B-spline through the K grid values."""

    lo: float
    step: float
    h: float
    coef: np.ndarray

    @property
    def npoints(self):
        return len(self.coef) - 2

    @property
    def hi(self):
        return self.lo + (self.npoints - 1) * self.step


_THOMAS = {}


def _thomas_factors(m):
    """the site-independent half of the Thomas algorithm for the m x m matrix tridiag(1/8, 3/4, 1/8): (c', 1 / pivot)"""
    if m not in _THOMAS:
        cp, inv = np.empty(m), np.empty(m)
        prev = 0.0
        for i in range(m):
            inv[i] = 1.0 / (0.75 - 0.125 * prev)
            prev = cp[i] = 0.125 * inv[i]
        _THOMAS[m] = (cp, inv)
    return _THOMAS[m]


def _spline_coefficients(dens):
    """Quadratic B-spline coefficients c[0..K+1] of the grid values dens (K, S), one column per estimate:
    c[i-1]/8 + 3c[i]/4 + c[i+1]/8 = dens[i] (i = 1..K) with zero second difference of c at either end.  The end conditions put
    c[1] = dens[1] and c[K] = dens[K]; what is left is tridiagonal with constant bands, solved for all columns at once."""
    K = dens.shape[0]
    c = np.empty((K + 2,) + dens.shape[1:])
    c[1], c[K] = dens[0], dens[K - 1]
    m = K - 2
    rhs = dens[1:K - 1].copy()
    rhs[0] -= 0.125 * c[1]
    rhs[m - 1] -= 0.125 * c[K]
    cp, inv = _thomas_factors(m)
    rhs[0] *= inv[0]
    for i in range(1, m):
        rhs[i] = (rhs[i] - 0.125 * rhs[i - 1]) * inv[i]
    for i in range(m - 2, -1, -1):
        rhs[i] -= cp[i] * rhs[i + 1]
    c[2:K] = rhs
    c[0] = 2.0 * c[1] - c[2]
    c[K + 1] = 2.0 * c[K] - c[K - 1]
    return c


def _kde_columns(X, inside, bandwidth=None, npoints=KDE_NPOINTS):
    """One density estimate per column of X (n, S) from the entries where ``inside``: (lo, step, h, coef (S, K + 2), n (S,)).
    A column without entries gets lo = 0, step = 1, h = 0 and zero coefficients."""
    X = np.asarray(X, dtype=np.float64)
    K = int(npoints)
    S = X.shape[1]
    n = inside.sum(axis=0)
    has = n > 0
    nn = np.maximum(n, 1)
    Xs = np.sort(np.where(inside, X, np.inf), axis=0)                          # entries first, in order
    Xz = np.where(inside, X, 0.0)
    cols = np.arange(S)
    if bandwidth is None:
        mean = Xz.sum(axis=0) / nn
        std = np.sqrt(np.where(inside, (X - mean) ** 2, 0.0).sum(axis=0) / np.maximum(n - 1, 1))

        def quantile(q):                                                       # type 7, the interpolation written as NumPy's
            pos = q * (nn - 1)
            lo_i = np.floor(pos).astype(np.int64)
            hi_i = np.minimum(lo_i + 1, nn - 1)
            t = pos - lo_i
            a_, b_ = np.where(has, Xs[lo_i, cols], 0.0), np.where(has, Xs[hi_i, cols], 0.0)
            dba = b_ - a_
            return np.where(a_ == b_, a_, np.where(t >= 0.5, b_ - dba * (1.0 - t), a_ + dba * t))

        w = np.minimum(std, (quantile(0.75) - quantile(0.25)) / 1.34)
        w = np.where(w == 0.0, np.where(std == 0.0, 1.0, std), w)
        h = np.where(n <= 1, 0.9, 0.9 * w * nn ** (-0.2))
    else:
        h = np.full(S, float(bandwidth))
    xmin = np.where(has, Xs[0], 0.0)
    xmax = np.where(has, Xs[np.maximum(n - 1, 0), cols], 0.0)
    lo, hi = xmin - 4.0 * h, xmax + 4.0 * h
    step = (hi - lo) / (K - 1)
    lo, step, h = np.where(has, lo, 0.0), np.where(has, step, 1.0), np.where(has, h, 0.0)
    # linear binning: k is the first grid index with grid[k] >= x (grid[k] = lo + k step), j = k - 1
    with np.errstate(invalid="ignore"):
        k = np.ceil((Xz - lo) / step).astype(np.int64)
    k -= (lo + (k - 1) * step) >= Xz
    k += (lo + k * step) < Xz
    ok = inside & (k >= 1) & (k <= K - 1)
    kk = np.where(ok, k, 1)
    scale = 1.0 / (nn * step * step)
    wj = np.where(ok, ((lo + kk * step) - Xz) * scale, 0.0)
    wk = np.where(ok, (Xz - (lo + (kk - 1) * step)) * scale, 0.0)
    flat = (cols * K + kk).ravel()
    cells = (np.bincount(flat - 1, weights=wj.ravel(), minlength=S * K) + np.bincount(flat, weights=wk.ravel(), minlength=S * K)).reshape(S, K)
    # the Normal kernel in Fourier space, coefficient m at omega_m = 2 pi m / (K step)
    omega = 2.0 * np.pi * np.arange(K // 2 + 1)[None, :] / (K * step[:, None])
    dens = np.fft.irfft(np.fft.rfft(cells, axis=1) * np.exp(-0.5 * (h[:, None] * omega) ** 2), n=K, axis=1)
    dens = np.where(has[:, None], np.maximum(dens, 0.0), 0.0)
    coef = np.ascontiguousarray(_spline_coefficients(np.ascontiguousarray(dens.T)).T)
    return lo, step, h, coef, n


def kde(xs, bandwidth=None, npoints=KDE_NPOINTS) -> UnivariateKDE:
    """kde(xs[; bandwidth]) of KernelDensity.jl with its defaults: Normal kernel, Silverman's bandwidth, ``npoints`` grid points
    from min - 4h to max + 4h, linear binning, the kernel applied in Fourier space, negative values clamped."""
    xs = np.asarray(xs, dtype=np.float64).reshape(-1, 1)
    lo, step, h, coef, _ = _kde_columns(xs, np.ones(xs.shape, dtype=bool), bandwidth, npoints)
    return UnivariateKDE(float(lo[0]), float(step[0]), float(h[0]), coef[0])


def _pdf_rows(lo, step, coef, x):
    """the spline of row r (lo[r], step[r], coef[r]) at x[r, :]: the interpolant inside [lo, lo + (K - 1) step], 0 outside"""
    K = coef.shape[1] - 2
    lo, step = lo[:, None], step[:, None]
    u = (x - lo) / step + 1.0
    i = np.where(np.isnan(u), 1.0, np.clip(np.rint(u), 1, K))                  # a NaN value reads index 1, as on the device, and stays NaN
    s = u - i
    i = i.astype(np.int64)
    take = lambda off: np.take_along_axis(coef, i + off, axis=1)
    val = take(-1) * (0.5 * (s - 0.5) ** 2) + take(0) * (0.75 - s ** 2) + take(1) * (0.5 * (s + 0.5) ** 2)
    return np.where((x < lo) | (x > lo + (K - 1) * step), 0.0, val)


def kde_pdf(k: UnivariateKDE, x):
    """pdf(kde, x) (KernelDensity.jl: the quadratic B-spline interpolant of the grid values, zero outside the grid); x of any shape"""
    x = np.asarray(x, dtype=np.float64)
    return _pdf_rows(np.array([k.lo]), np.array([k.step]), k.coef[None, :], x.reshape(1, -1)).reshape(x.shape)


def _trapezoid(y, x):
    return ((y[..., 1:] + y[..., :-1]) * 0.5 * np.diff(x)).sum(axis=-1)


def remove_zeros(xs_samps, f0):
    """remove_zeros! (bases.jl:269-291), in place on f0 (S,) or, row by row, (R, S): entries up to 1 % of the largest become the
    smallest entry above that, then f0 is divided by the trapezoid integral of its square - by the integral, not its root, as the
    reference does.  Returns (minval, norm); (0, 1) and f0 untouched where no entry is above the threshold."""
    rows = f0 if f0.ndim == 2 else f0[None, :]
    a = np.abs(rows)
    bad = a <= 0.01 * a.max(axis=1, keepdims=True)
    good = ~bad.all(axis=1)
    minval = np.where(good, np.where(bad, np.inf, a).min(axis=1), 0.0)
    np.copyto(rows, np.where(bad & good[:, None], minval[:, None], rows))
    norm = np.where(good, _trapezoid(rows * rows, xs_samps), 1.0)
    rows /= norm[:, None]
    return (minval, norm) if f0.ndim == 2 else (float(minval[0]), float(norm[0]))


def sahand_legendre_coeffs(xs_samp, f0, d):
    """sahand_legendre_coeffs (bases.jl:158-206) for f0 (S,) -> (d, d), or row by row (R, S) -> (R, d, d): row n holds the
    coefficients of function n, column i belongs to x^i.  Operation for operation - the n = 1 row takes c_1 = -1 / M[1][0]."""
    xs_samp = np.asarray(xs_samp, dtype=np.float64)
    rows = f0 if f0.ndim == 2 else f0[None, :]
    R = rows.shape[0]
    f2 = rows * rows
    mom = np.stack([_trapezoid(xs_samp ** p * f2, xs_samp) for p in range(2 * d - 1)], axis=1)      # (R, 2d - 1)
    M = mom[:, np.add.outer(np.arange(d), np.arange(d))]                                            # M[i][j] = moment i + j
    cv = np.zeros((R, d, d))
    cv[:, 0, 0] = 1.0
    for n in range(1, d):
        cv[:, n, 0] = 1.0
        if n == 1:
            cv[:, 1, 1] = -1.0 / M[:, 1, 0]
        else:
            C = cv[:, :n, :n]
            rhs = -np.einsum("rmj,rj->rm", C, M[:, 0, :n])
            A = np.einsum("rmj,rij->rmi", C, M[:, 1:n + 1, :n])
            cv[:, n, 1:n + 1] = np.linalg.solve(A, rhs[..., None])[..., 0]
        c = cv[:, n, :n + 1]
        cv[:, n] /= np.sqrt(np.einsum("ri,rij,rj->r", c, M[:, :n + 1, :n + 1], c))[:, None]
    return cv if f0.ndim == 2 else cv[0]


def _sahand_legendre_fit(X, d, rng, nsamples, bandwidth):
    """The fit of one Sahand-Legendre basis per column of X (n, S) (bases.jl:310-342): (kdes, minxs, scales, cVecs)."""
    a, b = rng
    X = np.asarray(X, dtype=np.float64)
    lo, step, h, coef, n = _kde_columns(X, (a <= X) & (X <= b), bandwidth)
    xs_samps = np.linspace(a, b, nsamples)
    S = X.shape[1]
    minxs, scales, cvecs = np.zeros(S), np.ones(S), np.zeros((S, d, d))
    has = np.flatnonzero(n > 0)
    if len(has):
        f0 = np.sqrt(np.maximum(_pdf_rows(lo[has], step[has], coef[has], np.broadcast_to(xs_samps, (len(has), nsamples))), 0.0))
        minxs[has], scales[has] = remove_zeros(xs_samps, f0)
        fit = minxs[has] != 0.0
        if fit.any():
            cvecs[has[fit]] = sahand_legendre_coeffs(xs_samps, f0[fit], d)
    kdes = [UnivariateKDE(float(lo[t]), float(step[t]), float(h[t]), coef[t]) for t in range(S)]
    return kdes, minxs, scales, cvecs


def init_sahand_legendre_time_dependent(X_norm, y=None, opts=None, range=None, max_samples=None, bandwidth=None):
    """bases.jl:310-342: [kdes, minxs, scales, cVecs], one entry per site.  A site without a value inside the range (the reference
    leaves its estimate undefined) and a site whose wavefunction is zero at every sample get zero coefficients."""
    X = np.asarray(X_norm, dtype=np.float64)
    nsamples = max(200, X.shape[1]) if max_samples is None else int(max_samples)
    kdes, minxs, scales, cvecs = _sahand_legendre_fit(X, opts.d, (-1.0, 1.0) if range is None else range, nsamples, bandwidth)
    return [kdes, minxs, scales, cvecs]


def init_sahand_legendre(X_norm, y=None, opts=None, range=None, max_samples=None, bandwidth=None):
    """bases.jl:294-307: [kde, minx, scale, cVecs] from all values at once.  The reference samples ``range(-a, b, S)``, a constant
    vector for (-1, 1); the samples here run from a to b as in the time-dependent form."""
    X = np.asarray(X_norm, dtype=np.float64)
    nsamples = max(200, X.shape[1]) if max_samples is None else int(max_samples)
    kdes, minxs, scales, cvecs = _sahand_legendre_fit(X.reshape(-1, 1), opts.d, (-1.0, 1.0) if range is None else range, nsamples, bandwidth)
    return [kdes[0], float(minxs[0]), float(scales[0]), cvecs[0]]


def sahand_legendre_encode(x, d, *args):
    """sahand_legendre_encode (bases.jl:111-129) for an array of values: ``(x, d, kde, minx, scale, cVecs)`` or, time dependent,
    ``(x, d, ti, kdes, minxs, scales, cVecs)`` with ``ti`` the site counted from 0.
    phi_n(x) = max(sqrt(max(pdf(kde, x), 0)), minx) / scale * sum_i cVecs[n][i] x^i."""
    if len(args) == 5:
        ti, kdes, minxs, scales, cvecs = args
        args = (kdes[ti], minxs[ti], scales[ti], cvecs[ti])
    k, minx, scale, cvecs = args
    x = np.asarray(x, dtype=np.float64)
    cvecs = np.asarray(cvecs, dtype=np.float64)[:d, :d]
    if not cvecs.any():
        return np.zeros(x.shape + (d,))
    f0 = np.maximum(np.sqrt(np.maximum(kde_pdf(k, x), 0.0)), minx)
    poly = np.zeros(x.shape + (d,))
    for i in range(d):                                                         # sum(c x^i) in the order of i, as :115 adds it
        poly += cvecs[:, i] * (x ** i)[..., None]
    return poly * f0[..., None] / scale


def sahand_legendre(time_dependent: bool = True) -> Encoding:
    """sahand_legendre(istimedependent) (basis_structs.jl:141-151)."""
    name = "Sahand-Legendre" + (" Time Dependent" if time_dependent else " Time Independent")
    init = init_sahand_legendre_time_dependent if time_dependent else init_sahand_legendre
    return Encoding(name, False, (-1.0, 1.0), sahand_legendre_encode, bool(time_dependent), True, init)


# ---------------------------------------------------------------------------------------
# Projected bases (basis_structs.jl:114-139, bases.jl:94-107, :141-154, :345-397): the closed-form Legendre / Fourier family, of
# which every site keeps the d members that carry most of the square root of a kernel density estimate of its training values
# ---------------------------------------------------------------------------------------
PROJ_LEGENDRE_TERMS, PROJ_FOURIER_TERMS = 7, 10                                # max_series_terms = 7d (bases.jl:390), 10d (:370)


def construct_kerneldensity_wavefunction(xs, xs_samps, max_samples=None, bandwidth=None):
    """bases.jl:141-154.  ``xs_samps`` an array: wf = sqrt(max(pdf(kde(xs), xs_samps), 0)); a (lo, hi) tuple: the sample points
    range(lo, hi, max_samples) - max(200, 2 len(xs)) of them by default - and wf.  The reference takes the root of the spline as it
    is and throws on a slightly negative value: the clamp is this package's definition, and so is wf = 0 for no values at all."""
    xs = np.asarray(xs, dtype=np.float64).ravel()
    if isinstance(xs_samps, tuple):
        samps = np.linspace(xs_samps[0], xs_samps[1], max(200, 2 * len(xs)) if max_samples is None else int(max_samples))
        return samps, construct_kerneldensity_wavefunction(xs, samps, bandwidth=bandwidth)
    xs_samps = np.asarray(xs_samps, dtype=np.float64)
    if len(xs) == 0:
        return np.zeros(xs_samps.shape)
    return np.sqrt(np.maximum(kde_pdf(kde(xs, bandwidth), xs_samps), 0.0))


def _trapezoid_weights(x):
    """w with sum(w * y) = _trapezoid(y, x), the same terms grouped by sample instead of by interval"""
    h = 0.5 * np.diff(x)
    w = np.zeros(len(x))
    w[:-1] += h
    w[1:] += h
    return w


def _select_terms(abs2, d):
    """partialsortperm(abs2, 1:d; rev=true) (bases.jl:354) per row: the 1-based positions of the d largest entries in descending
    order, ties to the smaller position (the sort is stable)"""
    return (np.argsort(-abs2, axis=-1, kind="stable")[..., :d] + 1).astype(np.int64)


def series_expand(basis, xs, ys, d):
    """series_expand (bases.jl:346-355): c_p = trapezoid(ys conj(b_p(xs)), xs) for the functions ``basis`` - a list of callables, or
    their values at xs as a (P, S) array -, then the 1-based positions of the d largest |c_p|^2, largest first."""
    xs = np.asarray(xs, dtype=np.float64)
    B = np.asarray(basis) if not callable(basis[0]) else np.stack([np.asarray(f(xs)) * np.ones(xs.shape) for f in basis])
    c = _trapezoid(np.asarray(ys) * np.conj(B), xs)
    return _select_terms(c.real ** 2 + c.imag ** 2, d)


def _projected_wavefunctions(X, rng, max_samples, bandwidth):
    """(xs_samps (S,), wf (T, S)): construct_kerneldensity_wavefunction of every column of X (N, T), all columns at once"""
    a, b = rng
    X = np.asarray(X, dtype=np.float64)
    N, T = X.shape
    S = max(200, 2 * N) if max_samples is None else int(max_samples)            # the length before the range filter (bases.jl:370)
    lo, step, h, coef, n = _kde_columns(X, (a <= X) & (X <= b), bandwidth)
    xs = np.linspace(-1.0, 1.0, S)                                              # (-1, 1) whatever the range is (:372, :392)
    wf = np.zeros((T, S))
    has = np.flatnonzero(n > 0)
    if len(has):
        wf[has] = np.sqrt(np.maximum(_pdf_rows(lo[has], step[has], coef[has], np.broadcast_to(xs, (len(has), S))), 0.0))
    return xs, wf


def _cospi(y):
    """cos(pi y) with the argument reduced first: y - 2 rint(y / 2) is exact, so only the rounding of y itself is left - the
    device's sincospi(y) has the same property"""
    return np.cos(np.pi * (y - 2.0 * np.rint(0.5 * y)))


def _sinpi(y):
    return np.sin(np.pi * (y - 2.0 * np.rint(0.5 * y)))


def project_legendre(X_norm, y=None, opts=None, range=None, d=None, max_series_terms=None, max_samples=None, bandwidth=None):
    """project_legendre (bases.jl:385-397) of the (N, T) training matrix: ``[ds]`` with ds (T, d) the 1-based positions, among the
    first 7d normalised Legendre polynomials (position p = order p - 1), of the d largest |c_p|^2 of the site's wavefunction.  One
    density estimate call and one (T, S) x (S, 7d) product for all sites."""
    d = int(opts.d if d is None else d)
    P = PROJ_LEGENDRE_TERMS * d if max_series_terms is None else int(max_series_terms)
    xs, wf = _projected_wavefunctions(X_norm, (-1.0, 1.0) if range is None else range, max_samples, bandwidth)
    c = wf @ (_legendre_table(xs, P) * _trapezoid_weights(xs)[:, None])
    return [_select_terms(c * c, d)]


def project_fourier(X_norm, y=None, opts=None, range=None, d=None, max_series_terms=None, max_samples=None, bandwidth=None):
    """project_fourier (bases.jl:365-376): ``[ds]`` with ds (T, d) the 1-based positions in get_fourier_freqs(10 d) = 0, 1, -1, 2, ...
    of the d largest |c_p|^2.  The wavefunction is real, so c_{-f} = conj(c_f): the coefficients are computed for f >= 0 only and
    those of -f are DEFINED as their conjugates.  |c|^2 of +f and -f is then the same number to the last bit, and of such a pair +f,
    which stands first in the list, is selected first - computed separately the two would differ in the last bits and the rounding
    would pick.  (The reference has no method that takes the matrix and the options, bases.jl:397 exists for Legendre only: this
    init is this package's definition of what the constructor names.)"""
    d = int(opts.d if d is None else d)
    P = PROJ_FOURIER_TERMS * d if max_series_terms is None else int(max_series_terms)
    if P > PROJ_FOURIER_TERMS * d:
        raise ValueError(f"max_series_terms = {P}: the encoder reads the positions in get_fourier_freqs({PROJ_FOURIER_TERMS} d)")
    xs, wf = _projected_wavefunctions(X_norm, (-1.0, 1.0) if range is None else range, max_samples, bandwidth)
    freqs = np.asarray(get_fourier_freqs(P))
    ang = xs[:, None] * np.arange(np.abs(freqs).max() + 1, dtype=np.float64)
    w = _trapezoid_weights(xs)[:, None]
    re, im = wf @ (_cospi(ang) * w), wf @ (-_sinpi(ang) * w)                    # conj(cispi(f x)), f >= 0
    abs2 = re * re + im * im
    return [_select_terms(abs2[:, np.abs(freqs)], d)]


def _site_positions(ds, ti):
    ds = np.asarray(ds)
    return (ds if ds.ndim == 1 else ds[ti]).astype(np.int64)


def projected_legendre_orders(ds):
    """The Legendre orders legendre_encode(x, nds, ds) (bases.jl:94-105) evaluates for the selected positions ds: Pl(x, p) with p the
    1-based position itself, one above the order p - 1 of the term that was selected.  Kept: it is what a model trained by the
    reference contains.  (An upstream fix is ``ds - 1`` here and nowhere else.)"""
    return np.asarray(ds, dtype=np.int64)


def projected_legendre_inv_norm(orders):
    """1 / sqrt(Pl(1, m; normalized) m) with m the largest order of each site (bases.jl:98-102), orders (..., d)"""
    m = np.asarray(orders).max(axis=-1).astype(np.float64)
    return 1.0 / np.sqrt(np.sqrt((2.0 * m + 1.0) / 2.0) * m)


def projected_fourier_freqs(ds, d):
    """The signed frequencies of the selected positions ds in get_fourier_freqs(10 d)"""
    return np.asarray(get_fourier_freqs(PROJ_FOURIER_TERMS * int(d)), dtype=np.int64)[np.asarray(ds, dtype=np.int64) - 1]


def projected_legendre_encode(x, d, ti, ds, norm=True):
    """legendre_encode(x, nds, ti, ds; norm) (bases.jl:94-107) for an array of values, ``ti`` the site counted from 0, ds (T, d) the
    fit's positions (or one site's (d,)): sqrt((2k + 1) / 2) P_k(x) for k in projected_legendre_orders(ds[ti]), with ``norm``
    divided by sqrt(Pl(1, m; normalized) m), m the site's largest order."""
    orders = projected_legendre_orders(_site_positions(ds, ti))
    out = _legendre_table(x, int(orders.max()) + 1)[..., orders]
    if norm:
        out = out * projected_legendre_inv_norm(orders)
    return out


def projected_legendre_encode_no_norm(x, d, ti, ds):
    return projected_legendre_encode(x, d, ti, ds, norm=False)


def projected_fourier_encode(x, d, ti, ds):
    """cispi(f_p x) / sqrt(d) for the site's selected positions p.  The reference's fourier_encode(x, nds, ds) (bases.jl) cannot be
    called and would use the position as the frequency: this is this package's definition, by intent."""
    x = np.asarray(x, dtype=np.float64)
    y = x[..., None] * projected_fourier_freqs(_site_positions(ds, ti), d).astype(np.float64)
    inv = 1.0 / math.sqrt(d)
    return (_cospi(y) * inv) + 1j * (_sinpi(y) * inv)


def legendre(norm: bool = False, project: bool = False) -> Encoding:
    """legendre(; norm, project) (basis_structs.jl:126-137).  ``project``: the projected basis, time dependent and data driven."""
    if not project:
        return model_encoding("Legendre_Norm" if norm else "Legendre_No_Norm")
    return Encoding("Projected Legendre_Norm" if norm else "Projected Legendre", False, (-1.0, 1.0),
                    projected_legendre_encode if norm else projected_legendre_encode_no_norm, True, True, project_legendre)


def legendre_no_norm(project: bool = False) -> Encoding:
    """basis_structs.jl:139."""
    return legendre(norm=False, project=project)


def fourier(project: bool = False) -> Encoding:
    """fourier(; project) (basis_structs.jl:114-124)."""
    if not project:
        return model_encoding("Fourier")
    return Encoding("Projected Fourier", True, (-1.0, 1.0), projected_fourier_encode, True, True, project_fourier)


_PROJ_DEVICE_BASIS = {projected_legendre_encode: "Legendre_Norm", projected_legendre_encode_no_norm: "Legendre_No_Norm",
                      projected_fourier_encode: "Fourier"}

_SPLIT_PREFIXES = (("hist_split_", "hist._split_", "histogram_split_"), ("unif_split_", "unif._split_", "uniform_split_"))


def model_encoding(symbol, custom: Optional[Encoding] = None, project: bool = False) -> Encoding:
    """options.jl:243-279."""
    if project:
        raise NotImplementedError("projected_basis=True is not built from the options: set encoding='Custom' and pass "
                                  "custom_encoding=legendre(project=True), legendre(norm=True, project=True) or fourier(project=True)")
    if isinstance(symbol, Encoding):
        return symbol
    s = str(symbol).lstrip(":").lower()
    for kind, prefixes in enumerate(_SPLIT_PREFIXES):                          # :261-272
        if s.startswith(prefixes):
            aux = model_encoding(s[s.index("split_") + 6:])
            return uniform_split(aux) if kind else histogram_split(aux)
    canon, iscomplex, rng, data_driven = encoding_info(symbol)
    if canon == "Custom":
        if custom is None:
            raise ValueError("To use a custom encoding, pass custom_encoding")
        return custom
    if data_driven:
        ctor = {"SLTD": "sahand_legendre(time_dependent=True)", "Sahand_Legendre": "sahand_legendre(time_dependent=False)",
                "Projected_Legendre": "legendre(project=True)", "Projected_Legendre_Norm": "legendre(norm=True, project=True)",
                "Projected_Fourier": "fourier(project=True)"}[canon]
        what = "a projected basis (projected_basis)" if canon.startswith("Projected_") else f"encoding {canon}"
        raise NotImplementedError(f"{what} is not built from its symbol: set encoding='Custom' and pass custom_encoding={ctor}")
    fn = {"Legendre_No_Norm": legendre_encode_no_norm, "Legendre_Norm": legendre_encode, "Fourier": fourier_encode,
          "Stoudenmire": angle_encode, "Sahand": sahand_encode, "Uniform": uniform_encode}[canon]
    return Encoding(canon, iscomplex, rng, fn)


def symbolic_encoding(enc: Encoding) -> str:
    """Inverse of model_encoding (options.jl:281-296); basis_tests.jl:8 pins the round trip."""
    return enc.name.replace(" ", "_").replace("-", "_")


def encoding_from_name(name) -> Optional[Encoding]:
    """The Encoding of a stored ``Encoding.name`` where a constructor of this package builds it - the Sahand-Legendre bases, the
    projected bases and whatever model_encoding builds from the name's symbol -, else None (a function_basis has to be handed over again)."""
    for enc in (sahand_legendre(True), sahand_legendre(False), legendre(project=True), legendre(norm=True, project=True), fourier(project=True)):
        if enc.name == name:
            return enc
    try:
        return model_encoding(str(name).replace(" ", "_").replace("-", "_"))
    except (ValueError, NotImplementedError):
        return None


def opts_encoding(opts, custom: Optional[Encoding] = None) -> Encoding:
    """opts.encoding as an Encoding (the reference's Options holds the object, MPSOptions here its name)."""
    return model_encoding(opts.encoding, custom, opts.projected_basis)


# ---------------------------------------------------------------------------------------
# the fit step: opts.encoding.init(X_norm, y; opts) (encodings.jl:129-138) and encode_TS (:1-31) bound to its result
# ---------------------------------------------------------------------------------------
class FittedEncoder:
    """encode_TS with the encoding arguments bound: ``enc(X)`` maps an (N, T) matrix of values in the encoding's range to
    (N, T, d), column t through site t's basis; ``enc.table(xvals, T)`` tabulates candidate values - (ngrid, d), or
    (T, ngrid, d) for a time-dependent encoding (imputation.jl:92-107)."""

    def __init__(self, enc: Encoding, d: int, args):
        self.enc, self.d, self.args = enc, int(d), args

    def __call__(self, X):
        X = np.asarray(X, dtype=np.float64)
        if not self.enc.istimedependent:
            return self.enc.encode(X, self.d, *self.args)
        return np.stack([self.enc.encode(X[:, t], self.d, t, *self.args) for t in range(X.shape[1])], axis=1)

    def table(self, xvals, T):
        if not self.enc.istimedependent:
            return self.enc.encode(xvals, self.d, *self.args)
        return np.stack([self.enc.encode(xvals, self.d, t, *self.args) for t in range(T)])

    @property
    def bins(self):
        """the split bases' edges: (nbins + 1,) shared by all sites or (T, nbins + 1); None for any other encoding"""
        return np.asarray(self.args[1][0]) if self.enc.aux_enc is not None else None

    @property
    def kde(self):
        """the Sahand-Legendre bases' fitted tables as the device takes them (mpst_kde_opts): a dict of ``npoints``, ``per_site`` and
        the arrays lo, step (S,), coef (S, K + 2), minx, scale (S,), cvecs (S, d, d), S = T or 1; None for any other encoding"""
        if self.enc.encode is not sahand_legendre_encode:
            return None
        kdes, minxs, scales, cvecs = self.args
        if not self.enc.istimedependent:
            kdes, minxs, scales, cvecs = [kdes], [minxs], [scales], [cvecs]
        c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        return dict(npoints=kdes[0].npoints, per_site=int(self.enc.istimedependent), lo=c([k.lo for k in kdes]), step=c([k.step for k in kdes]),
                    coef=c([k.coef for k in kdes]), minx=c(minxs), scale=c(scales), cvecs=c(cvecs)[:, :self.d, :self.d].copy())

    @property
    def orders(self):
        """the projected bases' fitted tables as the device takes them (mpst_proj_opts): a dict of ``basis`` ("Legendre_Norm",
        "Legendre_No_Norm" or "Fourier"), ``orders`` (T, d) int32 - the Legendre orders or signed Fourier frequencies that are
        evaluated, not the fit's positions - and ``inv_norm`` (T,), ones unless the basis is "Legendre_Norm"; None for any other
        encoding"""
        basis = _PROJ_DEVICE_BASIS.get(self.enc.encode)
        if basis is None:
            return None
        ds = np.asarray(self.args[0], dtype=np.int64)
        orders = projected_fourier_freqs(ds, self.d) if basis == "Fourier" else projected_legendre_orders(ds)
        inv = projected_legendre_inv_norm(orders) if basis == "Legendre_Norm" else np.ones(len(orders))
        return dict(basis=basis, orders=np.ascontiguousarray(orders, dtype=np.int32), inv_norm=np.ascontiguousarray(inv, dtype=np.float64))

    def device_kwargs(self):
        """the keyword argument SweepEngine.encode_dataset / encode_values take this encoding's fitted tables by: {} for an encoding
        without any (the closed-form bases), else its ``bins``, ``kde`` or ``orders`` under that name; None for a fitted encoding the
        device does not encode"""
        if self.enc.init is None:
            return {}
        for key in ("bins", "kde", "orders"):
            tables = getattr(self, key)
            if tables is not None:
                return {key: tables}
        return None


def fit_encoding(enc: Encoding, X_norm, y, opts: MPSOptions):
    """The fit step of encode_safe_dataset (encodings.jl:129-132): ``(encoding_args, encoder)``.  ``X_norm`` is the training
    matrix (N, T) after transform_train_data, ``encoder`` a FittedEncoder.  Closed-form encodings have nothing to fit: their
    encoder is ``enc.encode(X, d)`` itself."""
    if enc.isdatadriven and opts.encode_classes_separately:
        raise NotImplementedError("encode_classes_separately=True together with a data-driven encoding is not implemented")
    args = [] if enc.init is None else enc.init(X_norm, y, opts=opts)
    return args, FittedEncoder(enc, opts.d, args)


def fit_encoding_from_training_data(opts: MPSOptions, X_train, y_train=None, custom: Optional[Encoding] = None):
    """get_enc_args_from_opts (imputation.jl:23-45): re-derive the encoding arguments from the raw training data a
    TrainedMPS carries.  Returns (enc, norms, encoder)."""
    enc = opts_encoding(opts, custom)
    if enc.init is None:
        return enc, None, FittedEncoder(enc, opts.d, [])
    X_norm, norms = transform_train_data(X_train, opts, enc.range)
    if y_train is not None:
        X_norm = X_norm[np.argsort(np.asarray(y_train), kind="stable")]        # :39-40
    return enc, norms, fit_encoding(enc, X_norm, y_train, opts)[1]


# ---------------------------------------------------------------------------------------
# preprocessing (src/utils.jl:161-295).  Series are ROWS here ((N, T)); both normalisations
# are fitted over the whole matrix, so the reference's transposed orientation is immaterial.
# ---------------------------------------------------------------------------------------
@dataclass
class Norms:
    sigmoid: Optional[tuple] = None   # (median, iqr)  - Normalization.jl RobustSigmoid
    minmax: Optional[tuple] = None    # (min, max)


def _robust_sigmoid(X, med, iqr):
    return 1.0 / (1.0 + np.exp(-(X - med) / (iqr / 1.35)))


def transform_train_data(X_train, opts: MPSOptions, enc_range):
    """utils.jl:161-199."""
    Xs = np.array(X_train, dtype=np.float64, copy=True)
    norms = Norms()
    if opts.sigmoid_transform:
        med = float(np.median(Xs))
        q75, q25 = np.percentile(Xs, [75.0, 25.0])
        norms.sigmoid = (med, float(q75 - q25))
        Xs = _robust_sigmoid(Xs, *norms.sigmoid)
    if opts.minmax:
        lo, hi = float(Xs.min()), float(Xs.max())
        norms.minmax = (lo, hi)
        Xs = (Xs - lo) / (hi - lo)
        lb, ub = opts.data_bounds
        Xs = Xs * (ub - lb) + lb
    a, b = enc_range
    return (b - a) * Xs + a, norms


def transform_test_data(X_test, norms: Norms, opts: MPSOptions, enc_range, rescale_out_of_bounds=True):
    """utils.jl:202-275: train-fitted transforms, then per-series out-of-bounds rescale (:243-266)."""
    Xs = np.array(X_test, dtype=np.float64, copy=True)
    if Xs.size == 0:
        return Xs, []
    if norms.sigmoid is not None:
        Xs = _robust_sigmoid(Xs, *norms.sigmoid)
    if norms.minmax is not None:
        lo, hi = norms.minmax
        Xs = (Xs - lo) / (hi - lo)
    if opts.minmax:
        lb, ub = opts.data_bounds
        Xs = Xs * (ub - lb) + lb
    oob = []
    if rescale_out_of_bounds:
        for i in range(Xs.shape[0]):
            ts = Xs[i]
            tr = [i, 0.0, 1.0]
            lo, hi = float(ts.min()), float(ts.max())
            if lo < 0:
                ts -= lo
                hi = float(ts.max())
                tr[1] = lo
            if hi > 1:
                ts /= hi
                tr[2] = hi
            if tr[1:] != [0.0, 1.0]:
                oob.append(tr)
    a, b = enc_range
    return (b - a) * Xs + a, oob


def transform_data(X_train, X_test, opts: MPSOptions, enc_range):
    """utils.jl:287-295."""
    Xtr, norms = transform_train_data(X_train, opts, enc_range)
    Xte, oob = transform_test_data(X_test, norms, opts, enc_range)
    return Xtr, Xte, norms, oob


# ---------------------------------------------------------------------------------------
# encode_dataset (Encodings/encodings.jl:33-156)
# ---------------------------------------------------------------------------------------
def encode_dataset(X_orig, X_scaled, y, enc: Encoding, d, class_keys, encoder=None) -> EncodedTimeSeriesSet:
    """Stable sort by class (:43), range check (:115-119), encode every value, class
    distribution in class-key order (:151-152).  ``encoder``: the FittedEncoder of the training set (``fit_encoding``),
    required for an encoding with an init step (:133-138)."""
    if encoder is None:
        if enc.init is not None:
            raise ValueError("Can't encode a test or val set without training encoding arguments!")
        encoder = FittedEncoder(enc, d, [])
    y = np.asarray(y)
    if X_scaled.shape[0] == 0:
        return EncodedTimeSeriesSet.empty()
    order = np.argsort(y, kind="stable")
    Xo, Xs, ys = np.asarray(X_orig)[order], X_scaled[order], y[order]
    a, b = enc.range
    if not np.all((a <= Xs) & (Xs <= b)):
        raise ValueError(f"Data must be rescaled between {a} and {b} before a {enc.name} encoding.")
    phi = encoder(Xs)
    label_index = np.array([class_keys[v] for v in ys.tolist()], dtype=np.int32)
    _, counts = np.unique(ys, return_counts=True)
    return EncodedTimeSeriesSet(phi, ys, label_index, np.array(Xo, dtype=np.float64), counts.astype(np.int64))
