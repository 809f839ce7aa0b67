"""Loop-by-loop restatement of the projected bases ("Projected bases"): the fit - the wavefunction of one site, its series
coefficients, the selection - and the two encoders, one site and one value at a time.  The checker of tests/test_proj_host.py and
tests/test_gpu_proj.py: it shares no code with the package; the density estimate is tests/kde_ref.py's.  The encoders take the
number type as an argument: np.float64 restates what package and device compute, np.longdouble is the yardstick that says how much
of a state float64 arithmetic itself loses."""
import math

import numpy as np

from tests import kde_ref as KR

LEGENDRE_TERMS, FOURIER_TERMS = 7, 10


def fourier_freqs(n):
    """0, 1, -1, 2, -2, ...: the first n"""
    out = [0]
    f = 1
    while len(out) < n:
        out += [f, -f]
        f += 1
    return out[:n]


def legendre_values(x, kmax, dtype=np.float64):
    """[sqrt((2k + 1) / 2) P_k(x) for k = 0 .. kmax], Bonnet's recursion in ``dtype``"""
    x = dtype(x)
    one, two = dtype(1), dtype(2)
    p = [one, x]
    for k in range(1, kmax):
        p.append((dtype(2 * k + 1) * x * p[k] - dtype(k) * p[k - 1]) / dtype(k + 1))
    return [p[k] * np.sqrt((two * dtype(k) + one) / two) for k in range(kmax + 1)]


def wavefunction(column, bw=None):
    """(sample points, wf) of one site: S = max(200, 2 len(column)) points over [-1, 1], wf = sqrt(max(pdf, 0)) of the estimate of
    the values inside [-1, 1], zeros when there is none"""
    S = max(200, 2 * len(column))
    samp = [float(v) for v in np.linspace(-1.0, 1.0, S)]
    xs = [float(v) for v in column if -1.0 <= v <= 1.0]
    if not xs:
        return samp, [0.0] * S
    k = KR.kde(xs, bw)
    return samp, [math.sqrt(max(KR.pdf(k, x), 0.0)) for x in samp]


def legendre_abs2(samp, wf, nterms):
    """|c_p|^2, p = 1 .. nterms: c_p = trapezoid(wf b_p), b_p the normalised Legendre polynomial of order p - 1"""
    table = [legendre_values(x, nterms - 1) for x in samp]
    return [float(KR.trapezoid([wf[q] * table[q][p] for q in range(len(samp))], samp)) ** 2 for p in range(nterms)]


def fourier_abs2(samp, wf, nterms):
    """|c_p|^2 for the frequencies fourier_freqs(nterms): c_f = trapezoid(wf conj(cispi(f x))) for f >= 0, c_{-f} = conj(c_f) by
    definition"""
    freqs = fourier_freqs(nterms)
    pos = {}
    for f in range(max(abs(v) for v in freqs) + 1):
        re = KR.trapezoid([wf[q] * math.cos(math.pi * f * samp[q]) for q in range(len(samp))], samp)
        im = KR.trapezoid([-wf[q] * math.sin(math.pi * f * samp[q]) for q in range(len(samp))], samp)
        pos[f] = (re, im)
    coef = [(pos[abs(f)][0], pos[abs(f)][1] if f >= 0 else -pos[abs(f)][1]) for f in freqs]
    return [re * re + im * im for re, im in coef]


def select(abs2, d):
    """the 1-based positions of the d largest entries, largest first, ties to the smaller position"""
    return sorted(range(1, len(abs2) + 1), key=lambda p: (-abs2[p - 1], p))[:d]


def fit(X, d, kind, bw=None):
    """(ds, abs2): per site the selected positions and all |c_p|^2; kind "legendre" or "fourier" """
    X = np.asarray(X, dtype=np.float64)
    ds, all_abs2 = [], []
    for t in range(X.shape[1]):
        samp, wf = wavefunction(X[:, t], bw)
        abs2 = legendre_abs2(samp, wf, LEGENDRE_TERMS * d) if kind == "legendre" else fourier_abs2(samp, wf, FOURIER_TERMS * d)
        ds.append(select(abs2, d))
        all_abs2.append(abs2)
    return ds, all_abs2


def encode_legendre_value(x, positions, norm, dtype=np.float64):
    """The reference's legendre_encode(x, nds, ds): Pl(x, p) for the selected 1-based POSITION p - one above the order p - 1 of the
    term that was selected -, with ``norm`` divided by sqrt(Pl(1, m) m), m = max(positions), Pl(1, m) = sqrt((2m + 1) / 2)."""
    m = max(positions)
    vals = legendre_values(x, m, dtype)
    out = [vals[p] for p in positions]
    if norm:
        nrm = np.sqrt(np.sqrt((dtype(2) * dtype(m) + dtype(1)) / dtype(2)) * dtype(m))
        out = [v / nrm for v in out]
    return out


def _pi(dtype):
    return dtype(4) * np.arctan(dtype(1))


def encode_fourier_value(x, positions, d, dtype=np.float64):
    """cispi(f_p x) / sqrt(d) for the selected positions p in fourier_freqs(10 d), as (re, im) pairs.  f x is formed in ``dtype``
    and reduced by whole periods - exactly - before it meets pi."""
    freqs = fourier_freqs(FOURIER_TERMS * d)
    out = []
    for p in positions:
        y = dtype(freqs[p - 1]) * dtype(x)
        r = y - dtype(2) * np.rint(y / dtype(2))
        out.append((np.cos(_pi(dtype) * r) / np.sqrt(dtype(d)), np.sin(_pi(dtype) * r) / np.sqrt(dtype(d))))
    return out


def encode_matrix(X, ds, kind, d, norm=False, dtype=np.float64):
    """(N, T) values -> (N, T, d) states of ``dtype`` (Legendre) or its complex counterpart (Fourier); ds: per site the positions"""
    X = np.asarray(X, dtype=np.float64)
    cdt = np.clongdouble if dtype is np.longdouble else np.complex128
    out = np.zeros(X.shape + (d,), dtype=dtype if kind == "legendre" else cdt)
    for i in range(X.shape[0]):
        for t in range(X.shape[1]):
            pos = [int(p) for p in ds[t]]
            if kind == "legendre":
                out[i, t] = encode_legendre_value(float(X[i, t]), pos, norm, dtype)
            else:
                for j, (re, im) in enumerate(encode_fourier_value(float(X[i, t]), pos, d, dtype)):
                    out[i, t, j] = cdt(re) + cdt(1j) * cdt(im)
    return out


def float64_loss(X, ds, kind, d, norm=False):
    """e_ref: the largest |float64 restatement - longdouble restatement| over the states of X - what float64 arithmetic itself loses
    on these inputs -, and the float64 states"""
    lo = encode_matrix(X, ds, kind, d, norm, np.float64)
    hi = encode_matrix(X, ds, kind, d, norm, np.longdouble)
    return float(np.abs(hi - lo).max()), lo
