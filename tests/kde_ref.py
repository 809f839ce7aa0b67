"""Loop-by-loop restatement of the Sahand-Legendre definitions ("Sahand-Legendre encodings"): the density estimate, the
fit and the encode step, one site and one value at a time.  The checker of tests/test_kde_host.py and tests/test_gpu_kde.py: it
shares no code with the package - the spline comes from a dense (K + 2) x (K + 2) solve, the polynomials from sum(c * x**i)."""
import math

import numpy as np

K_DEFAULT = 2048


def bandwidth(xs):
    n = len(xs)
    if n <= 1:
        return 0.9
    std = float(np.std(xs, ddof=1))
    q25, q75 = np.quantile(xs, [0.25, 0.75])
    w = min(std, float(q75 - q25) / 1.34)
    if w == 0.0:
        w = 1.0 if std == 0.0 else std
    return 0.9 * w * n ** (-0.2)


_SPLINE = {}


def spline_matrix(K):
    if K not in _SPLINE:
        A = np.zeros((K + 2, K + 2))
        A[0, :3] = (1.0, -2.0, 1.0)
        A[K + 1, K - 1:] = (1.0, -2.0, 1.0)
        for i in range(1, K + 1):
            A[i, i - 1:i + 2] = (0.125, 0.75, 0.125)
        _SPLINE[K] = A
    return _SPLINE[K]


def kde(xs, bw=None, K=K_DEFAULT):
    """dict(lo, step, h, K, coef) of the estimate of the values xs"""
    xs = [float(v) for v in xs]
    n = len(xs)
    h = bandwidth(np.array(xs)) if bw is None else float(bw)
    lo, hi = min(xs) - 4.0 * h, max(xs) + 4.0 * h
    step = (hi - lo) / (K - 1)
    grid = [lo + k * step for k in range(K)]
    cells = [0.0] * K
    for x in xs:
        k = 0
        lo_k, hi_k = 0, K                       # first index with grid[k] >= x, by bisection
        while lo_k < hi_k:
            mid = (lo_k + hi_k) // 2
            if grid[mid] >= x:
                hi_k = mid
            else:
                lo_k = mid + 1
        k = lo_k
        j = k - 1
        if j >= 0 and k <= K - 1:
            cells[j] += (grid[k] - x) / (n * step * step)
            cells[k] += (x - grid[j]) / (n * step * step)
    ft = np.fft.rfft(np.array(cells))
    for m in range(len(ft)):
        omega = 2.0 * math.pi * m / (K * step)
        ft[m] *= math.exp(-0.5 * h * h * omega * omega)
    dens = np.maximum(np.fft.irfft(ft, n=K), 0.0)
    rhs = np.concatenate([[0.0], dens, [0.0]])
    coef = np.linalg.solve(spline_matrix(K), rhs)
    return dict(lo=lo, step=step, h=h, K=K, coef=coef)


def pdf(k, x):
    lo, step, K, c = k["lo"], k["step"], k["K"], k["coef"]
    if x < lo or x > lo + (K - 1) * step:
        return 0.0
    u = (x - lo) / step + 1.0
    i = int(min(max(round(u), 1), K))           # Python rounds halves to even, as Julia does
    s = u - i
    return c[i - 1] * 0.5 * (s - 0.5) ** 2 + c[i] * (0.75 - s * s) + c[i + 1] * 0.5 * (s + 0.5) ** 2


def trapezoid(ys, xs):
    return sum((ys[q] + ys[q + 1]) * 0.5 * (xs[q + 1] - xs[q]) for q in range(len(xs) - 1))


def remove_zeros(xs, f0):
    tol = 0.01 * max(abs(v) for v in f0)
    good = [abs(v) for v in f0 if abs(v) > tol]
    if not good:
        return 0.0, 1.0
    minval = min(good)
    for q in range(len(f0)):
        if abs(f0[q]) <= tol:
            f0[q] = minval
    norm = trapezoid([v * v for v in f0], xs)
    for q in range(len(f0)):
        f0[q] /= norm
    return minval, norm


def moment_matrix(xs, f0, d):
    return np.array([[trapezoid([xs[q] ** (i + j) * f0[q] ** 2 for q in range(len(xs))], xs) for j in range(d)] for i in range(d)])


def coeffs(xs, f0, d):
    M = moment_matrix(xs, f0, d)
    cv = np.zeros((d, d))
    cv[0, 0] = 1.0
    for n in range(1, d):
        if n == 1:
            cv[1, 0] = 1.0
            cv[1, 1] = -1.0 / M[1, 0]
        else:
            C = cv[:n, :n]
            rhs = -(C @ M[0, :n])
            A = C @ M[1:n + 1, :n].T
            sol = np.linalg.solve(A, rhs)
            cv[n, 0] = 1.0
            cv[n, 1:n + 1] = sol
        c = cv[n, :n + 1]
        cv[n] = cv[n] / math.sqrt(c @ M[:n + 1, :n + 1] @ c)
    return cv


def fit_site(xs_all, d, a, b, S, bw=None):
    """(kde or None, minx, scale, cvecs) of one site from its values xs_all"""
    xs = [float(v) for v in xs_all if a <= v <= b]
    zero = np.zeros((d, d))
    if not xs:
        return None, 0.0, 1.0, zero
    k = kde(xs, bw)
    samp = [float(v) for v in np.linspace(a, b, S)]
    f0 = [math.sqrt(max(pdf(k, x), 0.0)) for x in samp]
    minx, scale = remove_zeros(samp, f0)
    if minx == 0.0:
        return k, minx, scale, zero
    return k, minx, scale, coeffs(samp, f0, d)


def fit_time_dependent(X, d, a=-1.0, b=1.0, bw=None):
    X = np.asarray(X, dtype=np.float64)
    S = max(200, X.shape[1])
    return [fit_site(X[:, t], d, a, b, S, bw) for t in range(X.shape[1])]


def fit_time_independent(X, d, a=-1.0, b=1.0, bw=None):
    X = np.asarray(X, dtype=np.float64)
    return fit_site(X.ravel(), d, a, b, max(200, X.shape[1]), bw)


def encode_value(x, d, site):
    k, minx, scale, cv = site
    if not cv.any():
        return np.zeros(d)
    f0 = max(math.sqrt(max(pdf(k, x), 0.0)), minx)
    return np.array([sum(cv[n, i] * x ** i for i in range(d)) * f0 / scale for n in range(d)])


def encode_matrix(X, d, sites):
    """(N, T) values -> (N, T, d); sites: one fit per column, or a single fit for all columns"""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros(X.shape + (d,))
    for i in range(X.shape[0]):
        for t in range(X.shape[1]):
            out[i, t] = encode_value(float(X[i, t]), d, sites[t] if isinstance(sites, list) else sites)
    return out
