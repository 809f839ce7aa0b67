"""NumPy restatement of the observed conditionals (mpst_observed_conditionals): the marginal site conditionals of tests/margcond_ref.py
with a measurement operator E_t at every site.

    E = phi phi^H (EXACT), 1 (MISSING), sum_k w_k k_k g_k g_k^H (GAUSS, INTERVAL: the likelihood k_k on the grid, w_k the weights of
        cumul_trapz_even), E_user (OPERATOR)
    step:   L' = sum_{s'} B_{s'}^T L conj(A_{s'}),  B_{s'} = sum_s conj(E[s, s']) A_s   (tests/margcond_ref._step at EXACT / MISSING)
    rho_t:  tests/margcond_ref.rho_site of L_{t-1}, W_t, R_{t+1} - site t's own observation never enters it
    predictive group: from p_k = max(Re(g_k^H rho_t g_k), 0);   posterior group: from k_k p_k
    nll_obs = -ln(tr(E_t rho_t) / trapz(p)),   logev = sum of the logs of the left walk's traces + ln tr(E_{T-1} rho_{T-1})

``dense_evidence`` gives logev and rho_t from the full d^T amplitude tensor contracted with the E_t (tiny chains only);
``logev_longdouble`` walks in extended precision.  TEST INFRASTRUCTURE ONLY (checker of tests/test_observed_host.py and
tests/test_gpu_observed.py)."""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import impute_numpy as I
from tests import margcond_ref as M
from tests import site_cond_ref as S
from tests.marginal_ref import class_slice, label_site_of

EXACT, MISSING, GAUSS, INTERVAL, OPERATOR = 0, 1, 2, 3, 4
LEVELS = (0.05, 0.5, 0.95)


def quad_weights(xs):
    w = np.full(len(xs), xs[1] - xs[0])
    w[0] = w[-1] = 0.5 * (xs[1] - xs[0])
    return w


def likelihood(kind, a, b, xs):
    """k_k of a GAUSS / INTERVAL site on the grid"""
    if kind == GAUSS:
        return np.exp(-(xs - a) ** 2 / (2.0 * b * b)) / (b * np.sqrt(2.0 * np.pi))
    return ((a <= xs) & (xs <= b)).astype(np.float64)


def operator_quadrature(kind, a, b, xs, g):
    """(E, bound): E[s, s'] = sum_k w_k k_k g_k[s] conj(g_k[s']) and the entrywise bound (ngrid + 8) 2^-52 sum_k w_k k_k |g_k[s]| |g_k[s']|:
    the worst case of a sum of ngrid rounded terms in any order, plus the ulps of exp"""
    wk = quad_weights(xs) * likelihood(kind, a, b, xs)
    E = np.einsum("k,ks,kt->st", wk, g, np.conj(g))
    bound = (len(xs) + 8) * 2.0 ** -52 * np.einsum("k,ks,kt->st", wk, np.abs(g), np.abs(g))
    return E, bound


def site_operator(kind, a, b, phi, E_user, xs, g):
    if kind == EXACT:
        return np.outer(phi, np.conj(phi))
    if kind == MISSING:
        return np.eye(g.shape[1], dtype=g.dtype)
    if kind == OPERATOR:
        return np.asarray(E_user)
    return operator_quadrature(kind, a, b, xs, g)[0]


def _step(L, A, kind, phi_j, E):
    """the step through a site: margcond_ref._step at EXACT / MISSING, the generalised form with the operator E otherwise"""
    if kind <= MISSING:
        return M._step(L, A, phi_j, kind == MISSING)
    d = A.shape[1]
    out = 0
    for sp in range(d):
        B = sum(np.conj(E[s, sp]) * A[:, s, :] for s in range(d))
        out = out + B.T @ L @ np.conj(A[:, sp, :])
    return out


def walks(cm, kinds, enc, ops, scaled=True):
    """(L, R, lg): L[t] = L_{t-1}, R[t] = R_{t+1}, lg[t] = the sum of the logs of the traces the left walk divided by up to L[t]"""
    T = len(cm)
    one = np.ones((1, 1), dtype=np.result_type(cm[0].dtype, *(o.dtype for o in ops)))
    L, lg = [one], [0.0]
    for j in range(T - 1):
        n = _step(L[-1], cm[j], kinds[j], enc[j], ops[j])
        tr = np.trace(n).real if scaled else 1.0
        L.append(n / tr)
        lg.append(lg[-1] + np.log(tr))
    R = [one]
    for j in range(T - 1, 0, -1):
        n = _step(R[-1], cm[j].transpose(2, 1, 0), kinds[j], enc[j], ops[j])
        R.append(n / np.trace(n).real if scaled else n)
    return L, R[::-1], lg


@dataclass
class ObservedRef:
    pred: S.SiteCondRef         # the predictive group; pred.nll is nll_obs, pred.pit is pit
    post: S.SiteCondRef         # the posterior group (NaN at EXACT / OPERATOR sites and where trapz(k p) is not positive)
    pred_mean: np.ndarray       # (N, T)
    post_mean: np.ndarray
    logev: np.ndarray           # (N,)
    E: np.ndarray               # (N, T, d, d) the operators used
    rho: np.ndarray             # (N, T, d, d)
    excused: np.ndarray         # (N, T) bool: a selection margin of either group is at most 1e-9


def _margin(sc, nq):
    m = np.minimum(sc.med_margin, sc.err_margin)
    return np.minimum(m, sc.lev_margin.min(axis=2)) if nq else m


def observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x, xs, grid_phi, levels=(), scaled=True, E_given=None):
    """``E_given`` (N, T, d, d): the operators of the GAUSS / INTERVAL sites are taken from it (the device's own E_out) instead of the
    quadrature.  ``x`` (N, T): the values of EXACT sites, held-out values or NaN at MISSING ones."""
    N, T = kind.shape
    d = W[0].shape[1]
    dt = np.result_type(W[0].dtype, grid_phi.dtype)
    pred, post = S._empty(x, len(xs), len(levels)), S._empty(x, len(xs), len(levels))
    pmean, qmean, logev = np.zeros((N, T)), np.zeros((N, T)), np.zeros(N)
    Eall, rho = np.zeros((N, T, d, d), dtype=dt), np.zeros((N, T, d, d), dtype=dt)
    slices = {c: class_slice(W, c) for c in set(int(c) for c in lab)}
    nanfill = lambda sc, i, t: [getattr(sc, f).__setitem__((i, t), np.nan) for f in ("median", "err", "quantiles", "F")]
    for i in range(N):
        cm = slices[int(lab[i])]
        gt = lambda t: grid_phi[t] if grid_phi.ndim == 3 else grid_phi
        ops = []
        for t in range(T):
            k = int(kind[i, t])
            if E_given is not None and k in (GAUSS, INTERVAL):
                ops.append(np.asarray(E_given[i, t]))
            else:
                ops.append(site_operator(k, a[i, t], b[i, t], phi[i, t], None if E_user is None else E_user[i, t], xs, gt(t)).astype(dt))
            Eall[i, t] = ops[-1]
        L, R, lg = walks(cm, kind[i], phi[i], ops, scaled)
        for t in range(T):
            k = int(kind[i, t])
            r = M.rho_site(L[t], cm[t], R[t])
            rho[i, t] = r
            p = M.grid_density(r, gt(t))
            Z = I.cumul_trapz_even(xs, p)[-1]
            xv = x[i, t] if k <= MISSING else np.nan
            if k <= MISSING:
                pobs = float((np.conj(phi[i, t]) @ r @ phi[i, t]).real) if np.isfinite(xv) else np.nan
            else:
                pobs = float(np.trace(ops[t] @ r).real)
            S._finish(pred, i, t, xs, p, pobs, xv, levels)
            if np.isfinite(pobs) and not pobs > 0.0:
                pred.nll[i, t] = np.inf
            pmean[i, t] = I.cumul_trapz_even(xs, xs * p)[-1] / Z
            if t == T - 1:
                tr = float(np.trace(ops[t] @ r).real)
                logev[i] = lg[t] + np.log(tr) if tr > 0 else -np.inf
            # the posterior group
            post.med_margin[i, t] = post.err_margin[i, t] = 1.0
            post.lev_margin[i, t] = 1.0
            if k in (EXACT, OPERATOR):
                nanfill(post, i, t)
                qmean[i, t] = np.nan
                continue
            kp = p * likelihood(k, a[i, t], b[i, t], xs) if k in (GAUSS, INTERVAL) else p
            Zq = I.cumul_trapz_even(xs, kp)[-1]
            if not (Zq > 0 and np.isfinite(Zq)):
                nanfill(post, i, t)
                qmean[i, t] = np.nan
                continue
            S._finish(post, i, t, xs, kp, np.nan, np.nan, levels)
            qmean[i, t] = I.cumul_trapz_even(xs, xs * kp)[-1] / Zq
    margin = np.minimum(_margin(pred, len(levels)), _margin(post, len(levels)))
    return ObservedRef(pred, post, pmean, qmean, logev, Eall, rho, margin <= 1e-9)


def dense_evidence(cm, ops):
    """(logev, rho): from the amplitude tensor psi[s_1 ... s_T]: value = sum_{s s'} prod_t conj(E_t[s_t, s'_t]) psi(s) conj(psi(s')) and
    rho_t[s, s'] the same with site t left open (rho_t[s, s'] = sum psi(.. s ..) conj(psi(.. s' ..)) over the others)."""
    T = len(cm)
    psi = cm[0][0]
    for w in cm[1:]:
        psi = np.tensordot(psi, w, axes=([psi.ndim - 1], [0]))
    psi = psi[..., 0]

    def applied(skip):
        y = psi
        for t in range(T):
            if t != skip:
                y = np.moveaxis(np.tensordot(y, np.conj(ops[t]), axes=([t], [0])), -1, t)      # y(.. s'_t ..) = sum_s conj(E[s, s']) y(.. s ..)
        return y
    value = np.sum(applied(None) * np.conj(psi)).real
    rho = []
    for t in range(T):
        y = np.moveaxis(applied(t), t, 0).reshape(psi.shape[t], -1)
        c = np.moveaxis(np.conj(psi), t, 0).reshape(psi.shape[t], -1)
        rho.append(y @ c.T)
    return float(np.log(value)), rho


def logev_longdouble(cm, kinds, enc, ops):
    """logev from a left walk in np.longdouble (np.clongdouble), rescaled at every site"""
    cx = any(np.iscomplexobj(v) for v in list(cm) + list(ops))
    dt = np.dtype(np.clongdouble if cx else np.longdouble)
    cml = [np.asarray(w, dtype=dt) for w in cm]
    opl = [np.asarray(o, dtype=dt) for o in ops]
    encl = np.asarray(np.where(np.isnan(enc), 0, enc), dtype=dt)
    T = len(cm)
    L, lg = np.ones((1, 1), dtype=dt), np.longdouble(0)
    for j in range(T - 1):
        n = _step(L, cml[j], kinds[j], encl[j], opl[j])
        tr = np.trace(n).real
        L, lg = n / tr, lg + np.log(tr)
    r = M.rho_site(L, cml[T - 1], np.ones((1, 1), dtype=dt))
    return lg + np.log(np.trace(opl[T - 1] @ r).real)


def random_operators(N, T, d, cx, rng):
    """Hermitian positive semi-definite d x d matrices at a scale near one"""
    G = rng.standard_normal((N, T, d, d))
    if cx:
        G = G + 1j * rng.standard_normal((N, T, d, d))
    return np.einsum("ntab,ntcb->ntac", G, np.conj(G)) / d


def make_kinds(N, T, rng):
    """One row of each pure kind, a row EXACT everywhere but one GAUSS site, scattered mixtures for the rest (every row of a case with
    fewer than five rows is a scattered mixture)."""
    kind = rng.integers(0, 5, size=(N, T)).astype(np.uint8)
    if N >= 5:
        for k in range(5):
            kind[k] = k
    if N >= 6:
        kind[5] = EXACT
        kind[5, T // 2] = GAUSS
    return kind


def make_case(T, d, chi, C, N, seed, cx=False, label_site=None, ngrid=201, long_chain=False, per_site=False, full_bonds=False):
    """(W, phi, lab, kind, a, b, E_user, x_in, xs, grid_phi): a case of tests/site_cond_ref.make_case with observation kinds.  GAUSS:
    the true value plus noise, sd between 2 and 40 grid spacings; INTERVAL: an interval around the true value, from one grid spacing
    to the whole grid wide (see below), its ends clipped to the grid; OPERATOR: a random positive semi-definite matrix.  Every second row supplies
    the true value at its MISSING sites; phi is NaN wherever the call must not read it."""
    W, phi, lab, x, xs, grid_phi = S.make_case(T, d, chi, C, N, seed, cx=cx, label_site=label_site, ngrid=ngrid, long_chain=long_chain)
    rng = np.random.default_rng(seed + 104729)
    if full_bonds:
        W = M.full_bond_chain(T, d, chi, C, label_site_of(W), cx, rng)
    if per_site:
        sg = np.where(rng.uniform(size=(T, 1, d)) < 0.5, -1.0, 1.0)
        grid_phi = grid_phi[None] * sg
        phi = phi * sg[:, 0][None]
    kind = make_kinds(N, T, rng)
    dx = xs[1] - xs[0]
    sd = dx * np.exp(rng.uniform(np.log(2.0), np.log(40.0), size=(N, T)))
    g, iv = kind == GAUSS, kind == INTERVAL
    # an interval of a few grid values leaves the posterior cdf flat at 0 and 1 on either side, and its outer levels tied between all
    # the grid values of a plateau: such a pair is excused by its margin whatever the seed.  So that a case stays within its one
    # pair in a hundred: one interval per 150 pairs is narrow - the first exactly one grid spacing wide, the others up to eight - and
    # the rest are 16 spacings to the whole grid wide
    width = np.exp(rng.uniform(np.log(16 * dx), np.log(xs[-1] - xs[0]), size=(N, T)))
    narrow = rng.permutation(np.flatnonzero(iv.ravel()))[:(N * T) // 150]
    width.ravel()[narrow] = dx * np.exp(rng.uniform(0.0, np.log(8.0), size=len(narrow)))
    width.ravel()[narrow[:1]] = dx
    lo = np.clip(x - width * rng.uniform(size=(N, T)), xs[0], xs[-1])
    hi = np.clip(lo + width, xs[0], xs[-1])
    a = np.where(g, np.clip(x + sd * rng.standard_normal((N, T)), xs[0], xs[-1]), np.where(iv, lo, 0.0))
    b = np.where(g, sd, np.where(iv, hi, 0.0))
    E_user = random_operators(N, T, d, cx, rng)
    E_user[kind != OPERATOR] = np.nan
    held = (kind == MISSING) & (np.arange(N)[:, None] % 2 == 0)
    valued = (kind == EXACT) | held
    x_in = np.where(valued, x, np.nan)
    phi = np.array(phi)
    phi[~valued] = np.nan
    return W, phi, lab, kind, a, b, E_user, x_in, xs, grid_phi


# (T, d, chi, C, N) of tests/test_gpu_observed.py
SHAPES = [(1, 3, 1, 2, 5), (9, 4, 7, 2, 19), (10, 3, 12, 3, 17), (6, 4, 72, 2, 5)]
LONG = (1000, 4, 8, 2, 2)


@functools.lru_cache(maxsize=None)
def case(T, d, chi, C_, N, cx=False, label="last", ngrid=201, per_site=False):
    """the inputs of a committed case - built once, shared, never modified"""
    seed = 4000 + 31 * T + 7 * d + chi + 3 * C_ + N + ngrid + (1 if cx else 0) + (2 if label == "mid" else 0) + (4 if per_site else 0)
    inp = make_case(T, d, chi, C_, N, seed, cx=cx, label_site=T // 2 if label == "mid" else None, ngrid=ngrid, long_chain=T >= 1000,
                    per_site=per_site, full_bonds=chi > 64)
    for v in list(inp[0]) + list(inp[1:]):
        v.setflags(write=False)
    return inp


def gpu_cases():
    """every (shape, cx, label, ngrid, per_site) tests/test_gpu_observed.py compares with the restatement"""
    out = []
    for shape in SHAPES:
        cxs = (True,) if shape == (10, 3, 12, 3, 17) else (False,)
        for cx in cxs:
            for label, ngrid in (("last", 201), ("mid", 257)):
                out.append((shape, cx, label, ngrid, False))
    out.append(((9, 4, 7, 2, 19), False, "mid", 201, True))
    out += [(LONG, False, "last", 201, False), (LONG, True, "last", 201, False)]
    return out


_LONG = {}


def long_reference(cx):
    """the restatement of the committed T = 1000 case, computed once"""
    if cx not in _LONG:
        W, phi, lab, kind, a, b, E_user, x_in, xs, gp = case(*LONG, cx)
        _LONG[cx] = observed_conditionals_ref(W, phi, lab, kind, a, b, E_user, x_in, xs, gp, LEVELS)
    return _LONG[cx]


def long_logev_distance(cx):
    """the distance of the restatement's logev from the np.longdouble walk on the committed T = 1000 case"""
    W, phi, lab, kind, a, b, E_user, x_in, xs, gp = case(*LONG, cx)
    ref = long_reference(cx)
    dist = 0.0
    for i in range(len(lab)):
        ld = logev_longdouble(class_slice(W, int(lab[i])), kind[i], phi[i], list(ref.E[i]))
        dist = max(dist, float(abs(ld - np.longdouble(ref.logev[i]))))
    return dist
