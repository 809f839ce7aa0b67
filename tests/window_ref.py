"""NumPy restatement of the window conditionals (mpst_window_conditionals), in two forms.  TEST INFRASTRUCTURE ONLY (checker of
tests/test_window_host.py and tests/test_gpu_window.py).

    nll[i][t][w-1] = ln l_c(i; {t, ..., t+w-1}) - ln l_c(i; {}),        c = lab[i],  t + w <= T,  NaN elsewhere

``window_nll_masked`` is that difference itself, both terms from ``marginal_ref.log_marginals_ref`` on the class slice of the series.
``window_nll_local`` is the window-local form the device runs: the rescaled rows of the leave-one-out walk, then per start one
vector recursion (the known values) and one density recursion (``marginal_ref._step``, the values summed out) over the window only,
each width closed with the right row behind it."""
import numpy as np

from tests.marginal_ref import _step, class_slice, gaussian_chain, label_site_of, log_marginals_ref, normalised_chain, random_states

# (T, d, chi, C, N, max_width) -> how the chain is made: the shapes of tests/test_gpu_window.py
SHAPES = {
    "whole-1": dict(T=1, d=3, chi=1, C=2, N=3, mw=1, label_site=0),
    "whole-2": dict(T=2, d=3, chi=3, C=2, N=3, mw=2, label_site=0),
    "whole-2-last": dict(T=2, d=3, chi=3, C=2, N=3, mw=2),
    "ragged-tile": dict(T=6, d=3, chi=4, C=2, N=5, mw=6),
    "second-tile": dict(T=9, d=4, chi=7, C=2, N=19, mw=9),
    "three-tiles": dict(T=12, d=4, chi=12, C=1, N=33, mw=5),
    "complex-mid": dict(T=12, d=3, chi=12, C=3, N=4, mw=6, cx=True, label_site=5),
    "bond-17": dict(T=10, d=4, chi=17, C=2, N=3, mw=4),
    "big-real": dict(T=8, d=4, chi=72, C=2, N=2, mw=4),
    "big-complex": dict(T=8, d=4, chi=72, C=2, N=2, mw=4, cx=True),
    "long-200": dict(T=200, d=4, chi=8, C=2, N=2, mw=4, long_chain=True),
    "long-1000": dict(T=1000, d=4, chi=8, C=2, N=2, mw=3, long_chain=True),
}


def make_case(name, seed=0):
    """(W, phi, lab, max_width) of a named shape: Gaussian site tensors (``normalised_chain`` for the long ones), unit-norm states"""
    s = SHAPES[name]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    T, d, chi, C, N, cx = s["T"], s["d"], s["chi"], s["C"], s["N"], s.get("cx", False)
    if s.get("long_chain"):
        W = normalised_chain(T, d, chi, C, rng, cx)
    else:
        W = gaussian_chain(T, d, chi, C, s.get("label_site", T - 1), cx, rng)
    phi = random_states(N, T, d, cx, rng)
    lab = (np.arange(N) % C).astype(np.int32)
    return W, phi, lab, s["mw"]


def walk_rows(cm, enc):
    """l[t] = l~_{t-1} and r[t] = r~_t (r[T] = 1) of one series: l_j = l_{j-1} M_j, r_j = M_j r_{j+1}, each divided by its largest
    magnitude as the device's walk does"""
    T = len(cm)
    M = [np.einsum("asb,s->ab", cm[j], np.conj(enc[j])) for j in range(T)]
    l = [np.ones(1, dtype=M[0].dtype)]
    for j in range(T):
        v = l[-1] @ M[j]
        l.append(v / np.abs(v).max())
    r = [np.ones(1, dtype=M[0].dtype)]
    for j in range(T - 1, -1, -1):
        v = M[j] @ r[-1]
        r.append(v / np.abs(v).max())
    return M, l, r[::-1]


def window_nll_local(W, phi, lab, max_width, pairs=None):
    """(N, T, max_width) by the window-local recursion; ``pairs``: only these (i, t), the rest NaN"""
    N, T = phi.shape[:2]
    out = np.full((N, T, max_width), np.nan)
    todo = [(i, t) for i in range(N) for t in range(T)] if pairs is None else list(pairs)
    rows = {}
    for i, t in todo:
        cm = class_slice(W, int(lab[i]))
        if i not in rows:
            rows[i] = walk_rows(cm, phi[i])
        M, l, r = rows[i]
        x = l[t] / np.linalg.norm(l[t])
        E = np.outer(x, np.conj(x))
        lgx = lgE = 0.0
        for k in range(1, min(max_width, T - t) + 1):
            j = t + k - 1
            x = x @ M[j]
            n2 = float(np.vdot(x, x).real)
            if n2 > 0.0:
                lgx += np.log(n2)
                x = x / np.sqrt(n2)
            E = _step(E, cm[j], None, True)
            tr = float(np.trace(E).real)
            if not (tr > 0.0 and np.isfinite(tr)):
                break
            lgE += np.log(tr)
            E = E / tr
            q = float((r[j + 1] @ E @ np.conj(r[j + 1])).real)
            if not (q > 0.0 and np.isfinite(q)):
                break
            den = float(np.abs(x @ r[j + 1]) ** 2) if n2 > 0.0 else 0.0
            out[i, t, k - 1] = np.inf if den == 0.0 else (np.log(q) + lgE) - (np.log(den) + lgx)
    return out


def window_nll_masked(W, phi, lab, max_width, pairs=None):
    """(N, T, max_width) as log_marginals(window masked) - log_marginals(complete), each series under its own class slice"""
    N, T = phi.shape[:2]
    out = np.full((N, T, max_width), np.nan)
    todo = [(i, t) for i in range(N) for t in range(T)] if pairs is None else list(pairs)
    ls = label_site_of(W)
    for i in sorted({i for i, _ in todo}):
        starts = [t for ii, t in todo if ii == i]
        Wc = [w[..., int(lab[i])][..., None] if j == ls else w for j, w in enumerate(W)]
        wins = [(t, w) for t in starts for w in range(1, min(max_width, T - t) + 1)]
        mask = np.zeros((len(wins) + 1, T), dtype=bool)
        for n, (t, w) in enumerate(wins):
            mask[n + 1, t:t + w] = True
        lm = log_marginals_ref(Wc, np.broadcast_to(phi[i], (len(wins) + 1,) + phi[i].shape), mask)[:, 0]
        for n, (t, w) in enumerate(wins):
            out[i, t, w - 1] = lm[n + 1] - lm[0]
    return out


def expected_nan(N, T, max_width):
    """where the definition has no window: t + w > T"""
    t, w = np.arange(T)[:, None], np.arange(1, max_width + 1)[None, :]
    return np.broadcast_to(t + w > T, (N, T, max_width))
