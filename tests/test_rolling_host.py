"""The rolling-origin forecasts without a GPU: the restatement (tests/rolling_ref.py) against the full amplitude tensor, the table
recursion of the kernels written in NumPy against the restatement, the identities the kernels lean on, and the NumPy
evaluators of mpstime.jl_amd/rolling.py on hand-made arrays."""
import numpy as np
import pytest

from mpstime_jl_amd import prefix, rolling
from tests import margcond_ref as M
from tests import marginal_ref as MR
from tests import rolling_ref as RR
from tests import site_cond_ref as S
from tests.prefix_ref import prefix_log_marginals_ref, suffix_mask

NAN = np.nan
# (T, d, chi, C, cx, label site): the three chains the recursion was first checked on
CHAINS = [(6, 3, 5, 2, False, None), (7, 4, 7, 3, True, 3), (5, 2, 4, 2, False, 0)]


# ---- the recursion of the kernels, unscaled -------------------------------------------------------------------------------------------
def env_tables(cm):
    """G[t], t = 0 .. T: the density recursion from the right end through the sites T-1 .. t, all summed out"""
    T = len(cm)
    G = [None] * T + [np.ones((1, 1), dtype=cm[0].dtype)]
    for t in range(T - 1, -1, -1):
        G[t] = sum(cm[t][:, s, :] @ G[t + 1] @ np.conj(cm[t][:, s, :]).T for s in range(cm[t].shape[1]))
    return G


def chain_tables(cm, G, H):
    """K[(t, u)][s][s']: K^{u,u} = W_u[s] G^{u+1} W_u[s']^H, K^{t,u} = sum_q W_t[q] K^{t+1,u} W_t[q]^H for t = u-1 .. u-H+1"""
    T, d = len(cm), cm[0].shape[1]
    K = {}
    for u in range(T):
        K[u, u] = [[cm[u][:, s, :] @ G[u + 1] @ np.conj(cm[u][:, sp, :]).T for sp in range(d)] for s in range(d)]
        for t in range(u - 1, max(u - H, -1), -1):
            K[t, u] = [[sum(cm[t][:, q, :] @ K[t + 1, u][s][sp] @ np.conj(cm[t][:, q, :]).T for q in range(d)) for sp in range(d)] for s in range(d)]
    return K


def rows(cm, enc):
    """x_t, t = 0 .. T-1: the row walk through the known sites 0 .. t-1"""
    x = [np.ones(1, dtype=cm[0].dtype)]
    for j in range(len(cm) - 1):
        x.append(x[-1] @ np.einsum("s,asb->ab", np.conj(enc[j]), cm[j]))
    return x


def recursion_rho(W, phi, c, H):
    """(N, T, H, d, d) rho_c of every triple from the tables, zero beyond the chain"""
    cm = MR.class_slice(W, c)
    N, T, d = phi.shape
    G = env_tables(cm)
    K = chain_tables(cm, G, H)
    out = np.zeros((N, T, H, d, d), dtype=np.result_type(cm[0].dtype, phi.dtype))
    for i in range(N):
        x = rows(cm, phi[i])
        for t in range(T):
            for h in range(min(H, T - t)):
                Kt = K[t, t + h]
                out[i, t, h] = [[x[t] @ Kt[s][sp] @ np.conj(x[t]) for sp in range(d)] for s in range(d)]
    return out, G, K


def case(T, d, chi, C, cx, ls, N=3, seed=11):
    return S.make_case(T, d, chi, C, N, seed, cx=cx, label_site=ls, ngrid=41)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,d,cx,ls", [(5, 3, False, None), (6, 4, True, 2), (4, 2, False, 0)])
def test_the_restatement_is_the_amplitude_tensor(T, d, cx, ls):
    assert d ** T <= 4096
    W, phi, lab, x, xs, gp = case(T, d, 5, 2, cx, ls)
    H = T
    r = RR.rolling_forecasts_ref(W, phi, lab, x, xs, gp, H, (0.05, 0.5, 0.95))
    m = RR.rolling_forecasts_ref(W, phi, np.full(len(lab), -1), x, xs, gp, H, (0.05, 0.5, 0.95))
    assert r.done.sum() == T * (T + 1) // 2 == m.done.sum()
    for i in range(len(lab)):
        for t in range(T):
            miss = suffix_mask(1, T, t)[0]
            for h in range(T - t):
                dense = [M.dense_rho(MR.class_slice(W, c), phi[i], miss, t + h) for c in range(2)]
                own = dense[int(lab[i])]
                # a labelled row: the scaled walks leave a factor, the normalised rho is the same
                assert rel(r.rho[i, t, h] / np.trace(r.rho[i, t, h]).real, own / np.trace(own).real) <= 1e-12
                # a mixture row: the classes at their stored scale
                assert rel(m.rho[i, t, h], dense[0] + dense[1]) <= 1e-12
    assert np.all(np.isnan(r.nll[:, ~r.done])) and not np.any(np.isnan(r.nll[:, r.done]))
    assert not np.any(np.isnan(m.median[:, m.done])) and not np.any(np.isnan(m.quantiles[:, m.done]))


@pytest.mark.parametrize("T,d,chi,C,cx,ls", CHAINS)
def test_the_table_recursion_is_the_restatement(T, d, chi, C, cx, ls):
    W, phi, lab, x, xs, gp = case(T, d, chi, C, cx, ls)
    H = min(T, 4)
    N = phi.shape[0]
    total = 0.0
    worst = 0.0
    for c in range(C):
        rho, G, K = recursion_rho(W, phi, c, H)
        ref = RR.rolling_forecasts_ref(W, phi, np.full(N, c), x, xs, gp, H, ())
        # the restatement's rho of a labelled row is scaled: compare what the outputs are made of, rho at trace one
        for t in range(T):
            for h in range(min(H, T - t)):
                for i in range(N):
                    a, b = rho[i, t, h], ref.rho[i, t, h]
                    worst = max(worst, rel(a / np.trace(a).real, b / np.trace(b).real))
        total = total + rho
        # sum_s K^{t,u}[s, s] = G^t for every u
        for (t, u), Kt in K.items():
            assert rel(sum(Kt[s][s] for s in range(d)), G[t]) <= 1e-12
            for s in range(d):
                for sp in range(s):
                    assert rel(Kt[s][sp], np.conj(Kt[sp][s]).T) <= 1e-12
    mix = RR.rolling_forecasts_ref(W, phi, np.full(N, -1), x, xs, gp, H, ())
    done = mix.done
    print(f"largest relative deviation of rho {worst:.1e}, of the class sum {rel(total[:, done], mix.rho[:, done]):.1e}")
    assert worst <= 1e-12 and rel(total[:, done], mix.rho[:, done]) <= 1e-12


@pytest.mark.parametrize("T,d,chi,C,cx,ls", CHAINS)
def test_the_trace_of_the_class_sum_gives_the_prefix_posteriors(T, d, chi, C, cx, ls):
    W, phi, lab, x, xs, gp = case(T, d, chi, C, cx, ls)
    H = 3
    tr = np.stack([np.einsum("nthss->nth", recursion_rho(W, phi, c, H)[0]).real for c in range(C)], axis=-1)      # (N, T, H, C)
    post = prefix.posteriors_from(prefix_log_marginals_ref(W, phi))                                              # (N, T + 1, C)
    for t in range(T):
        for h in range(min(H, T - t)):
            assert np.abs(tr[:, t, h] / tr[:, t, h].sum(axis=1, keepdims=True) - post[:, t]).max() <= 1e-12


def test_the_weighted_mixture_is_the_unscaled_one():
    W, phi, lab, x, xs, gp = case(7, 4, 7, 3, True, 3)
    sites = [2, 3, 4, 6]
    for i in range(3):
        a, b = RR.mixture_rho(W, phi[i], 2, sites), RR.mixture_rho(W, phi[i], 2, sites, weighted=True)
        for ra, rb in zip(a, b):
            assert rel(ra / np.trace(ra).real, rb / np.trace(rb).real) <= 1e-12


@pytest.mark.parametrize("T,d,chi,C,cx,ls", CHAINS)
def test_the_restatement_is_the_whole_call_on_every_suffix_mask(T, d, chi, C, cx, ls):
    """rolling_forecasts_ref finishes only the sites it reads: bit for bit marginal_conditionals_ref on the suffix mask of every origin"""
    W, phi, lab, x, xs, gp = case(T, d, chi, C, cx, ls)
    levels = (0.05, 0.5, 0.95)
    H = 3
    r = RR.rolling_forecasts_ref(W, phi, lab, x, xs, gp, H, levels)
    for t in range(T):
        whole = M.marginal_conditionals_ref(W, phi, lab, suffix_mask(len(lab), T, t), x, xs, gp, levels)
        for h in range(min(H, T - t)):
            u = t + h
            for got, want in ((r.nll, whole.sc.nll), (r.pit, whole.sc.pit), (r.median, whole.sc.median), (r.err, whole.sc.err), (r.mean, whole.mean),
                              (r.quantiles, whole.sc.quantiles), (r.rho, whole.rho), (r.excused, whole.excused)):
                assert np.array_equal(got[:, t, h], want[:, u])


# ---- the evaluators ---------------------------------------------------------------------------------------------------------------------
# one series, T = 3, H = 2: x = (1, 2, 4); forecasts [origin][horizon - 1], the corner (2, 2) beyond the series
X = np.array([[1.0, 2.0, 4.0]])
POINT = np.array([[[1.5, 1.0], [2.0, 7.0], [3.0, NAN]]])


def test_the_triangle_and_the_targets():
    assert rolling.valid_forecast_triangle(3, 2).tolist() == [[True, True], [True, True], [True, False]]
    assert rolling.valid_forecast_triangle(2, 2).tolist() == [[True, True], [True, False]]
    assert np.array_equal(rolling.targets_of(X, 2), [[[1.0, 2.0], [2.0, 4.0], [4.0, NAN]]], equal_nan=True)


def test_errors_by_horizon():
    mae, rmse = rolling.horizon_errors_from(POINT, X)
    # horizon 1: |1.5 - 1|, |2 - 2|, |3 - 4|; horizon 2: |1 - 2|, |7 - 4|
    assert np.allclose(mae, [1.5 / 3, 2.0]) and np.allclose(rmse, [np.sqrt(1.25 / 3), np.sqrt(5.0)])
    mae, rmse = rolling.horizon_errors_from(POINT, X, min_origin=1)
    assert np.allclose(mae, [0.5, 3.0]) and np.allclose(rmse, [np.sqrt(0.5), 3.0])
    mae, _ = rolling.horizon_errors_from(POINT, X, min_origin=2)
    assert mae[0] == 1.0 and np.isnan(mae[1])                                   # no origin from 2 on has a second horizon
    # a value in the corner never counts, whatever it holds; a NaN inside the triangle is left out
    full = np.array(POINT)
    full[0, 2, 1] = 1e9
    assert np.allclose(rolling.horizon_errors_from(full, X)[0], [0.5, 2.0])
    holed = np.array(POINT)
    holed[0, 0, 0] = NAN
    assert np.allclose(rolling.horizon_errors_from(holed, X)[0], [0.5, 2.0])
    with pytest.raises(ValueError):
        rolling.horizon_errors_from(POINT, X, min_origin=3)
    with pytest.raises(ValueError):
        rolling.horizon_errors_from(POINT[:, :, :1].reshape(1, 1, 3), X[:, :1])     # H > T


def test_coverage_and_pinball_of_a_known_case():
    lo, hi = POINT - 0.75, POINT + 0.75
    # inside: horizon 1: 1 (0.5 off), 2 (0 off), not 4 (1 off); horizon 2: not 2 (1 off), not 4 (3 off)
    assert np.allclose(rolling.interval_coverage_from(lo, hi, X), [2.0 / 3.0, 0.0])
    assert np.allclose(rolling.interval_coverage_from(lo, hi, X, min_origin=1), [0.5, 0.0])
    q = np.stack([POINT, POINT], axis=-1)
    pin = rolling.pinball_loss_from([0.5, 0.9], q, X)
    # x - q: horizon 1: -0.5, 0, 1; horizon 2: 1, -3.  tau = 0.5: half the absolute error.  tau = 0.9: 0.9 d above, 0.1 |d| below
    assert pin.shape == (2, 2) and np.allclose(pin[:, 0], [0.25, 1.0])
    assert np.allclose(pin[:, 1], [(0.05 + 0.0 + 0.9) / 3, (0.9 + 0.3) / 2])
    with pytest.raises(ValueError):
        rolling.pinball_loss_from([0.5], q, X)
    with pytest.raises(ValueError):
        rolling.interval_coverage_from(lo, hi[:, :2], X)
