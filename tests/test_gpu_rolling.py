"""mpst_rolling_forecasts on the device against the NumPy restatement (tests/rolling_ref.py: marginal_conditionals_ref on the suffix mask
of every origin), against mpst_marginal_conditionals and mpst_site_conditionals where their questions coincide, and end to end through
rolling_forecasts / backtest.

Bounds are the project's: nll 1e-10, pit 1e-12, mean 1e-12 * max|grid_x|; median, WMAD and levels EQUAL wherever the
restatement's selection margin exceeds 1e-9, and at most 1 % of a case's triples excused by it.  The chain of a thousand sites takes
the long-chain allowances: nll 1e-8 (DESIGN 24 at T = 1000), pit 1e-10 and mean 1e-10 * max|grid_x| (the T = 10 bounds times T / 10,
as DESIGN 18)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import marginal, rolling
from mpstime_jl_amd.conditionals import marginal_conditionals_model
from tests import margcond_ref as M
from tests import marginal_ref as MR
from tests import rolling_ref as RR
from tests import site_cond_ref as S
from tests.prefix_ref import suffix_mask

pytestmark = pytest.mark.gpu

LEVELS = (0.05, 0.5, 0.95)
NLL_TOL, PIT_TOL, MEAN_TOL = 1e-10, 1e-12, 1e-12
LONG_ORIGINS = tuple(range(0, 1000, 125)) + (992, 999)
# name -> (T, d, chi, C, N, H, seed, complex, label site (None: last), variant, origins restated (None: all))
CASES = {
    "smallest": (1, 3, 1, 2, 3, 1, 11, False, None, "", None),
    "t9_real_last": (9, 4, 7, 2, 19, 4, 12, False, None, "", None),
    "t9_real_at4": (9, 4, 7, 2, 19, 4, 12, False, 4, "", None),
    "t9_real_at0": (9, 4, 7, 2, 19, 4, 12, False, 0, "", None),
    "t9_complex_last": (9, 4, 7, 2, 19, 4, 12, True, None, "", None),
    "t9_complex_at4": (9, 4, 7, 2, 19, 4, 12, True, 4, "", None),
    "t9_complex_at0": (9, 4, 7, 2, 19, 4, 12, True, 0, "", None),
    "t9_real_grid_per_site": (9, 4, 7, 2, 19, 4, 12, False, None, "per_site", None),
    "t10_real_last": (10, 3, 12, 3, 17, 10, 13, False, None, "", None),
    "t10_complex_at5": (10, 3, 12, 3, 17, 10, 13, True, 5, "", None),
    "chi72_real": (6, 4, 72, 2, 5, 3, 14, False, None, "full_bonds", None),
    "chi72_complex_at2": (6, 4, 72, 2, 5, 3, 14, True, 2, "full_bonds", None),
    "chi128": (6, 6, 128, 3, 1, 6, 15, False, None, "", (0, 2, 3, 5)),
    "long_real": (1000, 4, 8, 2, 2, 8, 11, False, None, "long", LONG_ORIGINS),
    "long_complex": (1000, 4, 8, 2, 2, 8, 11, True, None, "long", LONG_ORIGINS),
}


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(W, phi, lab, x, xs, grid_phi) - built once, shared by the tests below, never modified"""
    T, d, chi, Cn, N, H, seed, cx, ls, variant, _ = CASES[name]
    W, phi, lab, x, xs, gp = S.make_case(T, d, chi, Cn, N, seed, cx=cx, label_site=ls, long_chain=variant == "long")
    rng = np.random.default_rng(seed + 7919)
    if variant == "full_bonds":
        W = M.full_bond_chain(T, d, chi, Cn, MR.label_site_of(W), cx, rng)
    if variant == "per_site":       # one table per site: the shared one, each site's states under its own sign pattern
        sg = np.where(rng.uniform(size=(T, 1, d)) < 0.5, -1.0, 1.0)
        gp = gp[None] * sg
        phi = phi * sg[:, 0][None]
    for a in list(W) + [phi, lab, x, xs, gp]:
        a.setflags(write=False)
    return W, phi, lab, x, xs, gp


def labels_of(name, mode):
    lab = inputs(name)[2]
    if mode == "label":
        return lab
    if mode == "mixture":
        return np.full(len(lab), -1, dtype=np.int32)
    return np.where(np.arange(len(lab)) % 2 == 1, -1, lab).astype(np.int32)


@functools.lru_cache(maxsize=None)
def restated(name, mode):
    """the restatement of a case with all rows labelled or all rows under the mixture - computed once"""
    W, phi, lab, x, xs, gp = inputs(name)
    H, variant, origins = CASES[name][5], CASES[name][9], CASES[name][10]
    return RR.rolling_forecasts_ref(W, phi, labels_of(name, mode), x, xs, gp, H, LEVELS, origins=origins, weighted=variant == "long")


def run(eng, name, lab, x="given", levels=LEVELS):
    W, phi, _, xv, xs, gp = inputs(name)
    return eng.rolling_model(W, phi, lab, CASES[name][5], xv if x == "given" else None, xs, gp, levels=levels)


def check_against(name, got, refs, rows_of, tols):
    """got: (nll, pit, med, err, mean, q); refs: [(restatement, rows it speaks for)]"""
    nll, pit, med, err, mean, q = got[:6]
    T, H = CASES[name][0], CASES[name][5]
    tri = rolling.valid_forecast_triangle(T, H)
    for a in (nll, pit, med, err, mean, q):
        assert a.shape[:3] == (nll.shape[0], T, H)
        assert np.all(np.isnan(a[:, ~tri])) and not np.any(np.isnan(a[:, tri]))         # the corner exactly, nothing inside
    worst = dict(nll=0.0, pit=0.0, mean=0.0)
    excused = total = 0
    for ref, rows in refs:
        at = ref.done
        assert np.array_equal(at & tri, at) and at.any()
        r = np.asarray(rows)
        if not len(r):
            continue
        worst["nll"] = max(worst["nll"], np.abs(nll[r][:, at] - ref.nll[r][:, at]).max())
        worst["pit"] = max(worst["pit"], np.abs(pit[r][:, at] - ref.pit[r][:, at]).max())
        worst["mean"] = max(worst["mean"], np.abs(mean[r][:, at] - ref.mean[r][:, at]).max())
        ok = ~ref.excused[r][:, at]
        excused += int((~ok).sum())
        total += ok.size
        assert np.array_equal(med[r][:, at][ok], ref.median[r][:, at][ok])
        assert np.array_equal(err[r][:, at][ok], ref.err[r][:, at][ok])
        assert np.array_equal(q[r][:, at][ok], ref.quantiles[r][:, at][ok])
    print(f"{name} {rows_of}: |d nll| {worst['nll']:.2e}  |d pit| {worst['pit']:.2e}  |d mean| {worst['mean']:.2e}  excused {excused} of {total}")
    assert worst["nll"] <= tols[0] and worst["pit"] <= tols[1] and worst["mean"] <= tols[2]
    assert excused <= 0.01 * total


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(eng, name):
    """three calls: all rows labelled, all rows under the class mixture, the two mixed - whose rows give the bits of the other two"""
    W, phi, lab, x, xs, gp = inputs(name)
    N, T = x.shape
    long = CASES[name][9] == "long"
    tols = (1e-8, 1e-10, 1e-10) if long else (NLL_TOL, PIT_TOL, MEAN_TOL * np.abs(xs).max())
    if name == "chi128":
        assert max(t.shape[2] for t in W) == 128
    every = np.arange(N)
    a = run(eng, name, labels_of(name, "label"))
    check_against(name, a, [(restated(name, "label"), every)], "labelled", tols)
    b = run(eng, name, labels_of(name, "mixture"))
    check_against(name, b, [(restated(name, "mixture"), every)], "mixture", tols)
    mixed = labels_of(name, "mixed")
    c = run(eng, name, mixed)
    check_against(name, c, [(restated(name, "label"), every[mixed >= 0]), (restated(name, "mixture"), every[mixed < 0])], "mixed", tols)
    for k in range(6):
        assert np.array_equal(c[k][mixed >= 0], a[k][mixed >= 0], equal_nan=True)
        assert np.array_equal(c[k][mixed < 0], b[k][mixed < 0], equal_nan=True)


BASE = "t9_complex_at4"


def test_one_class_is_its_own_mixture(eng):
    W, phi, lab, x, xs, gp = S.make_case(5, 3, 4, 1, 4, 11)
    a = eng.rolling_model(W, phi, lab, 3, x, xs, gp, levels=LEVELS)
    b = eng.rolling_model(W, phi, np.full(4, -1, dtype=np.int32), 3, x, xs, gp, levels=LEVELS)
    assert np.all(lab == 0) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in range(6))
    assert np.all(np.isfinite(a[0][:, rolling.valid_forecast_triangle(5, 3)]))


@pytest.mark.parametrize("name", ["t9_real_last", BASE, "t9_real_grid_per_site"])
def test_the_last_origins_are_the_other_queries(eng, name):
    """origin T - H is mpst_marginal_conditionals on the last-H mask with the true values supplied; [i][T-1][0] is the leave-one-out
    conditional of mpst_site_conditionals at the last site"""
    W, phi, lab, x, xs, gp = inputs(name)
    N, T = x.shape
    H = CASES[name][5]
    nll, pit, med, err, mean, q, _ = run(eng, name, lab)
    ref = restated(name, "label")
    mc = marginal_conditionals_model(eng, W, phi, lab, suffix_mask(N, T, T - H), x, xs, gp, levels=LEVELS)
    for h in range(H):
        u, ok = T - H + h, ~ref.excused[:, T - H, h]
        assert np.abs(nll[:, T - H, h] - mc.nll[:, u]).max() <= NLL_TOL and np.abs(pit[:, T - H, h] - mc.pit[:, u]).max() <= PIT_TOL
        assert np.abs(mean[:, T - H, h] - mc.mean[:, u]).max() <= MEAN_TOL * np.abs(xs).max()
        assert np.array_equal(med[:, T - H, h][ok], mc.median[:, u][ok]) and np.array_equal(err[:, T - H, h][ok], mc.err[:, u][ok])
        assert np.array_equal(q[:, T - H, h][ok], mc.quantiles[:, u][ok])
    snll, spit, smed, serr, sq, _ = eng.site_conditionals(W, phi, lab, x, xs, gp, levels=LEVELS)
    ok = ~ref.excused[:, T - 1, 0]
    assert np.abs(nll[:, T - 1, 0] - snll[:, T - 1]).max() <= NLL_TOL and np.abs(pit[:, T - 1, 0] - spit[:, T - 1]).max() <= PIT_TOL
    assert np.array_equal(med[:, T - 1, 0][ok], smed[:, T - 1][ok]) and np.array_equal(err[:, T - 1, 0][ok], serr[:, T - 1][ok])
    assert np.array_equal(q[:, T - 1, 0][ok], sq[:, T - 1][ok])


@pytest.mark.parametrize("mode", ["label", "mixture"])
def test_origin_zero_knows_nothing_of_the_series(eng, mode):
    lab = labels_of(BASE, mode)
    _, _, med, err, mean, q, _ = run(eng, BASE, lab)
    for c in np.unique(lab):
        r = np.flatnonzero(lab == c)
        assert len(r) > 1
        for a in (med, err, mean, q):
            assert all(np.array_equal(a[i, 0], a[r[0], 0]) for i in r)


def test_a_permutation_of_the_series_permutes_the_bits(eng):
    W, phi, lab, x, xs, gp = inputs(BASE)
    mixed = labels_of(BASE, "mixed")
    perm = np.random.default_rng(3).permutation(len(lab))
    a = run(eng, BASE, mixed)
    b = eng.rolling_model(W, phi[perm], mixed[perm], CASES[BASE][5], x[perm], xs, gp, levels=LEVELS)
    assert all(np.array_equal(a[k][perm], b[k], equal_nan=True) for k in range(6))


def test_two_calls_give_equal_bits(eng):
    a, b = run(eng, BASE, labels_of(BASE, "mixed")), run(eng, BASE, labels_of(BASE, "mixed"))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in range(6))


@functools.lru_cache(maxsize=None)
def cut_case():
    """N = 40, T = 9, d = 4, chi = 16, C = 2, H = 9: the sums of tests/test_rolling_plan.py (CUT)"""
    W, phi, lab, x, xs, gp = S.make_case(9, 4, 16, 2, 40, 12)
    assert max(t.shape[2] for t in W) == 16
    return W, phi, np.where(np.arange(40) % 3 == 1, -1, lab).astype(np.int32), x, xs, gp


@pytest.mark.parametrize("gb,series_blocks,target_blocks", [("0.001", 3, 9), ("0.004", 1, 2)])
def test_blocks_do_not_change_the_result(eng, monkeypatch, gb, series_blocks, target_blocks):
    """With the five outputs and three levels a series brings 18 000 bytes, a target 368 640 and the fixed part 407 712
    (tests/test_rolling_plan.py works the sums out).  Under 0.001 GB = 1 073 741 bytes a block of tables holds one target and 16 series
    fit: N = 40 in blocks of 16, 16 and 8, nine blocks of targets each.  Under 0.004 GB all 40 series fit and a block of tables holds
    five targets: two blocks.  The bits of one block."""
    W, phi, lab, x, xs, gp = cut_case()
    one = eng.rolling_model(W, phi, lab, 9, x, xs, gp, levels=LEVELS)
    info = eng.impute_info()
    assert (info["env_workgroups"], info["chains"]) == (1, 1)
    monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", gb)
    cut = eng.rolling_model(W, phi, lab, 9, x, xs, gp, levels=LEVELS)
    info = eng.impute_info()
    assert (info["env_workgroups"], info["chains"]) == (series_blocks, target_blocks)
    tri = rolling.valid_forecast_triangle(9, 9)
    assert np.all(np.isfinite(one[0][:, tri])) and all(np.array_equal(one[k], cut[k], equal_nan=True) for k in range(6))


@pytest.mark.parametrize("mode", ["label", "mixture"])
def test_a_vanishing_state_is_nan_from_the_next_origin_on(eng, mode):
    """the state of series 2 at site 3 is zero - a valid input: NaN at that series' origins >= 4, the bits of everything else kept.
    (Its nll at the target 3 is +inf, the density of a state of norm zero.)"""
    W, phi, _, x, xs, gp = inputs(BASE)
    lab = labels_of(BASE, mode)
    T, H = CASES[BASE][0], CASES[BASE][5]
    zeroed = np.array(phi)
    zeroed[2, 3] = 0.0
    a = run(eng, BASE, lab)
    b = eng.rolling_model(W, zeroed, lab, H, x, xs, gp, levels=LEVELS)
    tri = rolling.valid_forecast_triangle(T, H)
    gone = tri & (np.arange(T)[:, None] >= 4)
    at3 = tri & (np.arange(T)[:, None] + np.arange(H)[None, :] == 3)
    others = np.arange(len(lab)) != 2
    for k in range(6):
        assert np.all(np.isnan(b[k][2][gone])) and not np.any(np.isnan(b[k][2][tri & ~gone]))
        assert np.array_equal(a[k][others], b[k][others], equal_nan=True)
        keep = tri & ~gone & (~at3 if k == 0 else True)
        assert np.array_equal(a[k][2][keep], b[k][2][keep])
    assert np.all(np.isposinf(b[0][2][at3]))


def test_without_the_values_there_is_no_pit(eng):
    a = run(eng, BASE, labels_of(BASE, "mixed"))
    b = run(eng, BASE, labels_of(BASE, "mixed"), x=None)
    assert b[1] is None and all(np.array_equal(a[k], b[k], equal_nan=True) for k in (0, 2, 3, 4, 5))
    c = run(eng, BASE, labels_of(BASE, "mixed"), levels=None)
    assert c[5] is None and all(np.array_equal(a[k], c[k], equal_nan=True) for k in range(5))


def test_argument_errors(eng):
    W, phi, lab, x, xs, gp = inputs("t9_real_last")
    lib, dp, L = eng.lib, C.POINTER(C.c_double), mt._lib
    N, T = x.shape
    H = 4
    want = run(eng, "t9_real_last", lab)
    before = eng.impute_info()
    lv = np.array(LEVELS)
    o = L.SiteCondOpts(0, 1, 3, 0, lv.ctypes.data_as(dp))
    outs = [np.zeros((N, T, H)) for _ in range(5)] + [np.zeros((N, T, H, 3))]
    xc, gxc, gpc = np.ascontiguousarray(x), np.ascontiguousarray(xs), np.ascontiguousarray(gp)

    def call(m, H=H, labels=lab, x=xc, outs=outs, model=True):
        li = np.ascontiguousarray(labels, dtype=np.int32)
        m.label_idx = li.ctypes.data_as(C.POINTER(C.c_int32))
        ptr = [None if a is None else a.ctypes.data_as(dp) for a in outs]
        return lib.mpst_rolling_forecasts(eng.ctx, C.byref(m) if model else None, H, None if x is None else x.ctypes.data_as(dp), gxc.ctypes.data_as(dp),
                                          C.c_void_p(gpc.ctypes.data), len(gxc), C.byref(o), *ptr, None)
    m, keep = marginal.model_struct(W, phi)
    bad = np.array(lab)
    assert call(m, H=0) == L.MPST_ERR_INVALID and call(m, H=T + 1) == L.MPST_ERR_INVALID
    bad[1] = -2
    assert call(m, labels=bad) == L.MPST_ERR_INVALID
    bad[1] = 2
    assert call(m, labels=bad) == L.MPST_ERR_INVALID
    assert call(m, model=False) == L.MPST_ERR_INVALID and call(m, outs=[None] * 6) == L.MPST_ERR_INVALID
    assert call(m, x=None) == L.MPST_ERR_INVALID                            # pit_out without the values
    m32, keep32 = marginal.model_struct(W, phi, "f32")
    assert call(m32) == L.MPST_ERR_UNSUPPORTED
    assert eng.impute_info() == before                                      # a rejected call leaves the context as it was
    # ... and the call after them succeeds with the bits of the first
    assert call(m) == 0
    assert all(np.array_equal(outs[k], want[k], equal_nan=True) for k in range(6))
    del keep, keep32
    rng = np.random.default_rng(2)
    enc = mt.model_encoding("Legendre_No_Norm")

    def refused(Wb, d, Cn):
        xb = rng.uniform(-0.9, 0.9, (2, len(Wb)))
        pb = np.asarray(enc.encode(xb.ravel(), d)).reshape(2, len(Wb), d)
        with pytest.raises(mt.MPSTError) as ei:
            eng.rolling_model(Wb, pb, np.zeros(2, dtype=np.int32), 2, xb, xs, np.asarray(enc.encode(xs, d)))
        return ei.value.code
    assert refused(MR.gaussian_chain(3, 2, 2, 17, 2, False, rng), 2, 17) == L.MPST_ERR_UNSUPPORTED            # C > 16
    assert refused(MR.gaussian_chain(3, 17, 2, 2, 2, False, rng), 17, 2) == L.MPST_ERR_UNSUPPORTED            # d > 16
    wide = [rng.standard_normal(s) / 16.0 for s in ((1, 2, 129), (129, 2, 129), (129, 2, 1, 2))]
    assert refused(wide, 2, 2) == L.MPST_ERR_UNSUPPORTED                                                      # chi_max > 128
    again = run(eng, "t9_real_last", lab)
    assert all(np.array_equal(again[k], want[k], equal_nan=True) for k in range(6))


def test_phases_are_the_tables_and_the_grid(eng):
    got = run(eng, BASE, labels_of(BASE, "mixed"))
    first, grid = eng.impute_phases()
    assert first > 0.0 and grid > 0.0 and first + grid <= got[6] * (1.0 + 1e-6) + 1e-6


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E_H, E2E_T = 6, 24


@functools.lru_cache(maxsize=None)
def problem():
    """two trendy_sine classes at phase zero (periods in (12, 15) and in (16, 19)), T = 24: 80 training and 8 test series"""
    rng = np.random.default_rng(5)

    def draw(n):
        y = np.arange(n) % 2
        X = np.stack([mt.trendy_sine(E2E_T, 1, period=rng.uniform(12.0, 15.0) if c == 0 else rng.uniform(16.0, 19.0),
                                     slope=rng.choice([-3.0, 0.0, 3.0]), phase=0.0)[0][0] for c in y])
        return X + 0.1 * rng.standard_normal(X.shape), y
    Xtr, ytr = draw(80)
    Xte, yte = draw(8)
    trained, _, _ = mt.fitMPS(Xtr, ytr, Xte, yte, mt.MPSOptions(chi_max=8, nsweeps=3, verbosity=-1, d=4))
    return mt.init_imputation_problem(trained, Xte, yte, dx=0.01, verbosity=0)


def test_end_to_end(eng):
    from mpstime_jl_amd.imputation import _scaled_instances
    imp = problem()
    N, T = imp.X_test.shape
    tri = rolling.valid_forecast_triangle(T, E2E_H)
    for classes in ("label", "mixture"):
        f = mt.rolling_forecasts(imp, E2E_H, classes=classes, engine=eng)
        assert isinstance(f, mt.RollingForecasts) and f.median.shape == (N, T, E2E_H) and f.levels.shape == (N, T, E2E_H, 2) and f.x.shape == (N, T)
        for a in (f.median, f.mean, f.wmad, f.nll, f.pit, f.levels):
            assert np.all(np.isfinite(a[:, tri])) and np.all(np.isnan(a[:, ~tri]))
        assert np.all(f.levels[:, tri, 0] <= f.median[:, tri]) and np.all(f.median[:, tri] <= f.levels[:, tri, 1])     # raw units
        assert np.allclose(f.x, imp.X_test, rtol=0, atol=1e-9 * np.abs(imp.X_test).max())
        assert np.all((f.pit[:, tri] >= 0.0) & (f.pit[:, tri] <= 1.0))
        bt = mt.backtest(imp, E2E_H, min_origin=4, classes=classes, engine=eng)
        assert bt.mae.shape == bt.rmse.shape == bt.coverage.shape == bt.nll.shape == (E2E_H,) and bt.pinball.shape == (E2E_H, 2)
        assert np.all(np.isfinite(bt.mae)) and np.all(bt.rmse >= bt.mae - 1e-12) and np.all((bt.coverage >= 0.0) & (bt.coverage <= 1.0))
        assert len(bt.pit) == E2E_H and len(bt.pit[0]) == N * (T - 4) and len(bt.pit[-1]) == N * (T - 4 - (E2E_H - 1))
        assert np.array_equal(bt.mae, rolling.horizon_errors_from(f.median, f.x, 4)[0])
        everything = np.ones((N, T), dtype=bool)
        uncond = mt.marginal_conditionals(imp, everything, get_wmad=False, engine=eng).nll
        print(f"classes={classes}: MAE by horizon {np.round(bt.mae, 4).tolist()}  coverage of the 5 % .. 95 % band {np.round(bt.coverage, 3).tolist()}  "
              f"mean one-step nll {bt.nll[0]:.4f} beside the unconditional {np.nanmean(uncond):.4f}")
    # the arrays: origin t0 against mpst_marginal_conditionals on the suffix mask of t0, on the very states the call was given
    t0 = 10
    scaled = _scaled_instances(imp, np.arange(N), np.zeros((N, T), dtype=bool))[4]
    states = imp.encoder(scaled)
    lab = np.array([imp.class_map[c] for c in np.asarray(imp.y_test).tolist()], dtype=np.int32)
    xr = imp.x_guess_range
    nll, pit, med, err, mean, q, _ = eng.rolling_model(imp.mps, states, lab, E2E_H, scaled, xr.xvals, xr.xvals_enc, levels=LEVELS)
    mc = marginal_conditionals_model(eng, imp.mps, states, lab, suffix_mask(N, T, t0), scaled, xr.xvals, xr.xvals_enc, levels=LEVELS)
    ref = RR.rolling_forecasts_ref([np.asarray(t) for t in imp.mps], np.asarray(states), lab, scaled, np.asarray(xr.xvals), np.asarray(xr.xvals_enc),
                                   E2E_H, LEVELS, origins=[t0])
    for h in range(E2E_H):
        u, ok = t0 + h, ~ref.excused[:, t0, h]
        assert np.abs(nll[:, t0, h] - mc.nll[:, u]).max() <= NLL_TOL and np.abs(pit[:, t0, h] - mc.pit[:, u]).max() <= PIT_TOL
        assert np.abs(mean[:, t0, h] - mc.mean[:, u]).max() <= MEAN_TOL * np.abs(xr.xvals).max()
        assert np.array_equal(med[:, t0, h][ok], mc.median[:, u][ok]) and np.array_equal(q[:, t0, h][ok], mc.quantiles[:, u][ok])
