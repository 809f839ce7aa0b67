"""mpst_impute_dist / mpst_impute_model_dist on the device: more levels and the conditional cdf next to the median (get_cdfs,
src/Imputation/imputation.jl:581-622).  The yardsticks: the plain median call (bits), MPST_IMPUTE_QUANTILE with a constant uniform
number (bits, first site), the NumPy restatement tests/impute_dist_ref.py (the bars of test_batched_sweep_against_the_oracle), and
the outputs against each other (the level is the argmin of the returned cdf; stride 7 is a subset of stride 1)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import impute_numpy as I
from oracle import ref_numpy as R
from tests import impute_dist_ref as D
from tests.test_gpu_impute_model import _complex_mps, _problem

pytestmark = pytest.mark.gpu

LEVELS = (0.05, 0.5, 0.95)
CASES = [(True, 8, 20), (False, 4, 33)]
IDS = ["fourier_d8", "legendre_d4_chi33"]


def _oracle_problem(cx, d, chi):
    N, T, Cn = 21, 10, 3
    return _problem(N, T, d, chi, Cn, seed=4000 + d + chi, ngrid=2001, cx=cx)


def _against_restatement(W, xs, grid_phi, phi, y, m, x, q, cdf, order, f64, levels=LEVELS, max_cut=None):
    """Check 4 of the issue: on the prefix of sites (in imputation order) whose median equals the restatement's within 1e-12, every
    level within 1.0000001 (f64) / 4.0000001 (f32) grid steps and the cdf within 1e-9 / 5e-4; instances cut short: at most 3 of 21 /
    N // 2.  Prints the worst figures before asserting."""
    classes = I.expand_label_index(W)
    dx = xs[1] - xs[0]
    N = len(y)
    cut = 0
    worst_q = worst_c = 0.0
    fails = []
    for i in range(N):
        sites = np.flatnonzero(m[i])
        if len(sites) == 0:
            continue
        med, wm, cdfs, lidx, _ = D.impute_med_and_cdfs(classes[y[i]], phi[i], sites, xs, grid_phi, order, levels)
        ranks = list(range(len(sites))) if order == "forwards" else list(range(len(sites) - 1, -1, -1))
        npre = 0
        for r in ranks:
            if abs(x[i, sites[r]] - med[r]) > 1e-12:
                break
            npre += 1
        if npre < len(sites):
            cut += 1
            first = ranks[npre]
            if abs(x[i, sites[first]] - med[first]) > (1.0000001 if f64 else 4.0000001) * dx:
                fails.append(("median", i, first))
        for r in ranks[:npre]:
            dq = np.abs(q[i, sites[r]] - xs[lidx[r]]).max() / dx
            worst_q = max(worst_q, dq)
            if dq > (1.0000001 if f64 else 4.0000001):
                fails.append(("level", i, r, dq))
            if cdf is not None:
                dc = np.abs(cdf[i, r] - cdfs[r]).max()
                worst_c = max(worst_c, dc)
                if dc >= (1e-9 if f64 else 5e-4):
                    fails.append(("cdf", i, r, dc))
    print(f"[dist vs restatement] order={order} f64={f64}: worst level {worst_q:.3f} grid steps, worst |cdf diff| {worst_c:.3e}, "
          f"instances cut short {cut}/{N}")
    assert not fails, fails[:5]
    assert cut <= ((3 if f64 else N // 2) if max_cut is None else max_cut), cut


def _self_consistent(xs, m, x, q, cdf, levels=LEVELS):
    """Checks 2 and 5: level 0.5 is the median, levels ordered and on the grid, cdf 0 .. 1 non-decreasing, the level is the argmin of the
    returned cdf, zero rows beyond the missing count."""
    mask = m.astype(bool)
    order = np.argsort(levels)
    assert np.array_equal(q[..., list(levels).index(0.5)][mask], x[mask])
    assert np.all(q[~mask] == 0.0)
    qs = q[..., order][mask]
    assert np.all(np.diff(qs, axis=1) >= 0.0)
    assert qs.min() >= xs[0] and qs.max() <= xs[-1]
    assert np.all(np.isin(qs, xs))
    if cdf is None:
        return
    for i in range(m.shape[0]):
        nm = int(mask[i].sum())
        assert np.all(cdf[i, nm:] == 0.0)
        sites = np.flatnonzero(mask[i])
        for r in range(nm):
            c = cdf[i, r]
            assert c[0] == 0.0 and c[-1] == 1.0
            assert np.all(np.diff(c) >= 0.0), (i, r, np.diff(c).min())
            for l, lv in enumerate(levels):
                assert xs[int(np.argmin(np.abs(c - lv)))] == q[i, sites[r], l], (i, r, lv)


@pytest.mark.parametrize("order", [0, 1], ids=["forwards", "backwards"])
@pytest.mark.parametrize("compute", ["f64", "f32"])
@pytest.mark.parametrize("cx,d,chi", CASES, ids=IDS)
def test_no_outputs_is_the_plain_median_call(engine_cls, monkeypatch, cx, d, chi, compute, order):
    """Check 1: nq = 0 and cdf_stride = 0 through the new entry points equal the old ones bit for bit, batched route and MPST_IMP_NO_BATCH."""
    W, xs, enc, gphi, X, y, phi, m, rng = _oracle_problem(cx, d, chi)
    eng = engine_cls(0)
    try:
        for nb in (False, True):
            if nb:
                monkeypatch.setenv("MPST_IMP_NO_BATCH", "1")
            x0, e0, _ = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute)
            b0 = eng.impute_info()["batched_sweep"]
            model_args = (W, phi, y, m, xs, gphi, 0, True)
            # (the Python wrapper takes the old path without the arguments: call the entry point itself with nq = 0, stride 0)
            x1, e1 = _raw_model_dist(eng, *model_args, order=order, compute=compute, levels=None, cdf_stride=0)[:2]
            assert eng.impute_info()["batched_sweep"] == b0 == (not nb)
            assert np.array_equal(x0, x1) and np.array_equal(e0, e1)
            # and with levels: the median itself does not move
            x2, e2, _, q2, _ = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, levels=LEVELS)
            assert eng.impute_info()["batched_sweep"] == b0
            assert np.array_equal(x0, x2) and np.array_equal(e0, e2)
        if not cx and compute == "f64":
            srt = np.argsort(y, kind="stable")
            eng.set_options(chi_max=chi)
            eng.set_dataset(1, phi[srt], y[srt], 3)
            eng.set_mps(W)
            xa, ea, _ = eng.impute(1, m[srt], xs, gphi, 0, True, order=order)
            xb, eb = _raw_ctx_dist(eng, 1, m[srt], xs, gphi, order=order)[:2]
            assert np.array_equal(xa, xb) and np.array_equal(ea, eb)
    finally:
        eng.close()


def _raw_model_dist(eng, W, phi, y, m, xs, gphi, method, get_wmad, order=0, compute="f64", levels=None, cdf_stride=0, cdf_rows=None,
                    expect=None):
    """mpst_impute_model_dist itself, with whatever arguments (the wrapper refuses the bad ones on the host).  Returns (x, err, q, cdf),
    or the status code when `expect` is given."""
    from mpstime_jl_amd import _lib as L
    from mpstime_jl_amd.engine import _site_to_abi, cdf_points
    cx = any(np.iscomplexobj(t) for t in W)
    dt = np.complex128 if cx else np.float64
    T = len(W)
    ls = [j for j, t in enumerate(W) if np.ndim(t) == 4][0]
    chi = np.array([W[0].shape[0]] + [t.shape[2] for t in W], dtype=np.int32)
    bufs = [_site_to_abi(t, dt) for t in W]
    ptrs = (C.c_void_p * T)(*[b.ctypes.data for b in bufs])
    ph = np.ascontiguousarray(phi, dtype=dt)
    lab = np.ascontiguousarray(y, dtype=np.int32)
    mm = np.ascontiguousarray(m, dtype=np.uint8)
    N, d = ph.shape[0], ph.shape[2]
    gx = np.ascontiguousarray(xs, dtype=np.float64)
    gp = np.ascontiguousarray(gphi, dtype=dt)
    model = L.ImputeModel(N, T, d, int(W[ls].shape[3]), ls, 1 if cx else 0, {"f64": 0, "f32": 1}[compute], C.cast(ptrs, C.POINTER(C.c_void_p)),
                          chi.ctypes.data_as(C.POINTER(C.c_int32)), ph.ctypes.data_as(C.c_void_p), lab.ctypes.data_as(C.POINTER(C.c_int32)))
    o = L.ImputeOpts(int(method), int(order), int(get_wmad), 1, 2 if cx else 1, 0, 0.0)
    dp = C.POINTER(C.c_double)
    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.float64)
    nq = 0 if lv is None else len(lv)
    rows = int(mm.sum(axis=1).max()) if cdf_rows is None else cdf_rows
    x, err = np.zeros((N, T)), np.zeros((N, T))
    q = np.zeros((N, T, max(nq, 1)))
    cdf = np.zeros((N, max(rows, 1), cdf_points(len(gx), cdf_stride))) if cdf_stride else None
    sec = C.c_double()
    rc = eng.lib.mpst_impute_model_dist(eng.ctx, C.byref(model), mm.ctypes.data_as(C.POINTER(C.c_uint8)), gx.ctypes.data_as(dp),
                                        gp.ctypes.data_as(C.c_void_p), len(gx), C.byref(o), x.ctypes.data_as(dp), err.ctypes.data_as(dp),
                                        C.byref(sec), nq, lv.ctypes.data_as(dp) if nq else None, q.ctypes.data_as(dp) if nq else None,
                                        cdf_stride, rows if cdf_stride else 0, cdf.ctypes.data_as(dp) if cdf is not None else None)
    if expect is not None:
        return rc, (eng.lib.mpst_last_error(eng.ctx) or b"").decode()
    assert rc == 0, eng.lib.mpst_last_error(eng.ctx)
    return x, err, q if nq else None, cdf


def _raw_ctx_dist(eng, which, m, xs, gphi, order=0):
    from mpstime_jl_amd import _lib as L
    mm = np.ascontiguousarray(m, dtype=np.uint8)
    N, T = mm.shape
    gx = np.ascontiguousarray(xs, dtype=np.float64)
    gp = np.ascontiguousarray(gphi, dtype=np.float64)
    o = L.ImputeOpts(0, int(order), 1, 1, 1, 0, 0.0)
    dp = C.POINTER(C.c_double)
    x, err = np.zeros((N, T)), np.zeros((N, T))
    sec = C.c_double()
    rc = eng.lib.mpst_impute_dist(eng.ctx, which, mm.ctypes.data_as(C.POINTER(C.c_uint8)), gx.ctypes.data_as(dp), gp.ctypes.data_as(dp), len(gx),
                                  C.byref(o), x.ctypes.data_as(dp), err.ctypes.data_as(dp), C.byref(sec), 0, None, None, 0, 0, None)
    assert rc == 0, eng.lib.mpst_last_error(eng.ctx)
    return x, err


@pytest.mark.parametrize("order", [0, 1], ids=["forwards", "backwards"])
@pytest.mark.parametrize("compute", ["f64", "f32"])
@pytest.mark.parametrize("cx,d,chi", CASES, ids=IDS)
def test_levels_and_cdf_against_the_restatement(engine_cls, monkeypatch, cx, d, chi, compute, order):
    """Checks 2, 3, 4, 5 on the inputs of test_batched_sweep_against_the_oracle (ragged masks, an instance with nothing missing)."""
    W, xs, enc, gphi, X, y, phi, m, rng = _oracle_problem(cx, d, chi)
    N, T = m.shape
    eng = engine_cls(0)
    try:
        x0, e0, _ = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute)
        plain = eng.impute_info()
        xl, el, _, ql, none = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, levels=LEVELS)
        assert none is None and eng.impute_info()["batched_sweep"] == plain["batched_sweep"] == True      # levels stay on the batched sweep
        x, e, _, q, cdf = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, levels=LEVELS, cdf_stride=1)
        x7, _, _, q7, cdf7 = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, levels=LEVELS, cdf_stride=7)
        # check 3: the first site imputed against the existing sampler with u == level
        qs = [eng.impute_model(W, phi, y, m, xs, gphi, 2, False, np.full((N, T, 1), lv), order=order, compute=compute)[0] for lv in LEVELS]
        # a call with a cdf runs on the one-instance kernel: its median is that kernel's plain median (MPST_IMP_NO_BATCH), bit for bit
        monkeypatch.setenv("MPST_IMP_NO_BATCH", "1")
        x1, e1, _ = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute)
    finally:
        eng.close()
    assert np.array_equal(x0, xl) and np.array_equal(e0, el)
    assert np.array_equal(x1, x) and np.array_equal(e1, e) and np.array_equal(x1, x7)
    assert cdf.shape == (N, int(m.sum(axis=1).max()), len(xs))
    for i in range(N):
        sites = np.flatnonzero(m[i])
        if len(sites):
            j = sites[0] if order == 0 else sites[-1]
            for l in range(len(LEVELS)):
                assert ql[i, j, l] == qs[l][i, j], (i, j, l)
    _self_consistent(xs, m, xl, ql, None)
    _self_consistent(xs, m, x, q, cdf)
    # stride 7: the stride-1 output at 0, 7, ..., and the last index
    from mpstime_jl_amd.engine import cdf_indices
    assert np.array_equal(cdf7, cdf[:, :, cdf_indices(len(xs), 7)]) and np.array_equal(q7, q)
    # the two routes of the levels (batched sweep / one-instance kernel of the cdf call) against the restatement
    od = "forwards" if order == 0 else "backwards"
    _against_restatement(W, xs, gphi, phi, y, m, xl, ql, None, od, compute == "f64")
    _against_restatement(W, xs, gphi, phi, y, m, x, q, cdf, od, compute == "f64")


@pytest.mark.parametrize("route", ["MPST_IMP_NO_TRIG", "MPST_IMP_NO_BATCH"])
@pytest.mark.parametrize("compute", ["f64", "f32"])
@pytest.mark.parametrize("cx,d,chi", CASES, ids=IDS)
def test_routes(engine_cls, monkeypatch, cx, d, chi, compute, route):
    """Check 6: the table path and the one-instance closed-form kernel serve the same outputs within the same bars."""
    W, xs, enc, gphi, X, y, phi, m, rng = _oracle_problem(cx, d, chi)
    eng = engine_cls(0)
    try:
        xa, _, _, qa, ca = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, compute=compute, levels=LEVELS, cdf_stride=1)
        monkeypatch.setenv(route, "1")
        x, e, _, q, cdf = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=1, compute=compute, levels=LEVELS, cdf_stride=1)
        info = eng.impute_info()
        xf, _, _, qf, cf = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, compute=compute, levels=LEVELS, cdf_stride=1)
    finally:
        eng.close()
    assert not info["batched_sweep"] and info["closed_form_densities"] == (route != "MPST_IMP_NO_TRIG")
    _self_consistent(xs, m, x, q, cdf)
    _self_consistent(xs, m, xf, qf, cf)
    f64 = compute == "f64"
    _against_restatement(W, xs, gphi, phi, y, m, x, q, cdf, "backwards", f64)
    _against_restatement(W, xs, gphi, phi, y, m, xf, qf, cf, "forwards", f64)
    if route == "MPST_IMP_NO_TRIG":
        # closed form against the table path directly, where both conditioned on the same medians
        dx = xs[1] - xs[0]
        mask = m.astype(bool)
        for i in range(m.shape[0]):
            sites = np.flatnonzero(mask[i])
            for r, j in enumerate(sites):
                if xa[i, j] != xf[i, j]:
                    break
                assert np.abs(qa[i, j] - qf[i, j]).max() <= (1.0000001 if f64 else 4.0000001) * dx
                assert np.abs(ca[i, r] - cf[i, r]).max() < (1e-9 if f64 else 5e-4)


@pytest.mark.parametrize("order", [0, 1], ids=["forwards", "backwards"])
@pytest.mark.parametrize("compute", ["f64", "f32"])
@pytest.mark.parametrize("cx,d,chi", CASES, ids=IDS)
def test_cdf_from_the_batched_sweep(engine_cls, monkeypatch, cx, d, chi, compute, order):
    """MPST_IMP_DIST_CDF_BATCH=1 (the other arm of the route A/B): the cdf written by k_imp_leftb, a wave per chain.  Same
    checks as the default route: the level is the argmin of the returned cdf, the median is the batched sweep's, and both meet the
    restatement's bars.  The variable is read on every call."""
    W, xs, enc, gphi, X, y, phi, m, rng = _oracle_problem(cx, d, chi)
    eng = engine_cls(0)
    try:
        x0, e0, _ = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute)
        eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, cdf_stride=5)
        assert not eng.impute_info()["batched_sweep"]
        monkeypatch.setenv("MPST_IMP_DIST_CDF_BATCH", "1")
        x, e, _, q, cdf = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, levels=LEVELS, cdf_stride=1)
        assert eng.impute_info()["batched_sweep"]
        x5, _, _, _, cdf5 = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=order, compute=compute, cdf_stride=5)
    finally:
        eng.close()
    from mpstime_jl_amd.engine import cdf_indices
    assert np.array_equal(x0, x) and np.array_equal(e0, e) and np.array_equal(x0, x5)
    assert np.array_equal(cdf5, cdf[:, :, cdf_indices(len(xs), 5)])
    _self_consistent(xs, m, x, q, cdf)
    _against_restatement(W, xs, gphi, phi, y, m, x, q, cdf, "forwards" if order == 0 else "backwards", compute == "f64")


@pytest.mark.parametrize("cx,compute,chi,d", [(False, "f64", 72, 3), (True, "f32", 72, 3)], ids=["real_f64_chi72", "complex_f32_chi72"])
def test_large_bond_route(engine_cls, monkeypatch, cx, compute, chi, d):
    """Check 6, chi = 72: the environments come from k_imp_right_big (built as test_bond_dimensions_beyond_the_lds_kernel builds it)."""
    N, Cn, T = 6, 1, 12
    rng = np.random.default_rng(chi)
    W = _complex_mps(T, d, chi, Cn, rng) if cx else R.random_mps(T, d, chi, Cn, rng)
    xs = -1.0 + (2.0 / 800) * np.arange(801)
    enc = (lambda x: R.fourier_encode(x, d)) if cx else (lambda x: R.legendre_encode(x, d))
    X = rng.uniform(-0.9, 0.9, (N, T))
    y = np.zeros(N, dtype=np.int32)
    m = (rng.uniform(size=(N, T)) < 0.5).astype(np.uint8)
    m[0] = 1
    eng = engine_cls(0)
    try:
        x0, e0, _ = eng.impute_model(W, enc(X), y, m, xs, enc(xs), 0, True, compute=compute)
        b0 = eng.impute_info()["batched_sweep"]
        xl, el, _, ql, _ = eng.impute_model(W, enc(X), y, m, xs, enc(xs), 0, True, compute=compute, levels=LEVELS)
        assert eng.impute_info()["batched_sweep"] == b0
        x, e, _, q, cdf = eng.impute_model(W, enc(X), y, m, xs, enc(xs), 0, True, compute=compute, levels=LEVELS, cdf_stride=1)
        monkeypatch.setenv("MPST_IMP_NO_BATCH", "1")
        x1, e1, _ = eng.impute_model(W, enc(X), y, m, xs, enc(xs), 0, True, compute=compute)
    finally:
        eng.close()
    assert np.array_equal(x0, xl) and np.array_equal(e0, el)
    assert np.array_equal(x1, x) and np.array_equal(e1, e)
    _self_consistent(xs, m, xl, ql, None)
    _against_restatement(W, xs, enc(xs), enc(X), y, m, xl, ql, None, "forwards", compute == "f64")
    _self_consistent(xs, m, x, q, cdf)
    _against_restatement(W, xs, enc(xs), enc(X), y, m, x, q, cdf, "forwards", compute == "f64")


@pytest.mark.parametrize("cx,d,chi", CASES, ids=IDS)
def test_blocks(engine_cls, monkeypatch, cx, d, chi):
    """Check 7: several blocks (MPST_IMPUTE_CHUNK_GB) give the bits of one block."""
    W, xs, enc, gphi, X, y, phi, m, rng = _oracle_problem(cx, d, chi)
    eng = engine_cls(0)
    try:
        monkeypatch.delenv("MPST_IMPUTE_CHUNK_GB", raising=False)
        a = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, levels=LEVELS, cdf_stride=3)
        al = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=1, levels=LEVELS)
        monkeypatch.setenv("MPST_IMPUTE_CHUNK_GB", "0.001")
        b = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, levels=LEVELS, cdf_stride=3)
        bl = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, order=1, levels=LEVELS)
    finally:
        eng.close()
    for k in (0, 1, 3, 4):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(al[0], bl[0]) and np.array_equal(al[3], bl[3])


def test_errors(engine_cls):
    """Check 8: the stated codes, each with a message; nothing traps."""
    from mpstime_jl_amd import _lib as L
    W, xs, enc, gphi, X, y, phi, m, rng = _problem(5, 6, 3, 4, 2, seed=1, ngrid=101, cx=False)
    eng = engine_cls(0)
    try:
        args = (eng, W, phi, y, m, xs, gphi)
        for method in (1, 2, 3, 4):
            rc, msg = _raw_model_dist(*args, method, True, levels=[0.5], expect=True)
            assert rc == L.MPST_ERR_UNSUPPORTED and "MEDIAN" in msg, (method, rc, msg)
        for lv in ([0.0], [1.0], [0.5, -0.2], list(np.linspace(0.05, 0.95, 17))):
            rc, msg = _raw_model_dist(*args, 0, True, levels=lv, expect=True)
            assert rc == L.MPST_ERR_INVALID and msg, (lv, rc, msg)
        rc, msg = _raw_model_dist(*args, 0, True, cdf_stride=1, cdf_rows=int(m.sum(axis=1).max()) - 1, expect=True)
        assert rc == L.MPST_ERR_INVALID and "cdf_rows" in msg, (rc, msg)
        # and the engine still works
        x, e, _, q, cdf = eng.impute_model(W, phi, y, m, xs, gphi, 0, True, levels=[0.25, 0.75], cdf_stride=2)
        assert np.all(q[..., 0] <= q[..., 1]) and cdf.shape[2] == (101 - 2) // 2 + 2
        with pytest.raises(ValueError):
            eng.impute_model(W, phi, y, m, xs, gphi, 1, True, levels=[0.5])
    finally:
        eng.close()


def test_host_api(engine_cls):
    """Check 9: impute_dataset(quantiles=) and get_cdfs on a fitted Legendre model and on a Fourier model."""
    import mpstime_jl_amd as mt
    rng = np.random.default_rng(5)
    X1, _ = mt.trendy_sine(24, 30, period=(12.0, 15.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
    X2, _ = mt.trendy_sine(24, 30, period=(16.0, 19.0), slope=[-3.0, 0.0, 3.0], sigma=0.1, rng=rng)
    Xtr, ytr = np.concatenate([X1[:20], X2[:20]]), np.repeat([0, 1], 20)
    Xte, yte = np.concatenate([X1[20:], X2[20:]]), np.repeat([0, 1], 10)
    opts = mt.MPSOptions(d=4, chi_max=12, nsweeps=2, verbosity=-1, encoding="Legendre_No_Norm")
    trained = mt.fitMPS(Xtr, ytr, Xte, yte, opts)[0]
    imp = mt.init_imputation_problem(trained, Xte, yte, dx=1e-3, verbosity=0)
    _host_checks(mt, imp, rng)
    # a Fourier model (complex: through impute_model)
    T, d, chi, Cn = 16, 5, 8, 2
    W = _complex_mps(T, d, chi, Cn, rng)
    optf = mt.MPSOptions(encoding="Fourier", d=d, chi_max=chi, verbosity=-1)
    t = np.linspace(0, 1, T)
    ytr2 = np.sort(rng.integers(0, Cn, 30))
    Xtr2 = np.sin(2 * np.pi * (t[None, :] * (1 + ytr2[:, None]) + rng.uniform(size=(30, 1)))) + 0.1 * rng.normal(size=(30, T))
    yte2 = rng.integers(0, Cn, 10)
    Xte2 = np.sin(2 * np.pi * (t[None, :] * (1 + yte2[:, None]) + rng.uniform(size=(10, 1)))) + 0.1 * rng.normal(size=(10, T))
    td = mt.EncodedTimeSeriesSet(None, ytr2, ytr2.astype(np.int32), Xtr2, np.bincount(ytr2, minlength=Cn))
    impf = mt.init_imputation_problem(mt.TrainedMPS(W, optf, td), Xte2, yte2, dx=1e-3, verbosity=0)
    _host_checks(mt, impf, rng)


def _host_checks(mt, imp, rng):
    from mpstime_jl_amd.imputation import _scaled_instances
    Nte, T = imp.X_test.shape
    mask = rng.uniform(size=(Nte, T)) < 0.3
    mask[0] = False
    mask[0, 3:9] = True
    for inv in (True, False):
        for compute in ("f64", "f32"):
            ts, err, bands = mt.impute_dataset(imp, mask, "median", invert_transform=inv, quantiles=(0.05, 0.95), compute=compute)
            ts0, err0 = mt.impute_dataset(imp, mask, "median", invert_transform=inv, compute=compute)
            assert np.array_equal(ts, ts0) and np.array_equal(err, err0)
            assert bands.shape == (Nte, T, 2)
            assert np.all(bands[..., 0][mask] <= ts[mask]) and np.all(ts[mask] <= bands[..., 1][mask])
            assert np.array_equal(bands[..., 0][~mask], ts[~mask]) and np.array_equal(bands[..., 1][~mask], ts[~mask])
    # get_cdfs: a row on which both fill values (mean of the training / of the test set) leave the out-of-bounds rescale inactive
    y = np.asarray(imp.y_test)
    row = None
    for r in range(Nte):
        mk = np.zeros((1, T), dtype=bool)
        mk[0, 3:9] = True
        enc, norms, raw, full, scaled, oob = _scaled_instances(imp, [r], mk)
        raw2 = imp.X_test[[r]].copy()
        raw2[mk] = np.mean(imp.X_test)
        scaled2, oob2 = mt.transform_test_data(raw2, norms, imp.opts, enc.range)
        if len(oob) == 0 and len(oob2) == 0 and np.array_equal(scaled[~mk], scaled2[~mk]):
            row = r
            break
    assert row is not None, "no row with an inactive out-of-bounds rescale under both fill values: the precondition of the comparison"
    cls = y[row]
    inst = int(np.flatnonzero(np.flatnonzero(y == cls) == row)[0])
    sites = np.arange(3, 9)
    mk = np.zeros((Nte, T), dtype=bool)
    mk[row, sites] = True
    for od in ("forwards", "backwards"):
        cdfs, ts, perr, target = mt.get_cdfs(imp, cls, inst, sites, impute_order=od)
        assert len(cdfs) == len(sites) and all(len(c) == len(imp.x_guess_range.xvals) for c in cdfs)
        ref, referr = mt.impute_dataset(imp, mk[[row]], "median", rows=[row], invert_transform=False, impute_order=od)
        assert np.array_equal(ts[0], ref[0]) and np.array_equal(perr[0], referr[0])
        xs = imp.x_guess_range.xvals
        for r, j in enumerate(sites):       # ascending site order: row r's median is the imputed value of site sites[r]
            assert cdfs[r][0] == 0.0 and cdfs[r][-1] == 1.0
            assert xs[int(np.argmin(np.abs(cdfs[r] - 0.5)))] == ts[0][j]
        assert target.shape == (T,)
    c4 = mt.get_cdfs(imp, cls, inst, sites, stride=4)[0]
    assert len(c4[0]) == (len(xs) - 2) // 4 + 2
    with pytest.raises(ValueError, match="get_cdfs only supports method=:median"):
        mt.get_cdfs(imp, cls, inst, sites, method="mean")


def test_configs4_full_size_with_two_levels(engine_cls):
    """Check 10: BASELINE configs[4]'s imputation shape (built as test_configs4_full_size_pass builds it) with two levels: finite, ordered
    around the median on all instances, x bit-equal to the plain median call."""
    import bench
    import mpstime_jl_amd as mt
    N, T, d, chi = 8192, 200, 8, 64
    rng = np.random.default_rng(100)
    W = bench.random_chain(T, d, chi, np.random.default_rng(7))
    enc = mt.model_encoding("Fourier")
    xs = -1.0 + 1e-4 * np.arange(20001)
    gphi = np.ascontiguousarray(enc.encode(xs, d), dtype=np.complex128)
    X = rng.uniform(-0.95, 0.95, (N, T))
    phi = np.ascontiguousarray(enc.encode(X, d), dtype=np.complex128)
    m = np.zeros((N, T), dtype=np.uint8)
    for i in range(N):
        s0 = rng.integers(0, T - T // 2 + 1)
        m[i, s0:s0 + T // 2] = 1
    lab = np.zeros(N, dtype=np.int32)
    eng = engine_cls(0)
    try:
        x0, e0, _ = eng.impute_model(W, phi, lab, m, xs, gphi, 0, True, compute="f32")
        i0 = eng.impute_info()
        x, e, _, q, _ = eng.impute_model(W, phi, lab, m, xs, gphi, 0, True, compute="f32", levels=(0.05, 0.95))
        i1 = eng.impute_info()
    finally:
        eng.close()
    assert i0["batched_sweep"] and i1["batched_sweep"]
    mask = m.astype(bool)
    assert np.all(np.isfinite(q)) and np.all(q[~mask] == 0.0)
    assert np.array_equal(x, x0) and np.array_equal(e, e0)
    assert np.all(q[..., 0][mask] <= x[mask]) and np.all(x[mask] <= q[..., 1][mask])
    assert q[mask].min() >= xs[0] and q[mask].max() <= xs[-1]


SHARD_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MPST_ROOT"])
import numpy as np
import torch, torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
import mpstime_jl_amd as mt
from tests.test_gpu_impute_traj import _imp_problem, shard_mask
imp, X, y = _imp_problem()
sh = mt.Shard(rank, world, rccl=False)
dev = rank % max(torch.cuda.device_count(), 1)
ts, err, bands = mt.impute_dataset(imp, shard_mask(X), "median", shard=sh, device=dev, quantiles=(0.05, 0.5, 0.95))
np.savez(os.path.join(os.environ["MPST_OUT"], f"bands{rank}.npz"), ts=ts, err=err, bands=bands)
dist.barrier()
dist.destroy_process_group()
"""


def test_sharded_bands_equal_single_process(tmp_path):
    """impute_dataset(..., quantiles=, shard=): three ranks on disjoint row sets gather the single-process bands on every rank."""
    import mpstime_jl_amd as mt
    from tests.test_gpu_impute_traj import _imp_problem, shard_mask
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(SHARD_WORKER)
    env = dict(os.environ, MPST_ROOT=root, MPST_OUT=str(tmp_path))
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
                    "--master-port", str(port), str(script)], check=True, env=env, timeout=600)
    imp, X, y = _imp_problem()
    mask = shard_mask(X)
    ts, err, bands = mt.impute_dataset(imp, mask, "median", quantiles=(0.05, 0.5, 0.95))
    assert bands.shape == mask.shape + (3,)
    assert np.array_equal(bands[..., 1], ts)
    assert np.all(bands[..., 0] <= ts) and np.all(ts <= bands[..., 2])
    for r in range(3):
        o = np.load(tmp_path / f"bands{r}.npz")
        assert np.array_equal(o["ts"], ts) and np.array_equal(o["err"], err, equal_nan=True) and np.array_equal(o["bands"], bands)
