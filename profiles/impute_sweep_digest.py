#!/usr/bin/env python3
"""One SHA-256 per imputation call over the arrays it returns (x, err and, for the distribution variant, levels and cdf rows), on seeded
small problems through SweepEngine.impute_model, with impute_info() next to it so the route that ran is visible.  Two builds of the
library that compute the same bits print the same text: run it once per build, each in a process of its own, and compare the outputs.
The shapes are those of tests/test_gpu_impute_model.py (the batched-against-one-chain shapes with 20 001 grid values, the launches
above 64 KB of LDS with levels and cdf rows, the three other closed-form bases of the mean), one ITS call with three trajectories
and one table per site; each on the default route and under MPST_IMP_NO_BATCH / MPST_IMP_NO_TRIG / MPST_IMP_DIST_CDF_BATCH.
usage: python profiles/impute_sweep_digest.py [--tree DIR] [--out FILE]     DIR: the checkout whose package and library to load"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {"default": None, "no_batch": "MPST_IMP_NO_BATCH", "no_trig": "MPST_IMP_NO_TRIG", "cdf_batch": "MPST_IMP_DIST_CDF_BATCH"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(a.tree))
    import mpstime_jl_amd as mt
    from oracle import ref_numpy as R
    lines = []
    eng = mt.SweepEngine(0)

    def run(tag, routes, *args, **kw):
        for route in routes:
            if ROUTES[route]:
                os.environ[ROUTES[route]] = "1"
            try:
                out = eng.impute_model(*args, **kw)
            finally:
                if ROUTES[route]:
                    del os.environ[ROUTES[route]]
            h = hashlib.sha256()
            for arr in out[:2] + out[3:]:
                if arr is not None:
                    h.update(np.ascontiguousarray(arr).tobytes())
            info = eng.impute_info()
            lines.append(f"{tag:<66}{route:<10}{h.hexdigest()}  closed_form={int(info['closed_form_densities'])} "
                         f"batched={int(info['batched_sweep'])} chains={info['chains']}")

    def complex_mps(T, d, chi, C, rng):
        return [x + 1j * y for x, y in zip(R.random_mps(T, d, chi, C, rng), R.random_mps(T, d, chi, C, rng))]

    def problem(N, T, d, chi, C, seed, ngrid, cx):
        rng = np.random.default_rng(seed)
        W = complex_mps(T, d, chi, C, rng) if cx else R.random_mps(T, d, chi, C, rng)
        xs = -1.0 + (2.0 / (ngrid - 1)) * np.arange(ngrid)
        enc = (lambda x: R.fourier_encode(x, d)) if cx else (lambda x: R.legendre_encode(x, d))
        y = rng.integers(0, C, N).astype(np.int32)
        X = rng.uniform(-0.95, 0.95, (N, T))
        m = (rng.uniform(size=(N, T)) < 0.4).astype(np.uint8)
        m[0], m[1] = 1, 0
        return W, xs, enc, enc(xs), y, enc(X), m, rng

    try:
        three = ("default", "no_batch", "no_trig")
        # every method, both orders, fp64 and fp32 chains: N = 37, T = 14, C = 3, 20 001 grid values
        for cx, d, chi in [(True, 8, 20), (True, 12, 9), (False, 12, 16), (False, 4, 33)]:
            W, xs, enc, gphi, y, phi, m, rng = problem(37, 14, d, chi, 3, 1000 + d + chi, 20001, cx)
            u = rng.uniform(0.02, 0.98, (37, 14, 3))
            for compute in ("f64", "f32"):
                for order in (0, 1):
                    tag = f"{'fourier' if cx else 'legendre'}_d{d}_chi{chi} {compute} order{order} "
                    kw = dict(order=order, compute=compute)
                    run(tag + "median+wmad", three, W, phi, y, m, xs, gphi, 0, True, **kw)
                    run(tag + "mode", three, W, phi, y, m, xs, gphi, 1, False, **kw)
                    run(tag + "quantile", three, W, phi, y, m, xs, gphi, 2, False, u[:, :, :1], **kw)
                    run(tag + "mean+std", three, W, phi, y, m, xs, gphi, 3, True, **kw)
                    run(tag + "its_reject", three, W, phi, y, m, xs, gphi, 4, True, u, max_trials=3, rejection_threshold=1.0, **kw)
            if (cx, d) == (True, 8):
                run("fourier_d8_chi20 f64 its_reject 3 trajectories seed 12345", three, W, phi, y, m, xs, gphi, 4, True, None, max_trials=3,
                    rejection_threshold=1.0, num_trajectories=3, seed=12345, row_id=np.arange(37)[::-1].copy())
            if (cx, d) == (False, 4):
                # one table per site: site t's grid states are the encoding of xs (1 - 0.02 t)
                per_site = np.ascontiguousarray(np.stack([enc(xs[::10] * (1.0 - 0.02 * t)) for t in range(14)]))
                run("legendre_d4_chi33 f64 table per site, median+wmad", ("default",), W, phi, y, m, np.ascontiguousarray(xs[::10]), per_site, 0, True)
                run("legendre_d4_chi33 f64 table per site, mode", ("default",), W, phi, y, m, np.ascontiguousarray(xs[::10]), per_site, 1, False)
        # the launches above 64 KB of LDS: N = 17, T = 4, 33 grid values, levels and cdf rows
        for name, (cx, d, chi, x0, h) in {"legendre_d16_chi8": (False, 16, 8, -0.0016, 1e-4), "fourier_d2_chi128": (True, 2, 128, -1.0, 2.0 / 32),
                                          "fourier_d2_chi32": (True, 2, 32, -1.0, 2.0 / 32)}.items():
            N, T, C = 17, 4, 2
            rng = np.random.default_rng(64 * 1024 + chi)
            dims = [1] + [chi] * (T - 1) + [1]
            W = []
            for j in range(T):
                shape = (dims[j], d, dims[j + 1]) + ((C,) if j == T - 1 else ())
                t = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cx else 0.0)
                W.append(t / np.linalg.norm(t))
            enc = (lambda x: R.fourier_encode(x, d)) if cx else (lambda x: R.legendre_encode(x, d))
            xs = x0 + h * np.arange(33)
            gphi, phi = enc(xs), enc(rng.uniform(-0.95, 0.95, (N, T)))
            y = rng.integers(0, C, N).astype(np.int32)
            pairs = [(p, q) for p in range(T) for q in range(p + 1, T)]
            m = np.zeros((N, T), dtype=np.uint8)
            for i in range(N):
                m[i, list(pairs[i % len(pairs)])] = 1
            for order in (0, 1):
                tag = f"{name} f64 order{order} median+wmad"
                run(tag, tuple(ROUTES), W, phi, y, m, xs, gphi, 0, True, order=order)
                run(tag + " levels", tuple(ROUTES), W, phi, y, m, xs, gphi, 0, True, order=order, levels=(0.25, 0.75))
                run(tag + " levels cdf_stride 4", tuple(ROUTES), W, phi, y, m, xs, gphi, 0, True, order=order, levels=(0.25, 0.75), cdf_stride=4)
        # the mean with the other closed-form bases: N = 9, T = 8, chi = 5, 1 001 grid values on [0, 1]
        for basis, d, code, fn in (("Stoudenmire", 2, 3, mt.angle_encode), ("Sahand", 4, 4, mt.sahand_encode), ("Uniform", 3, 5, mt.uniform_encode)):
            rng = np.random.default_rng(17)
            W = complex_mps(8, d, 5, 2, rng) if basis != "Uniform" else R.random_mps(8, d, 5, 2, rng)
            xs = np.arange(1001) / 1000.0
            X = rng.uniform(0.03, 0.97, (9, 8))
            y = rng.integers(0, 2, 9).astype(np.int32)
            m = (rng.uniform(size=(9, 8)) < 0.4).astype(np.uint8)
            m[0], m[1] = 1, 0
            for compute in ("f64", "f32"):
                run(f"mean+std, {basis} d{d} {compute}", ("default",), W, fn(X, d), y, m, xs, fn(xs, d), 3, True, mean_basis=code, compute=compute)
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
