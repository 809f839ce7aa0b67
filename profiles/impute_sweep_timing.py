#!/usr/bin/env python3
"""Timing of the imputation sweep where bench.py has no shape: real models with Legendre states, d = 12 and d = 6 (the table kernels are
built for one workgroup per CU above d = 8 and for two up to it), and a complex one with Fourier states, d = 8; chi = 16, N = 1024,
T = 100, half of every instance missing in one block, the reference's 20 001-value grid; fp64 and fp32 chains; median + WMAD, mean + std and the distribution variant (median + WMAD with two levels and every 100th cdf value) on the
three routes of the sweep - batched closed form (default; a call with cdf rows leaves it), one-chain closed form (MPST_IMP_NO_BATCH),
one-chain table (MPST_IMP_NO_TRIG).  Median of 5 calls after 1 warm-up, all in one process on one GPU; `device` is the call's own
`seconds`, `sweep` the second of its two phases (mpst_get_impute_phases: environments, sweep).
usage: python profiles/impute_sweep_timing.py [--tree DIR] [--out FILE]     DIR: the checkout whose package and library to load"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, CHI, NGRID, REPS, WARM = 1024, 100, 16, 20001, 5, 1
ROUTES = {"batched closed form": None, "one-chain closed form": "MPST_IMP_NO_BATCH", "one-chain table": "MPST_IMP_NO_TRIG"}
METHODS = (("median+wmad", 0, {}), ("mean+std", 3, {}), ("median+levels", 0, dict(levels=(0.25, 0.75))),
           ("median+levels+cdf", 0, dict(levels=(0.25, 0.75), cdf_stride=100)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import mpstime_jl_amd as mt
    lines = [f"impute_model, chi={CHI} N={N} T={T} ngrid={NGRID}, median of {REPS} after {WARM} warm-up, one MI355X",
             f"{'model, route, method':<64}{'device ms (min .. max)':>34}{'sweep ms':>12}"]
    xs = -1.0 + 1e-4 * np.arange(NGRID)
    eng = mt.SweepEngine(0)
    try:
        for model, d, enc in (("legendre d=12", 12, mt.legendre_encode), ("legendre d=6", 6, mt.legendre_encode), ("fourier d=8", 8, mt.fourier_encode)):
            rng = np.random.default_rng(12)
            W = mt.generate_startingMPS(CHI, T, d, 1, init_rng=12, dtype=np.complex128 if model.startswith("fourier") else np.float64)
            gphi, phi = enc(xs, d), enc(rng.uniform(-0.95, 0.95, (N, T)), d)
            m = np.zeros((N, T), dtype=np.uint8)
            for i in range(N):
                s0 = rng.integers(0, T - T // 2 + 1)
                m[i, s0:s0 + T // 2] = 1
            lab = np.zeros(N, dtype=np.int32)
            for compute in ("f64", "f32"):
                for route, var in ROUTES.items():
                    for name, method, kw in METHODS:
                        if var:
                            os.environ[var] = "1"
                        try:
                            dev, swp = [], []
                            for k in range(WARM + REPS):
                                out = eng.impute_model(W, phi, lab, m, xs, gphi, method, True, compute=compute, **kw)
                                if k >= WARM:
                                    dev.append(out[2])
                                    swp.append(eng.impute_phases()[1])
                            info = eng.impute_info()
                        finally:
                            if var:
                                del os.environ[var]
                        assert np.all(np.isfinite(out[0])) and info["closed_form_densities"] == (var != "MPST_IMP_NO_TRIG"), info
                        lines.append(f"{f'{model} {compute}, {route}, {name}':<64}"
                                     f"{f'{statistics.median(dev) * 1e3:.3f} ({min(dev) * 1e3:.3f} .. {max(dev) * 1e3:.3f})':>34}"
                                     f"{statistics.median(swp) * 1e3:>12.3f}   batched={int(info['batched_sweep'])}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
