#!/usr/bin/env python3
"""One timing of mpst_site_conditionals beside the route that gives the same medians without it, no threshold:
N = 256 complete series, T = 100, chi = 32, d = 4, C = 2, fp64, a random normalised MPS, Legendre states, a 2001-point grid, no
levels, WMAD on.  The other route is mpst_impute_model_dist over the N T = 25 600 replicas with one missing site each.  Median of 7
calls after 2 warm-ups, all in one process on one GPU; `device` is the call's own `seconds` (events around its kernels), the split
is mpst_get_impute_phases: (walk, grid phase) for the new call, (environment pass, sweep) for the replicas.
usage: python profiles/site_conditionals_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402

N, T, CHI, D, NC, NGRID, REPS, WARM = 256, 100, 32, 4, 2, 2001, 7, 2


def timed(fn, eng):
    dev, ph = [], []
    for k in range(WARM + REPS):
        s = fn()
        if k >= WARM:
            dev.append(s)
            ph.append(eng.impute_phases())
    med = statistics.median(dev)
    return med, min(dev), max(dev), ph[dev.index(sorted(dev)[len(dev) // 2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(19)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=19)
    x = rng.uniform(-0.95, 0.95, (N, T))
    phi = mt.legendre_encode_no_norm(x, D)
    lab = (np.arange(N) % NC).astype(np.int32)
    xs = np.linspace(-1.0, 1.0, NGRID)
    gphi = mt.legendre_encode_no_norm(xs, D)
    lines = [f"leave-one-out conditionals of N={N} series: T={T} chi={CHI} d={D} C={NC} fp64, ngrid={NGRID}, no levels, WMAD on; median of {REPS} "
             f"after {WARM} warm-ups, one MI355X",
             f"{'route':<58}{'device ms (min .. max)':>32}{'split ms':>24}"]
    eng = mt.SweepEngine(0)
    try:
        out = {}

        def new():
            *out["new"], s = eng.site_conditionals(W, phi, lab, x, xs, gphi)
            return s
        dev, lo, hi, ph = timed(new, eng)
        lines.append(f"{'mpst_site_conditionals':<58}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>32}"
                     f"{f'walk {ph[0] * 1e3:.3f} + grid {ph[1] * 1e3:.3f}':>24}")
        mask = np.tile(np.eye(T, dtype=np.uint8), (N, 1))
        phir, labr = np.repeat(phi, T, axis=0), np.repeat(lab, T)

        def old():
            out["x"], out["e"], s = eng.impute_model(W, phir, labr, mask, xs, gphi, method=0, get_wmad=True)[:3]
            return s
        dev2, lo, hi, ph = timed(old, eng)
        info = eng.impute_info()
        lines.append(f"{'mpst_impute_model_run, ' + str(N * T) + ' one-missing-site replicas':<58}{f'{dev2 * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>32}"
                     f"{f'env {ph[0] * 1e3:.3f} + sweep {ph[1] * 1e3:.3f}':>24}")
        sel = mask.astype(bool)
        lines.append(f"the replicas took the {'closed-form' if info['closed_form_densities'] else 'table'} densities, "
                     f"{'sixteen chains' if info['batched_sweep'] else 'one chain'} per workgroup; medians equal: "
                     f"{bool(np.array_equal(out['x'][sel].reshape(N, T), out['new'][2]))}, largest |WMAD difference| "
                     f"{np.abs(out['e'][sel].reshape(N, T) - out['new'][3]).max():.1e} (the grid values are not exact doubles); "
                     f"ratio of the device times {dev2 / dev:.2f}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
