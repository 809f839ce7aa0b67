#!/usr/bin/env python3
"""One timing of mpst_marginal_conditionals, no threshold: N = 256 series, T = 100, chi = 32, d = 4, C = 2, fp64, a random
normalised MPS, Legendre states, ngrid = 2001, 30 % of the sites missing at random, the true value supplied at every missing site,
three levels and the WMAD.  Beside it, on the same inputs in the same process:
  * mpst_marginal_model - the same density recursion from both ends without rho_t, the grid or a kept walk (and with the vector
    shortcut): the floor of the walk;
  * mpst_impute_model_dist with the same levels - the sequential median imputer.  It computes a DIFFERENT quantity (each missing site
    conditioned on the medians written before it, the missing sites only) and is here for context, not as a comparison of like with like.
Median of 7 calls after 2 warm-ups on one GPU; `device` is the call's own `seconds` (events around its kernels), the split is
mpst_get_impute_phases: (walk, grid phase) for the new call.
usage: python profiles/marginal_conditionals_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402

N, T, CHI, D, NC, NGRID, REPS, WARM = 256, 100, 32, 4, 2, 2001, 7, 2
LEVELS = (0.05, 0.5, 0.95)


def timed(fn, phases):
    dev, ph = [], []
    for k in range(WARM + REPS):
        s = fn()
        if k >= WARM:
            dev.append(s)
            ph.append(phases())
    return statistics.median(dev), min(dev), max(dev), ph[dev.index(sorted(dev)[len(dev) // 2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(23)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=23)
    x = rng.uniform(-0.95, 0.95, (N, T))
    phi = mt.legendre_encode_no_norm(x, D)
    lab = (np.arange(N) % NC).astype(np.int32)
    miss = rng.uniform(size=(N, T)) < 0.3
    xs = np.linspace(-1.0, 1.0, NGRID)
    gphi = mt.legendre_encode_no_norm(xs, D)
    lines = [f"marginal site conditionals of N={N} series: T={T} chi={CHI} d={D} C={NC} fp64, ngrid={NGRID}, {miss.mean() * 100:.1f} % of the sites "
             f"missing (scattered), levels {LEVELS} and the WMAD; median of {REPS} after {WARM} warm-ups, one MI355X",
             f"{'call':<58}{'device ms (min .. max)':>34}{'split ms':>34}"]
    eng = mt.SweepEngine(0)
    try:
        dev, lo, hi, ph = timed(lambda: eng.marginal_conditionals(W, phi, lab, miss, x, xs, gphi, levels=LEVELS).seconds, eng.impute_phases)
        lines.append(f"{'mpst_marginal_conditionals (all N T sites)':<58}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}"
                     f"{f'walk {ph[0] * 1e3:.3f} + grid {ph[1] * 1e3:.3f}':>34}")
        dev, lo, hi, ph = timed(lambda: eng.marginal_model(W, phi, miss)[1], eng.impute_phases)
        lines.append(f"{'mpst_marginal_model (the recursion alone: the floor)':<58}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}"
                     f"{'one kernel':>34}")
        dev, lo, hi, ph = timed(lambda: eng.impute_model(W, phi, lab, miss.astype(np.uint8), xs, gphi, method=0, get_wmad=True, levels=LEVELS)[2],
                                eng.impute_phases)
        lines.append(f"{'mpst_impute_model_dist (sequential; another quantity)':<58}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}"
                     f"{f'environments {ph[0] * 1e3:.3f} + sweep {ph[1] * 1e3:.3f}':>34}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
