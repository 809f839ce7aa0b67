#!/usr/bin/env python3
"""One timing of mpst_observed_conditionals, no threshold: N = 256 series, T = 100, chi = 32, d = 4, C = 2, fp64, a random
normalised MPS, Legendre states, ngrid = 2001, three levels and the WMAD, both groups and the scores.  Three calls on the same series in
the same process:
  * every site GAUSS (sd 10 grid spacings): new ground, no bound.  Matrix products per series: the right walk 2 d (T - 1), the left
    walk's rho_t 2 d T and its step 2 d (T - 1) - what an all-MISSING series costs;
  * 30 % of the sites MISSING at random and the rest EXACT, the true value supplied at every missing site;
  * mpst_marginal_conditionals on that second input: the baseline the EXACT / MISSING call should cost about as much as.
Median of 7 calls after 2 warm-ups on one GPU; `device` is the call's own `seconds` (events around its kernels), the split is
mpst_get_impute_phases: (operators + walk, grid phase) for the new call, (walk, grid phase) for the baseline.
usage: python profiles/observed_conditionals_timing.py [--out FILE]"""
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
    sd = 10 * (xs[1] - xs[0])
    gauss = mt.gaussian_noise(np.clip(x + sd * rng.standard_normal((N, T)), -1.0, 1.0), sd)
    z = np.zeros((N, T))
    hard = mt.ObservationModel(miss.astype(np.uint8), np.where(miss, 0.0, x), z)
    prods = 2 * D * (T - 1) + 2 * D * T + 2 * D * (T - 1)
    lines = [f"observed conditionals of N={N} series: T={T} chi={CHI} d={D} C={NC} fp64, ngrid={NGRID}, levels {LEVELS} and the WMAD, both groups; "
             f"median of {REPS} after {WARM} warm-ups, one MI355X",
             f"{'call':<66}{'device ms (min .. max)':>34}{'split ms':>38}"]
    eng = mt.SweepEngine(0)
    try:
        dev, lo, hi, ph = timed(lambda: eng.observed_conditionals(W, phi, lab, gauss, None, xs, gphi, levels=LEVELS).seconds, eng.impute_phases)
        lines.append(f"{f'mpst_observed_conditionals, every site GAUSS ({prods} products / series)':<66}"
                     f"{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}{f'operators + walk {ph[0] * 1e3:.3f} + grid {ph[1] * 1e3:.3f}':>38}")
        dev_o, lo, hi, ph = timed(lambda: eng.observed_conditionals(W, phi, lab, hard, x, xs, gphi, levels=LEVELS).seconds, eng.impute_phases)
        lines.append(f"{f'mpst_observed_conditionals, {miss.mean() * 100:.1f} % MISSING, the rest EXACT':<66}"
                     f"{f'{dev_o * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}{f'operators + walk {ph[0] * 1e3:.3f} + grid {ph[1] * 1e3:.3f}':>38}")
        dev_m, lo, hi, ph = timed(lambda: eng.marginal_conditionals(W, phi, lab, miss, x, xs, gphi, levels=LEVELS).seconds, eng.impute_phases)
        lines.append(f"{'mpst_marginal_conditionals on that input (the baseline)':<66}{f'{dev_m * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}"
                     f"{f'walk {ph[0] * 1e3:.3f} + grid {ph[1] * 1e3:.3f}':>38}")
        lines.append(f"EXACT / MISSING call over the baseline: {dev_o / dev_m:.3f}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
