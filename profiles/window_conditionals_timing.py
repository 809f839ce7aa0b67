#!/usr/bin/env python3
"""One timing of mpst_window_conditionals beside the route that gives the same scores without it, no threshold:
N = 256 complete series, T = 100, chi = 32, d = 4, C = 2, fp64, a random normalised MPS, Legendre states, max_width = 16.  The other
route is mpst_marginal_model on the window-masked replicas - one per (series, start, width), 378 880 of them, plus the N complete
series - minus its value on the complete series, batched into calls of at most 2^17 replicas (420 MB of encoded states each on the host
and again on the device).  Median of 7 passes after 2 warm-ups, all in one process on one GPU; `device` is the calls' own `seconds`
(events around their kernels; the composed route: the sum over its calls), the split is mpst_get_impute_phases: (walk, window kernel).
usage: python profiles/window_conditionals_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402

N, T, CHI, D, NC, MW, REPS, WARM, PER_CALL = 256, 100, 32, 4, 2, 16, 7, 2, 1 << 17


def timed(fn, phases=None):
    dev, ph = [], []
    for k in range(WARM + REPS):
        s = fn()
        if k >= WARM:
            dev.append(s)
            ph.append(phases() if phases else None)
    return statistics.median(dev), min(dev), max(dev), ph[dev.index(sorted(dev)[len(dev) // 2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(22)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=22)
    x = rng.uniform(-0.95, 0.95, (N, T))
    phi = mt.legendre_encode_no_norm(x, D)
    lab = (np.arange(N) % NC).astype(np.int32)
    wins = np.array([(i, t, w) for i in range(N) for t in range(T) for w in range(1, min(MW, T - t) + 1)], dtype=np.int64)
    lines = [f"window conditionals of N={N} series: T={T} chi={CHI} d={D} C={NC} fp64, max_width={MW} ({len(wins)} windows); median of {REPS} "
             f"after {WARM} warm-ups, one MI355X",
             f"{'route':<64}{'device ms (min .. max)':>34}{'split ms':>30}"]
    eng = mt.SweepEngine(0)
    try:
        out = {}

        def new():
            out["new"], s = eng.window_conditionals(W, phi, lab, MW)
            return s
        dev, lo, hi, ph = timed(new, eng.impute_phases)
        lines.append(f"{'mpst_window_conditionals':<64}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}"
                     f"{f'walk {ph[0] * 1e3:.3f} + window {ph[1] * 1e3:.3f}':>30}")
        # the composed route: the complete series once, then the masked replicas in as few calls as PER_CALL allows
        batches = []
        for b0 in range(0, len(wins), PER_CALL):
            sel = wins[b0:b0 + PER_CALL]
            mask = np.zeros((len(sel), T), dtype=np.uint8)
            cols = np.arange(T)[None, :]
            mask[(cols >= sel[:, 1:2]) & (cols < sel[:, 1:2] + sel[:, 2:3])] = 1
            batches.append((sel, np.ascontiguousarray(phi[sel[:, 0]]), mask))

        def old():
            full, s = eng.marginal_model(W, phi, None)
            res = np.full((N, T, MW), np.nan)
            for sel, ph_, mask in batches:
                logp, s1 = eng.marginal_model(W, ph_, mask)
                s += s1
                res[sel[:, 0], sel[:, 1], sel[:, 2] - 1] = logp[np.arange(len(sel)), lab[sel[:, 0]]] - full[sel[:, 0], lab[sel[:, 0]]]
            out["old"] = res
            return s
        dev2, lo, hi, _ = timed(old)
        lines.append(f"{'mpst_marginal_model, masked replicas in ' + str(len(batches)) + ' calls + the complete series':<64}"
                     f"{f'{dev2 * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>34}{'-':>30}")
        ok = ~np.isnan(out["old"])
        lines.append(f"NaN in the same places: {bool(np.array_equal(np.isnan(out['new']), ~ok))}; largest |difference| of the two results "
                     f"{np.abs(out['new'][ok] - out['old'][ok]).max():.3e}; ratio of the device times {dev2 / dev:.1f}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
