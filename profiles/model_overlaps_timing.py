#!/usr/bin/env python3
"""Timings of mpst_model_overlaps, no threshold; random normalised MPS of generate_startingMPS, fp64, one MI355X, one
process.  `device` is the call's own `seconds` (events around its launches), the median of 7 calls after 2 warm-ups.
  1. K = 1, C = 4, T = 100, chi = 32, d = 4: the class overlap matrix of the headline model; beside it the wall time of the NumPy
     restatement (tests/overlap_ref.py) on the host of the same box.
  2. K = 32 of that shape, all 528 pairs in one call, and the same 528 pairs as 528 calls of one pair each (the sum of their device
     seconds and the host's clock over the loop).  The flops of the two GEMMs of every site, 2 d (chi_a_l chi_b_l chi_b_r + chi_a_r
     chi_a_l chi_b_r) with the bonds as they are (not padded), over the device time, against the 78.6 TF/s fp64 matrix peak.
  3. K = 8 at T = 200, chi = 64, d = 8, C = 4, real and complex (a complex multiply-add counts four real ones).
usage: python profiles/model_overlaps_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402
from mpstime_jl_amd import overlaps as OV                                        # noqa: E402
from tests import overlap_ref as R                                               # noqa: E402

REPS, WARM, PEAK = 7, 2, 78.6e12


def flops(models, pairs, cx):
    tot = 0.0
    for a, b in pairs:
        ca = [models[a][0].shape[0]] + [t.shape[2] for t in models[a]]
        cb = [models[b][0].shape[0]] + [t.shape[2] for t in models[b]]
        d = models[a][0].shape[1]
        tot += sum(2.0 * d * (ca[j] * cb[j] * cb[j + 1] + ca[j + 1] * ca[j] * cb[j + 1]) for j in range(len(ca) - 1))
    return tot * (4 if cx else 1)


def timed(eng, models, table, cx):
    dev, wall = [], []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        _, _, sec = OV.overlaps_raw(eng, models, table, cx)
        if k >= WARM:
            dev.append(sec)
            wall.append(time.perf_counter() - t0)
    return statistics.median(dev), min(dev), max(dev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"model overlaps, fp64, one MI355X; device = the call's seconds, median of {REPS} after {WARM} warm-ups"]
    eng = mt.SweepEngine(0)
    try:
        models = [mt.generate_startingMPS(32, 100, 4, 4, init_rng=100 + k) for k in range(32)]
        med, lo, hi, wall = timed(eng, models[:1], None, False)
        t0 = time.perf_counter()
        R.normalised_ref(models[:1])
        host = time.perf_counter() - t0
        lines.append(f"1. K=1 C=4 T=100 chi=32 d=4: device {med * 1e3:.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), the call on the host's clock "
                     f"{wall * 1e3:.3f} ms; NumPy restatement on the host {host * 1e3:.1f} ms")
        pairs = [(x, y) for x in range(32) for y in range(x, 32)]
        med, lo, hi, wall = timed(eng, models, None, False)
        fl = flops(models, pairs, False)
        lines.append(f"2. K=32, 528 pairs, one call: device {med * 1e3:.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), host's clock {wall * 1e3:.1f} ms; "
                     f"{fl:.3e} flop = {fl / med / 1e12:.2f} TF/s = {fl / med / PEAK:.4f} of the {PEAK / 1e12:.1f} TF/s fp64 matrix peak")
        one = np.array([[0, 1]], dtype=np.int32)
        same = np.array([[0, 0]], dtype=np.int32)
        devs, walls = [], []
        for k in range(1 + 3):
            t0 = time.perf_counter()
            tot = 0.0
            for x, y in pairs:
                tot += OV.overlaps_raw(eng, [models[x]] if x == y else [models[x], models[y]], same if x == y else one, False)[2]
            if k >= 1:
                devs.append(tot)
                walls.append(time.perf_counter() - t0)
        lines.append(f"   the same 528 pairs as 528 calls: device {statistics.median(devs) * 1e3:.3f} ms summed, host's clock {statistics.median(walls) * 1e3:.1f} ms "
                     f"(median of 3 after 1 warm-up)")
        for cx in (False, True):
            big = [mt.generate_startingMPS(64, 200, 8, 4, init_rng=200 + k, dtype=np.complex128 if cx else np.float64) for k in range(8)]
            bp = [(x, y) for x in range(8) for y in range(x, 8)]
            med, lo, hi, wall = timed(eng, big, None, cx)
            fl = flops(big, bp, cx)
            lines.append(f"3. K=8 T=200 chi=64 d=8 C=4 {'complex' if cx else 'real'}, 36 pairs: device {med * 1e3:.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), "
                         f"host's clock {wall * 1e3:.1f} ms; {fl:.3e} flop = {fl / med / 1e12:.2f} TF/s = {fl / med / PEAK:.4f} of the peak")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
