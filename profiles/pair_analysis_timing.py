#!/usr/bin/env python3
"""One timing of mpst_pair_analysis, no threshold: T = 100, d = 4, chi = 32, C = 2, fp64, a random MPS, a random
symmetric observable per site, all three outputs.  Median of 7 calls after 2 warm-ups in one process on one GPU; `device` is the
call's own `seconds` (events around its kernels), the split is mpst_get_impute_phases: (k_an_pair, k_an_pair_ent); the rest of the
device time is k_an_canon, the left-density walk and the padded copy of the tensors.  The flop count of the pair walk,
C T (T-1)/2 * d (d+1)/2 * d * 4 chi^3, over the k_an_pair time is set against the 78.6 TF/s fp64 matrix peak.  The only comparison is
the recursion as NumPy matrix products (tests/pair_ref.py: transfer) for ONE class on the host of the same box.
usage: python profiles/pair_analysis_timing.py [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402
from mpstime_jl_amd import analysis                                              # noqa: E402
from tests import pair_ref as P                                                  # noqa: E402

T, CHI, D, NC, REPS, WARM = 100, 32, 4, 2, 7, 2
PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=20)
    rng = np.random.default_rng(20)
    O = rng.standard_normal((T, D, D))
    O = np.ascontiguousarray(0.5 * (O + O.transpose(0, 2, 1)))
    m = analysis._Model(W)
    mi, mean, cov = np.zeros((NC, T, T)), np.zeros((NC, T)), np.zeros((NC, T, T))
    dp = C.POINTER(C.c_double)
    sec = C.c_double()
    eng = mt.SweepEngine(0)
    dev, ph, wall = [], [], []
    try:
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            rc = eng.lib.mpst_pair_analysis(eng.ctx, C.byref(m.struct), O.ctypes.data_as(dp), 1, mi.ctypes.data_as(dp), mean.ctypes.data_as(dp),
                                            cov.ctypes.data_as(dp), C.byref(sec))
            t1 = time.perf_counter()
            assert rc == 0, eng.lib.mpst_last_error(eng.ctx)
            if k >= WARM:
                dev.append(sec.value)
                ph.append(eng.impute_phases())
                wall.append(t1 - t0)
    finally:
        eng.close()
    med = statistics.median(dev)
    p = ph[dev.index(sorted(dev)[len(dev) // 2])]
    flops = NC * T * (T - 1) / 2 * D * (D + 1) / 2 * D * 4 * CHI ** 3
    one = [t[..., :1] if t.ndim == 4 else t for t in W]
    t0 = time.perf_counter()
    hmi, hmean, hcov = P.transfer(one, O)
    host = time.perf_counter() - t0
    worst = max(float(np.abs(x[0] - y[0]).max()) for x, y in ((mi, hmi), (mean, hmean), (cov, hcov)))
    lines = [f"pair analysis: T={T} chi={CHI} d={D} C={NC} fp64, mi + mean + cov; median of {REPS} after {WARM} warm-ups, one MI355X",
             f"device {med * 1e3:.3f} ms ({min(dev) * 1e3:.3f} .. {max(dev) * 1e3:.3f}); k_an_pair {p[0] * 1e3:.3f} ms + k_an_pair_ent {p[1] * 1e3:.3f} ms; "
             f"the call on the host's clock {statistics.median(wall) * 1e3:.3f} ms",
             f"pair walk: {flops:.3e} flop / {p[0] * 1e3:.3f} ms = {flops / p[0] / 1e12:.2f} TF/s = {flops / p[0] / PEAK:.3f} of the {PEAK / 1e12:.1f} TF/s fp64 matrix peak",
             f"NumPy matrix-product recursion, one class, on the host: {host:.2f} s; largest |device - host| over mi, mean, cov of class 0: {worst:.2e}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
