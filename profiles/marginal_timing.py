#!/usr/bin/env python3
"""One timing of mpst_marginal_model beside mpst_classify, no threshold: N = 4096, T = 100, chi = 32, d = 4, C = 2,
fp64, a random normalised MPS, Legendre states; 0 % and 30 % of the values missing (scattered at random).  Median of 7 calls after
2 warm-ups, all in one process on one GPU.  `device` is the call's own `seconds` (events around its kernels), `host` a host clock
around the whole call, which for mpst_marginal_model includes packing and uploading the model and the states and for
mpst_classify only the launch, the synchronise and the copy of the result (its data set and MPS are resident).
usage: python profiles/marginal_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402
from mpstime_jl_amd.options import engine_options, safe_options                   # noqa: E402

N, T, CHI, D, NC, REPS, WARM = 4096, 100, 32, 4, 2, 7, 2


def timed(fn):
    dev, host = [], []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        s = fn()
        t1 = time.perf_counter()
        if k >= WARM:
            dev.append(s)
            host.append(t1 - t0)
    return statistics.median(dev), statistics.median(host), min(dev), max(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(18)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=18)
    assert all(np.all(np.isfinite(t)) for t in W)
    phi = mt.legendre_encode_no_norm(rng.uniform(-1, 1, (N, T)), D)
    masks = {"0 % missing": None, "30 % missing": rng.random((N, T)) < 0.3}
    lines = [f"mpst_marginal_model vs mpst_classify: N={N} T={T} chi={CHI} d={D} C={NC} fp64, median of {REPS} after {WARM} warm-ups, one MI355X",
             f"{'call':<42}{'device ms (min .. max)':>30}{'host ms':>12}"]
    eng = mt.SweepEngine(0)
    try:
        ref = None
        for name, m in masks.items():
            out = {}

            def call(m=m, out=out):
                out["lp"], s = eng.marginal_model(W, phi, m)
                return s
            dev, host, lo, hi = timed(call)
            assert np.all(np.isfinite(out["lp"]))
            if m is None:
                ref = out["lp"]
            lines.append(f"{'mpst_marginal_model, ' + name:<42}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>30}{host * 1e3:>12.3f}")
        eng.set_options(**engine_options(safe_options(mt.MPSOptions(d=D, chi_max=CHI, verbosity=-1))))
        eng.set_dataset(0, phi[:1], np.zeros(1, dtype=np.int32), NC)
        eng.set_dataset(1, phi, np.zeros(N, dtype=np.int32), NC)
        eng.set_mps(W)
        res = {}

        def cls(res=res):
            res["pred"], res["yh"] = eng.classify(1, return_overlaps=True)
            return float("nan")
        _, host, _, _ = timed(cls)
        lines.append(f"{'mpst_classify, complete set (resident)':<42}{'(no device clock)':>30}{host * 1e3:>12.3f}")
        gap = float(np.abs(ref - np.log(np.abs(res["yh"]) ** 2)).max())
        lines.append(f"largest |ln l_c - ln |yhat_c|^2| on the complete set: {gap:.3e}; argmax agrees on "
                     f"{int((np.argmax(ref, axis=1) == res['pred']).sum())} of {N}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
