#!/usr/bin/env python3
"""One timing of mpst_segment_marginals beside the route it replaces, no threshold: N = 256, T = 100, chi = 32, d = 4,
C = 2, label last, max_width = 16, fp64, a random normalised MPS, Legendre states.  The other route is mpst_marginal_model on the
256 * 1480 = 378 880 complement-masked replicas (replica (i, a, w) is series i with every site outside a .. a+w-1 masked), in the same
process on the same GPU.  Median of 7 calls after 2 warm-ups.  `device` is the call's own `seconds` (events around its kernels), the
phases are mpst_get_impute_phases after the call (table kernels, walk kernel), `host` a host clock around the whole call, which
includes packing and uploading the model and the states - 1480 times as many states on the replica route.
usage: python profiles/segment_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402

N, T, CHI, D, NC, MW, REPS, WARM = 256, 100, 32, 4, 2, 16, 7, 2


def timed(fn):
    dev, host, extra = [], [], []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        s, x = fn()
        t1 = time.perf_counter()
        if k >= WARM:
            dev.append(s)
            host.append(t1 - t0)
            extra.append(x)
    return statistics.median(dev), statistics.median(host), min(dev), max(dev), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(27)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=27)
    assert all(np.all(np.isfinite(t)) for t in W)
    phi = mt.legendre_encode_no_norm(rng.uniform(-1, 1, (N, T)), D)
    segs = [(s, w) for s in range(T) for w in range(1, MW + 1) if s + w <= T]
    rep_phi = np.tile(phi, (len(segs), 1, 1))                                     # replica k * N + i: segment k of series i
    rep_mask = np.ones((len(segs), N, T), dtype=np.uint8)
    for k, (s, w) in enumerate(segs):
        rep_mask[k, :, s:s + w] = 0
    rep_mask = rep_mask.reshape(len(segs) * N, T)
    lines = [f"mpst_segment_marginals vs mpst_marginal_model on {N} * {len(segs)} complement-masked replicas: N={N} T={T} chi={CHI} d={D} C={NC} "
             f"max_width={MW} fp64, median of {REPS} after {WARM} warm-ups, one MI355X",
             f"{'call':<50}{'device ms (min .. max)':>30}{'host ms':>12}"]
    eng = mt.SweepEngine(0)
    try:
        out = {}

        def new(out=out):
            out["lp"], _, s = eng.segment_model(W, phi, MW)
            return s, eng.impute_phases()
        dev_new, host_new, lo, hi, ph = timed(new)
        tab, walk = statistics.median(p[0] for p in ph), statistics.median(p[1] for p in ph)
        lines.append(f"{'mpst_segment_marginals':<50}{f'{dev_new * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>30}{host_new * 1e3:>12.3f}")
        lines.append(f"{'  table kernels (k_segment_left, k_prefix_env)':<50}{tab * 1e3:>30.3f}")
        lines.append(f"{'  walk kernel (k_segment_walk)':<50}{walk * 1e3:>30.3f}")

        def old(out=out):
            out["rep"], s = eng.marginal_model(W, rep_phi, rep_mask)
            return s, None
        dev_old, host_old, lo, hi, _ = timed(old)
        lines.append(f"{f'mpst_marginal_model, {N * len(segs)} replicas':<50}{f'{dev_old * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>30}{host_old * 1e3:>12.3f}")
        lines.append(f"replica route / segment call: device {dev_old / dev_new:.1f}x, host {host_old / host_new:.1f}x")
        rep = out["rep"].reshape(len(segs), N, NC)
        gap = max(float(np.abs(out["lp"][:, s, w - 1] - rep[k]).max()) for k, (s, w) in enumerate(segs))
        inside = np.array([[s + w <= T for w in range(1, MW + 1)] for s in range(T)])
        assert np.all(np.isfinite(out["lp"][:, inside])) and np.all(np.isnan(out["lp"][:, ~inside]))
        lines.append(f"largest |ln l (segment call) - ln l (replica route)|: {gap:.3e}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
