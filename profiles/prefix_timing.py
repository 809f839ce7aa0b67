#!/usr/bin/env python3
"""One timing of mpst_prefix_marginals beside the route it replaces, no threshold: N = 256, T = 100, chi = 32, d = 4,
C = 2, fp64, a random normalised MPS, Legendre states.  The other route is mpst_marginal_model on the 256 * 101 suffix-masked
replicas (replica (i, t) is series i with the sites t .. T-1 masked), in the same process on the same GPU.  Median of 7 calls after
2 warm-ups.  `device` is the call's own `seconds` (events around its kernels), the phases are mpst_get_impute_phases after the call
(environment kernel, walk-and-score kernel), `host` a host clock around the whole call, which includes packing and uploading the
model and the states - 101 times as many states on the replica route.
usage: python profiles/prefix_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402

N, T, CHI, D, NC, REPS, WARM = 256, 100, 32, 4, 2, 7, 2


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
    rng = np.random.default_rng(24)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=24)
    assert all(np.all(np.isfinite(t)) for t in W)
    phi = mt.legendre_encode_no_norm(rng.uniform(-1, 1, (N, T)), D)
    rep_phi = np.repeat(phi, T + 1, axis=0)                                       # replica i * (T + 1) + t
    rep_mask = np.tile(np.arange(T)[None, :] >= np.arange(T + 1)[:, None], (N, 1))
    lines = [f"mpst_prefix_marginals vs mpst_marginal_model on {N} * {T + 1} suffix-masked replicas: N={N} T={T} chi={CHI} d={D} C={NC} fp64, "
             f"median of {REPS} after {WARM} warm-ups, one MI355X",
             f"{'call':<50}{'device ms (min .. max)':>30}{'host ms':>12}"]
    eng = mt.SweepEngine(0)
    try:
        out = {}

        def new(out=out):
            out["lp"], s = eng.prefix_model(W, phi)
            return s, eng.impute_phases()
        dev_new, host_new, lo, hi, ph = timed(new)
        env, walk = statistics.median(p[0] for p in ph), statistics.median(p[1] for p in ph)
        lines.append(f"{'mpst_prefix_marginals':<50}{f'{dev_new * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>30}{host_new * 1e3:>12.3f}")
        lines.append(f"{'  environment kernel (k_prefix_env)':<50}{env * 1e3:>30.3f}")
        lines.append(f"{'  walk-and-score kernel (k_prefix_score)':<50}{walk * 1e3:>30.3f}")

        def old(out=out):
            out["rep"], s = eng.marginal_model(W, rep_phi, rep_mask)
            return s, None
        dev_old, host_old, lo, hi, _ = timed(old)
        lines.append(f"{f'mpst_marginal_model, {N * (T + 1)} replicas':<50}{f'{dev_old * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>30}{host_old * 1e3:>12.3f}")
        lines.append(f"replica route / prefix call: device {dev_old / dev_new:.1f}x, host {host_old / host_new:.1f}x")
        assert np.all(np.isfinite(out["lp"]))
        gap = float(np.abs(out["lp"] - out["rep"].reshape(N, T + 1, NC)).max())
        lines.append(f"largest |ln l (prefix call) - ln l (replica route)|: {gap:.3e}")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
