#!/usr/bin/env python3
"""One timing of mpst_rolling_forecasts beside the route it replaces, no threshold: N = 256, T = 100, chi = 32, d = 4,
C = 2, label last, max_horizon = 16, ngrid = 2001, three levels and the WMAD, fp64, a random normalised MPS, Legendre states.  The
other route is mpst_marginal_conditionals on the 256 * 100 = 25 600 suffix-masked replicas (replica (t, i) is series i with the sites
t .. T-1 masked and the true values supplied), in the same process on the same GPU; it computes all T conditionals of a replica, of
which the H from the origin on are read.  Median of 7 calls after 2 warm-ups.  `device` is the call's own `seconds` (events around its
kernels), the phases are mpst_get_impute_phases after the call, `host` a host clock around the whole call, which includes packing and
uploading the model and the states - 100 times as many states on the replica route.
usage: python profiles/rolling_timing.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpstime_jl_amd as mt                                                      # noqa: E402
from mpstime_jl_amd.conditionals import marginal_conditionals_model              # noqa: E402

N, T, CHI, D, NC, H, NGRID, REPS, WARM = 256, 100, 32, 4, 2, 16, 2001, 7, 2
LEVELS = (0.05, 0.5, 0.95)


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
    rng = np.random.default_rng(28)
    W = mt.generate_startingMPS(CHI, T, D, NC, init_rng=28)
    assert all(np.all(np.isfinite(t)) for t in W)
    x = rng.uniform(-1, 1, (N, T))
    phi = mt.legendre_encode_no_norm(x, D)
    xs = np.linspace(-1.0, 1.0, NGRID)
    gp = mt.legendre_encode_no_norm(xs, D)
    lab = (np.arange(N) % NC).astype(np.int32)
    rep_phi, rep_x, rep_lab = np.tile(phi, (T, 1, 1)), np.tile(x, (T, 1)), np.tile(lab, T)       # replica t * N + i: origin t of series i
    rep_mask = np.repeat(np.arange(T)[None, :] >= np.arange(T)[:, None], N, axis=0)
    lines = [f"mpst_rolling_forecasts vs mpst_marginal_conditionals on {N} * {T} suffix-masked replicas: N={N} T={T} chi={CHI} d={D} C={NC} "
             f"max_horizon={H} ngrid={NGRID} levels={len(LEVELS)} wmad fp64, median of {REPS} after {WARM} warm-ups, one MI355X",
             f"{'call':<56}{'device ms (min .. max)':>32}{'host ms':>12}"]
    eng = mt.SweepEngine(0)
    try:
        out = {}
        devs = {}
        for mode, labels in (("label", lab), ("mixture", np.full(N, -1, dtype=np.int32))):
            def new(labels=labels, mode=mode):
                out[mode] = eng.rolling_model(W, phi, labels, H, x, xs, gp, levels=LEVELS)
                return out[mode][6], eng.impute_phases()
            dev, host, lo, hi, ph = timed(new)
            devs[mode] = (dev, host)
            first, grid = statistics.median(p[0] for p in ph), statistics.median(p[1] for p in ph)
            lines.append(f"{f'mpst_rolling_forecasts, {mode} mode':<56}{f'{dev * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>32}{host * 1e3:>12.3f}")
            lines.append(f"{'  tables + rows + score (k_prefix_env, k_roll_rows / _tables / _score)':<72}{first * 1e3:>16.3f}")
            lines.append(f"{'  grid phase (k_roll_grid)':<72}{grid * 1e3:>16.3f}")

        def old():
            out["rep"] = marginal_conditionals_model(eng, W, rep_phi, rep_lab, rep_mask, rep_x, xs, gp, levels=LEVELS)
            return out["rep"].seconds, eng.impute_phases()
        dev_old, host_old, lo, hi, ph = timed(old)
        lines.append(f"{f'mpst_marginal_conditionals, {N * T} replicas':<56}{f'{dev_old * 1e3:.3f} ({lo * 1e3:.3f} .. {hi * 1e3:.3f})':>32}{host_old * 1e3:>12.3f}")
        lines.append(f"{'  walk (k_mc_walk)':<72}{statistics.median(p[0] for p in ph) * 1e3:>16.3f}")
        lines.append(f"{'  grid phase (k_mc_grid)':<72}{statistics.median(p[1] for p in ph) * 1e3:>16.3f}")
        dev_new, host_new = devs["label"]
        lines.append(f"replica route / rolling call (label mode): device {dev_old / dev_new:.1f}x, host {host_old / host_new:.1f}x")
        nll, pit, med, err, mean, q, _ = out["label"]
        rep = out["rep"]
        gaps = dict(nll=0.0, pit=0.0, mean=0.0)
        differ = total = 0
        for t in range(T):
            for h in range(min(H, T - t)):
                r = slice(t * N, (t + 1) * N)
                u = t + h
                gaps["nll"] = max(gaps["nll"], float(np.abs(nll[:, t, h] - rep.nll[r, u]).max()))
                gaps["pit"] = max(gaps["pit"], float(np.abs(pit[:, t, h] - rep.pit[r, u]).max()))
                gaps["mean"] = max(gaps["mean"], float(np.abs(mean[:, t, h] - rep.mean[r, u]).max()))
                differ += int((med[:, t, h] != rep.median[r, u]).sum() + (err[:, t, h] != rep.err[r, u]).sum() + (q[:, t, h] != rep.quantiles[r, u]).sum())
                total += 5 * N
        inside = np.arange(T)[:, None] + np.arange(1, H + 1)[None, :] <= T
        assert np.all(np.isfinite(nll[:, inside])) and np.all(np.isnan(nll[:, ~inside]))
        lines.append(f"largest disagreement of the two routes: nll {gaps['nll']:.3e}, pit {gaps['pit']:.3e}, mean {gaps['mean']:.3e}; "
                     f"{differ} of {total} selected grid values (median, WMAD, levels) differ")
    finally:
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
