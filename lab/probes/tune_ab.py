"""tune() against the plain loop it replaces (fitMPS + eval_loss, one fit at a time), in one process on one device, the two legs
alternating.  Shape: 5 folds x 8 candidates (eta) at chi_max = 32, d = 4, T = 100, a few hundred series per fold, 3 sweeps.
Wall times (median and spread over the repeats, every shape warmed up first, no profiler attached) and the launch count of a
scoring call against T + 2 per model go to --out (default profiles/tune_ab.json).  The rocprofv3 row of k_score_walk_b comes from a
run of its own:  rocprofv3 --kernel-trace --stats -- python lab/probes/tune_ab.py --repeats 1 --out /dev/null

    python lab/probes/tune_ab.py [--repeats 5] [--out profiles/tune_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import mpstime_jl_amd as mt                      # noqa: E402
from mpstime_jl_amd import tuning as tu          # noqa: E402


def data(n=500, T=100, seed=5):
    rng = np.random.default_rng(seed)
    X0, _ = mt.trendy_sine(T, n // 2 + 1, period=(20.0, 30.0), slope=(-2.0, 0.0), sigma=0.1, rng=rng)
    X1, _ = mt.trendy_sine(T, n - n // 2 - 1, period=(35.0, 50.0), slope=(0.0, 2.0), sigma=0.1, rng=rng)
    y = np.r_[np.zeros(len(X0), dtype=np.int64), np.ones(len(X1), dtype=np.int64)]
    p = rng.permutation(n)
    return np.vstack([X0, X1])[p], y[p]


def plain_loop(X, y, folds, opts_list, obj):
    out = []
    for o in opts_list:
        ls = []
        for tr, va in folds:
            m, _, _ = mt.fitMPS(X[tr], y[tr], opts=o, batch_hint=tu.BATCH_HINT)
            ls.append(float(np.mean(mt.eval_loss(obj, m, X[va], y[va]))))
        out.append(float(np.mean(ls)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "tune_ab.json"))
    a = ap.parse_args()
    X, y = data()
    folds = mt.make_stratified_cvfolds(X, y, 5, rng=1)
    obj = mt.MisclassificationRate()
    opts0 = mt.MPSOptions(verbosity=-5, log_level=-1, d=4, chi_max=32, nsweeps=3)
    etas = [0.005, 0.01, 0.02, 0.03, 0.05, 0.07, 0.1, 0.2]
    params = {"eta": etas}
    search = mt.MPSRandomSearch("Exhaustive")

    def leg_tune():
        return mt.tune(X, y, 5, params, search, objective=obj, opts0=opts0, foldmethod=folds, verbosity=0, return_info=True)

    def leg_loop():
        return plain_loop(X, y, folds, [opts0.set(eta=e) for e in etas], obj)

    best, cache, info = leg_tune()               # warm-up of both legs: every shape has been compiled, allocated and captured
    ref = leg_loop()
    worst = max(abs(cache[(e,)] - r) for e, r in zip(etas, ref))
    t_tune, t_loop = [], []
    for _ in range(a.repeats):                   # alternating legs
        t0 = time.perf_counter(); leg_tune(); t_tune.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); leg_loop(); t_loop.append(time.perf_counter() - t0)
    T = X.shape[1]
    res = {"shape": {"folds": 5, "candidates": len(etas), "chi_max": 32, "d": 4, "T": T, "series_per_fold_train": len(folds[0][0]), "nsweeps": 3},
           "tune_seconds": {"median": statistics.median(t_tune), "min": min(t_tune), "max": max(t_tune), "runs": t_tune},
           "plain_loop_seconds": {"median": statistics.median(t_loop), "min": min(t_loop), "max": max(t_loop), "runs": t_loop},
           "speedup_of_medians": statistics.median(t_loop) / statistics.median(t_tune),
           "largest_loss_difference": worst, "info": info,
           "launches_per_scoring_call": {"classify_batch": 2, "per_model_path": (T + 2) * info["fits"], "models": info["fits"]}}
    print(json.dumps(res))
    if a.out != "/dev/null":
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
