"""Probe: see_variation series per second and executed fp64 GFLOP/s of the density walk (csrc/mpst_analysis.hip) at
(T=100, chi=32, d=4, 64 series) and at the reference's ECG200 shape (T=96, chi=25, d=5, its first 64 training series), plus
the NumPy restatement (tests/analysis_ref.py) on one series on the CPU.  Run it under
`rocprofv3 --kernel-trace --stats -- python lab/probes/analysis_rate.py --no-cpu` for the per-kernel split.
usage: analysis_rate.py [--no-cpu] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import mpstime_jl_amd as mt                     # noqa: E402
from tests import analysis_ref as A             # noqa: E402


def walk_flops(chi, d, n):
    """Executed flops of the walk for n series: every chain (series, k) runs sites k..T-1, each site d products L B^s
    (2 chi_l^2 chi_r), d products B^sT X (2 chi_l chi_r^2) and d^2 Frobenius products (2 chi_l chi_r)."""
    T = len(chi) - 1
    per_site = [d * (2 * chi[j] ** 2 * chi[j + 1] + 2 * chi[j] * chi[j + 1] ** 2 + 2 * d * chi[j] * chi[j + 1]) for j in range(T)]
    suffix = np.cumsum(per_site[::-1])[::-1]          # sum over j >= k
    return float(n * suffix.sum())


def canonical_chi(W):
    """Bond dimensions after the right-canonical pass: min(chi_l, d chi_r) from the right."""
    T, d = len(W), W[0].shape[1]
    chi = [W[0].shape[0]] + [t.shape[2] for t in W]
    for j in range(T - 1, 0, -1):
        chi[j] = min(chi[j], d * chi[j + 1])
    return chi


def rate(tm, X, cls, eng, reps=5):
    mt.see_variation(tm, X[:2], cls, engine=eng)                     # warm-up (code objects, allocations)
    secs = []
    for _ in range(reps):
        _, s = mt.see_variation(tm, X, cls, engine=eng, return_seconds=True)
        secs.append(s)
    s = float(np.median(secs))
    fl = walk_flops(canonical_chi(tm.mps), tm.mps[0].shape[1], len(X))
    return {"series": len(X), "device_s_median": s, "device_s_all": secs, "series_per_s": len(X) / s,
            "walk_gflop": fl / 1e9, "walk_gflops_per_s": fl / s / 1e9}


def main():
    out = {}
    eng = mt.SweepEngine(0)
    try:
        rng = np.random.default_rng(0)
        T, chi, d = 100, 32, 4
        W = mt.generate_startingMPS(chi, T, d, 2, 1234)
        X = rng.uniform(-1, 1, (64, T))
        y = np.zeros(64, dtype=np.int64)
        td = mt.EncodedTimeSeriesSet(np.zeros((64, T, d)), y, y.astype(np.int32), X, np.array([64]))
        tm = mt.TrainedMPS(W, mt.MPSOptions(d=d, chi_max=chi, verbosity=-1), td)
        out["T100_chi32_d4"] = rate(tm, X, 0, eng)
        ecg = mt.load_trained_mps(os.path.join(ROOT, "tests", "golden", "ref_test_dataset.jld2"))
        out["ecg200_T96_chi25_d5"] = rate(ecg, ecg.train_data.original_data[:64], 1, eng)
        t0 = time.perf_counter()
        mt.bipartite_spectrum(ecg, engine=eng)
        mt.single_site_spectrum(ecg, engine=eng)
        out["ecg200_bee_plus_see_wall_s"] = time.perf_counter() - t0
    finally:
        eng.close()
    if "--no-cpu" not in sys.argv:
        opts = mt.options.safe_options(tm.opts)
        enc = mt.model_encoding(opts.encoding)
        _, norms = mt.transform_train_data(X, opts, enc.range)
        phi = enc.encode(mt.transform_test_data(X[:1], norms, opts, enc.range)[0], d)
        t0 = time.perf_counter()
        A.see_variation_encoded(A.expand_label_index(W)[0], phi)
        out["cpu_restatement_one_series_T100_chi32_d4_s"] = time.perf_counter() - t0
    print(json.dumps(out, indent=1))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
