"""A/B of the imputation engine's table route with and without a per-site grid table (mpst_impute_opts.grid_per_site): the median
imputer on one model and mask (N = 512, T = 32, 16 missing sites each, chi = 32, d = 8 real Legendre, 20 001 grid values nudged off
the uniform spacing so that the table route runs) through the shared table and - `new` only - through a per-site table holding T
copies of it: the same kernel with site stride 0 against ngrid * d.  Median / min / max of 7 device timings after 2 warm-up calls.
    python lab/probes/impute_per_site_ab.py new                    # this tree's library: shared, then per-site
    python lab/probes/impute_per_site_ab.py <parent's libmpstime_hip.so>   # a library built from the parent commit: shared only
Run the two alternately (parent, new, parent, new) on one device; profiles/impute_per_site_ab.txt holds such a run."""
import sys
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
which = sys.argv[1]
import mpstime_jl_amd as mt
from mpstime_jl_amd import _lib as L
if which != "new":
    L.LIB_PATH = which
    for k in ("mpst_encode_split_dataset", "mpst_encode_split_values"):
        L.SYMBOLS.pop(k)
from oracle import ref_numpy as R
rng = np.random.default_rng(5)
N, T, d, chi, ngrid = 512, 32, 8, 32, 20001
W = R.random_mps(T, d, chi, 1, rng)
xs = -1.0 + (2.0 / (ngrid - 1)) * np.arange(ngrid)
xs[1:-1] += 1e-9 * np.sin(np.arange(1, ngrid - 1))            # off the uniform grid: the table route
gp = np.ascontiguousarray(R.legendre_encode(xs, d))
X = rng.uniform(-0.95, 0.95, (N, T))
phi = np.ascontiguousarray(R.legendre_encode(X, d))
m = np.zeros((N, T), dtype=np.uint8)
m[:, 8:24] = 1
y = np.zeros(N, dtype=np.int32)
eng = mt.SweepEngine(0)
def run(table):
    ts = []
    for it in range(9):
        x, e, s = eng.impute_model(W, phi, y, m, xs, table, 0, True)
        ts.append(s)
    info = eng.impute_info()
    return float(np.median(ts[2:])), float(np.min(ts[2:])), float(np.max(ts[2:])), info["closed_form_densities"], x
a = run(gp)
print(which, "shared   median %.3f ms (min %.3f max %.3f) closed_form=%s" % (1e3 * a[0], 1e3 * a[1], 1e3 * a[2], a[3]), flush=True)
if which == "new":
    b = run(np.ascontiguousarray(np.broadcast_to(gp, (T,) + gp.shape)))
    print(which, "per-site median %.3f ms (min %.3f max %.3f) closed_form=%s equal=%s" % (1e3 * b[0], 1e3 * b[1], 1e3 * b[2], b[3], np.array_equal(a[4], b[4])), flush=True)
eng.close()
