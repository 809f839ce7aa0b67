"""Records tests/golden/encode_host_path/parent.npz: the bits of the device-side encoders as the commit BEFORE the encoding host path
was consolidated (EncodeBasis / encode_tables, csrc/mpst_encode_plan.h) produced them.  tests/test_gpu_encode_parent_bits.py imports
this file, regenerates the same seeded inputs on the current build and compares byte for byte.

The fixture is tied to the ROCm build it was recorded on: exp() of the sigmoid, sincospi() and sqrt() come from that toolchain's device
library, so another ROCm release may change last bits on both sides alike.  To regenerate it, check out and build the parent commit and
run this file with that checkout as the working directory (the package is imported from there):

    cd <built checkout of the parent> && python <this file> --out <repository>/tests/golden/encode_host_path/parent.npz \
        --commit <hash> --toolchain "<hipcc --version, one line>"

The file holds the SHA-256 of every output's bytes (sha/<case>/<door>/<output>), the arrays themselves for one value-train case per kind
(arr/<case>) so that a mismatch can be located, and meta_commit / meta_toolchain.

Shapes: N = 70, T = 5 - 350 values: k_encode runs a second, partly filled block; N is no multiple of 64: a wave straddles two sites; 70 is
no multiple of the 4 series per block of k_enc_series_fix - and one closed-form case at N = 5, T = 70 for that kernel's lane loop."""
import argparse
import hashlib
import os
import sys

import numpy as np

N, T, NT = 70, 5, 41
ARRAYS = ("legendre_no_norm_d4", "split_shared_legendre", "kde_per_site_zero", "proj_legendre_norm")     # one per kind, kept whole
ALL = ("values_train", "values_test", "dataset", "dataset_cast")


def _data(seed, n, t):
    rng = np.random.default_rng(seed)
    Xtr = rng.normal(size=(n, t)) + np.linspace(0, 1, t)
    Xte = 1.6 * rng.normal(size=(NT, t)) + 0.3                         # wider than the training data: out-of-bounds rescales
    return Xtr, Xte


def _kde_tables(rng, per_site, d, K, zero_site=None):
    S = T if per_site else 1
    tab = dict(npoints=K, per_site=per_site, lo=rng.uniform(-1.0, -0.8, S), step=rng.uniform(1.7, 2.0, S) / (K - 1),
               coef=rng.uniform(0.05, 1.0, (S, K + 2)), minx=rng.uniform(0.01, 0.05, S), scale=rng.uniform(0.5, 2.0, S),
               cvecs=rng.normal(size=(S, d, d)))
    if zero_site is not None:
        tab["cvecs"][zero_site] = 0.0
    return tab


def cases(mt):
    """name -> (basis, d, extra keyword arguments of encode_values / encode_dataset, the encoding's range, doors)"""
    from mpstime_jl_amd import encodings as E
    rng = np.random.default_rng(2024)
    out = {}
    for name, basis, d, doors in (("legendre_no_norm_d4", "Legendre_No_Norm", 4, ALL), ("legendre_norm_d3", "Legendre_Norm", 3, ALL[:1]),
                                  ("fourier_d5", "Fourier", 5, ALL), ("stoudenmire_d2", "Stoudenmire", 2, ALL[:1]),
                                  ("sahand_d4", "Sahand", 4, ALL[:1]), ("uniform_d3", "Uniform", 3, ALL[:1])):
        out[name] = (basis, d, {}, E.model_encoding(basis).range, doors)
    out["legendre_no_norm_d4_T70"] = ("Legendre_No_Norm", 4, {}, (-1.0, 1.0), ALL[:2])
    # split: shared uniform edges over Legendre, 3 bins x 2; per-site edges over Fourier, 2 x 2, site 1 with an empty bin (two equal
    # edges) and, through the "raw" door, series 3 exactly on the interior edge of site 0
    out["split_shared_legendre"] = ("unif_split_legendre", 6, dict(bins=np.linspace(-1.0, 1.0, 4)), E.model_encoding("unif_split_legendre").range, ALL)
    edges = np.sort(rng.uniform(-0.6, 0.6, (T, 1)), axis=1)
    per_site = np.concatenate([np.full((T, 1), -1.0), edges, np.full((T, 1), 1.0)], axis=1)
    per_site[0, 1], per_site[1] = 0.25, (-1.0, 0.5, 0.5)
    out["split_per_site_fourier"] = ("hist_split_fourier", 4, dict(bins=per_site), E.model_encoding("hist_split_fourier").range, ("values_train", "raw"))
    sl, sl0 = mt.sahand_legendre(True), mt.sahand_legendre(False)
    out["kde_per_site_zero"] = (sl, 3, dict(kde=_kde_tables(rng, 1, 3, 9, zero_site=2)), sl.range, ALL)
    out["kde_shared"] = (sl0, 3, dict(kde=_kde_tables(rng, 0, 3, 3)), sl0.range, ALL[:1])
    orders = np.array([[5, 3, 1], [2, 7, 4], [0, 1, 2], [9, 8, 6], [3, 1, 2]], dtype=np.int32)                 # unsorted lists
    ln, lnn, fo = mt.legendre(norm=True, project=True), mt.legendre(norm=False, project=True), mt.fourier(project=True)
    out["proj_legendre_norm"] = (ln, 3, dict(orders=dict(basis="Legendre_Norm", orders=orders, inv_norm=rng.uniform(0.3, 1.2, T))), ln.range, ALL)
    rep = orders.copy()
    rep[1], rep[3] = (4, 4, 2), (6, 6, 6)                                                                      # repeated orders
    out["proj_legendre_no_norm"] = (lnn, 3, dict(orders=dict(basis="Legendre_No_Norm", orders=rep, inv_norm=None)), lnn.range, ALL[:1])
    freqs = np.array([[0, 1, -1], [2, -2, 0], [-3, 1, 1], [0, -1, 4], [5, -5, 2]], dtype=np.int32)
    out["proj_fourier"] = (fo, 3, dict(orders=dict(basis="Fourier", orders=freqs, inv_norm=None)), fo.range, ALL[:1])
    return out


def _norms(norms):
    return np.array(list(norms.sigmoid) + list(norms.minmax), dtype=np.float64)


def _oob(oob):
    return np.array(oob, dtype=np.float64).reshape(-1, 3)


def outputs(mt):
    """{"<case>/<door>/<output>": array} of every case through its doors, each door on a context of its own"""
    from mpstime_jl_amd import encodings as E
    res = {}
    for k, (name, (basis, d, extra, enc_range, doors)) in enumerate(cases(mt).items()):
        n, t = (5, 70) if name.endswith("_T70") else (N, T)
        Xtr, Xte = _data(100 + k, n, t)
        cx = (basis if isinstance(basis, E.Encoding) else E.model_encoding(basis)).iscomplex
        lab = lambda m: (np.arange(m) >= m // 2).astype(np.int32)
        common = dict(basis=basis, d=d, sigmoid_transform=True, minmax=True, enc_range=enc_range, **extra)

        def put(door, **arrays):
            for key, a in arrays.items():
                res[f"{name}/{door}/{key}"] = np.ascontiguousarray(a)

        # the value doors: the training fit (sigmoid fitted on the device, min-max), then the test set with its norms
        eng = mt.SweepEngine(0)
        try:
            phi, _ = eng.encode_values(Xtr, **common)
            put("values_train", phi=phi)
            if "values_test" in doors:
                fit = mt.SweepEngine(0)                                 # encode_values returns no norms: the data-set door's fit
                try:
                    norms, _ = fit.encode_dataset(0, Xtr, lab(n), 2, **common)
                finally:
                    fit.close()
                phi, _ = eng.encode_values(Xte, norms=norms, rescale_out_of_bounds=True, **common)
                put("values_test", phi=phi, norms=_norms(norms))
            if "raw" in doors:                                          # no transforms, identity range map: x itself reaches the basis
                Xr = np.random.default_rng(7).uniform(-1.0, 1.0, (n, t))
                Xr[3, 0] = 0.25
                phi, _ = eng.encode_values(Xr, basis, d=d, **extra)
                put("raw", phi=phi)
        finally:
            eng.close()
        for door, dtype in (("dataset", None), ("dataset_cast", np.complex64 if cx else np.float32)):
            if door not in doors:
                continue
            eng = mt.SweepEngine(0)
            try:
                if dtype is not None:
                    eng.set_dtype(dtype)
                norms, _ = eng.encode_dataset(0, Xtr, lab(n), 2, **common)
                tr = eng.get_encoded(0)
                oob, _ = eng.encode_dataset(1, Xte, lab(NT), 2, norms=norms, **common)
                te = eng.get_encoded(1)
                assert tr.dtype == (dtype or (np.complex128 if cx else np.float64))
                put(door, train=tr, test=te, norms=_norms(norms), oob=_oob(oob))
            finally:
                eng.close()
    return res


def digest(a):
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--toolchain", default="unknown")
    a = ap.parse_args()
    sys.path.insert(0, os.getcwd())
    import mpstime_jl_amd as mt
    res = outputs(mt)
    doc = {"meta_commit": np.array(a.commit), "meta_toolchain": np.array(a.toolchain)}
    for key, arr in res.items():
        doc["sha/" + key] = np.array(digest(arr))
        if key.split("/")[0] in ARRAYS and key.endswith("values_train/phi"):
            doc["arr/" + key.split("/")[0]] = arr
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **doc)
    print(f"{len(res)} outputs of {len(cases(mt))} cases -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
