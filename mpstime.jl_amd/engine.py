"""SweepEngine: thin Python mirror of the C ABI (one context = one GPU).

Arrays cross the boundary in the layouts of include/mpstime_hip.h.  On the
Python side a site tensor is an ndarray (Dl, d, Dr) or (Dl, d, Dr, C) - the
boundary layout is its Fortran-order (d, Dl, Dr[, C]) permutation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _site_to_abi(t, dtype=np.float64):
    t = np.asarray(t, dtype=dtype)
    if t.ndim == 3:
        a = np.transpose(t, (1, 0, 2))          # (d, Dl, Dr)
    else:
        a = np.transpose(t, (1, 0, 2, 3))       # (d, Dl, Dr, C)
    return np.asfortranarray(a)


def label_site_of(W, error=AssertionError):
    """index of the one site tensor (Dl, d, Dr, C) that carries the label index"""
    ls = [j for j, t in enumerate(W) if np.ndim(t) == 4]
    if len(ls) != 1:
        raise error("exactly one site must carry the label index")
    return ls[0]


def model_to_abi(W, phi, compute="f64", label_site=None):
    """(mpst_impute_model, the arrays it points into) of site tensors ``W`` (Dl, d, Dr), the label site (Dl, d, Dr, C), and encoded
    values ``phi`` (N, T, d), or None for a model without data (N = 0); complex if any of them is.  label_idx is NULL: the callers
    that have labels set it."""
    cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi)
    dt = np.complex128 if cx else np.float64
    T = len(W)
    if label_site is None:
        label_site = label_site_of(W)
    Cn, d = int(W[label_site].shape[3]), int(W[0].shape[1])
    chi = np.array([W[0].shape[0]] + [t.shape[2] for t in W], dtype=np.int32)
    bufs = [_site_to_abi(t, dt) for t in W]
    ptrs = (C.c_void_p * T)(*[b.ctypes.data for b in bufs])
    ph = None if phi is None else np.ascontiguousarray(phi, dtype=dt)
    N = 0 if ph is None else ph.shape[0]
    assert ph is None or ph.shape == (N, T, d)
    model = L.ImputeModel(N, T, d, Cn, int(label_site), 1 if cx else 0, {"f64": 0, "f32": 1}[compute],
                          C.cast(ptrs, C.POINTER(C.c_void_p)), chi.ctypes.data_as(C.POINTER(C.c_int32)),
                          None if ph is None else ph.ctypes.data_as(C.c_void_p), None)
    return model, (bufs, ptrs, chi, ph)


def _site_from_abi(buf, Dl, d, Dr, Cj):
    shape = (d, Dl, Dr) + ((Cj,) if Cj else ())
    a = np.reshape(buf, shape, order="F")
    return np.ascontiguousarray(np.transpose(a, (1, 0, 2) + ((3,) if Cj else ())))


DTYPES = {np.dtype(np.float64): L.F64, np.dtype(np.float32): L.F32, np.dtype(np.complex128): L.C128, np.dtype(np.complex64): L.C64}


MAX_LEVELS = 16      # levels per mpst_impute_dist call (include/mpstime_hip.h)


def check_levels(levels):
    """``levels`` of an imputation call as a float64 array, or None: at most MAX_LEVELS numbers strictly inside (0, 1), in any order.
    Raises ValueError otherwise - on the host, before any device call."""
    if levels is None:
        return None
    lv = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.float64)
    if lv.ndim != 1 or lv.size == 0:
        raise ValueError("levels must be a non-empty sequence of numbers")
    if lv.size > MAX_LEVELS:
        raise ValueError(f"at most {MAX_LEVELS} levels per call (got {lv.size})")
    if not np.all((lv > 0.0) & (lv < 1.0)):
        raise ValueError(f"levels must lie strictly inside (0, 1) (got {lv.tolist()})")
    return lv


def cdf_points(ngrid, stride):
    """grid indices a cdf of stride ``stride`` is stored at: 0, s, 2s, ... and always ngrid - 1."""
    return (int(ngrid) - 2) // int(stride) + 2


def cdf_indices(ngrid, stride):
    n = cdf_points(ngrid, stride)
    k = np.arange(n) * int(stride)
    k[-1] = int(ngrid) - 1
    return k


def _dtype_of(x):
    """Element type of an array-like as the engine sees it (opts.dtype): float64 unless it already is one of the four."""
    dt = np.asarray(x).dtype
    return dt if dt in DTYPES else np.dtype(np.float64)


def _encode_opts(basis, sigmoid_transform, minmax, data_bounds, enc_range, norms, rescale_out_of_bounds):
    """mpst_encode_opts of a training set (``norms`` None: nothing fitted yet, fit_sigmoid left to the caller) or of a test set with
    the training fit's ``norms``."""
    eo = L.mpst_encode_opts()
    eo.basis, eo.sigmoid_transform, eo.minmax = L.BASIS[basis], int(bool(sigmoid_transform)), int(bool(minmax))
    eo.is_test, eo.rescale_out_of_bounds = int(norms is not None), int(bool(rescale_out_of_bounds))
    eo.data_lb, eo.data_ub = map(float, data_bounds)
    eo.range_a, eo.range_b = map(float, enc_range)
    if norms is not None:
        if norms.sigmoid is not None:
            eo.median, eo.iqr = norms.sigmoid
        eo.sigmoid_transform = int(norms.sigmoid is not None)
        if norms.minmax is not None:
            eo.lo, eo.hi = norms.minmax
    return eo


def _split_opts(aux_basis, d, T, bins):
    """mpst_split_opts of a split encoding over ``aux_basis`` with the fitted edges ``bins`` - (nbins + 1,) shared by all sites or
    (T, nbins + 1) - and the array the struct points into (keep it alive over the call)."""
    if bins is None:
        raise ValueError("a split encoding is encoded with the bin edges its fit produced: pass bins (fit_encoding(...)[1].bins)")
    b = np.ascontiguousarray(bins, dtype=np.float64)
    if b.ndim not in (1, 2) or b.shape[-1] < 2 or (b.ndim == 2 and b.shape[0] != T):
        raise ValueError(f"bins must be (nbins + 1,) or ({T}, nbins + 1), got {b.shape}")
    nbins = b.shape[-1] - 1
    sp = L.mpst_split_opts(L.BASIS[aux_basis], int(d) // nbins, nbins, int(b.ndim == 2), b.ctypes.data_as(C.POINTER(C.c_double)))
    return sp, b


def _kde_opts(kde, d, T):
    """mpst_kde_opts of a fitted Sahand-Legendre encoding - ``kde`` is its FittedEncoder (``fit_encoding(...)[1]``) or that encoder's
    ``kde`` tables - and the arrays the struct points into (keep them alive over the call).  The shapes are checked here: the
    library reads (S, K + 2) and (S, d, d) doubles behind the pointers, S = T or 1."""
    tab = getattr(kde, "kde", kde)
    if not isinstance(tab, dict):
        raise ValueError("a Sahand-Legendre encoding is encoded with the tables its fit produced: pass kde (fit_encoding(...)[1])")
    K, per_site = int(tab["npoints"]), int(tab["per_site"])
    S = T if per_site else 1
    shapes = dict(lo=(S,), step=(S,), coef=(S, K + 2), minx=(S,), scale=(S,), cvecs=(S, int(d), int(d)))
    arr = {k: np.ascontiguousarray(tab[k], dtype=np.float64) for k in shapes}
    for k, shp in shapes.items():
        if arr[k].shape != shp:
            raise ValueError(f"kde table {k!r} must have shape {shp}, got {arr[k].shape}")
    kd = L.mpst_kde_opts(K, per_site, *[arr[k].ctypes.data_as(C.POINTER(C.c_double)) for k in shapes])
    return kd, arr


def _proj_opts(orders, d, T):
    """mpst_proj_opts of a fitted projected encoding - ``orders`` is its FittedEncoder (``fit_encoding(...)[1]``) or that encoder's
    ``orders`` tables - and the arrays the struct points into (keep them alive over the call).  The shapes are checked here: the
    library reads (T, d) integers and (T,) doubles behind the pointers; it checks their values."""
    tab = getattr(orders, "orders", orders)
    if not isinstance(tab, dict):
        raise ValueError("a projected encoding is encoded with the orders its fit selected: pass orders (fit_encoding(...)[1])")
    o = np.ascontiguousarray(tab["orders"], dtype=np.int32)
    if o.shape != (T, int(d)):
        raise ValueError(f"orders table 'orders' must have shape {(T, int(d))}, got {o.shape}")
    inv = None
    if tab.get("inv_norm") is not None:
        inv = np.ascontiguousarray(tab["inv_norm"], dtype=np.float64)
        if inv.shape != (T,):
            raise ValueError(f"orders table 'inv_norm' must have shape {(T,)}, got {inv.shape}")
    max_order = int(np.abs(o.astype(np.int64)).max())
    pj = L.mpst_proj_opts(L.BASIS[tab["basis"]], o.ctypes.data_as(C.POINTER(C.c_int32)),
                          inv.ctypes.data_as(C.POINTER(C.c_double)) if inv is not None else None, max_order)
    return pj, (o, inv)


COMPLEX_BASES = ("Fourier", "Stoudenmire", "Sahand")     # the closed-form bases whose states are complex


def _basis_request(basis, d, T, bins=None, kde=None, orders=None):
    """What encode_dataset / encode_values were handed - a name or an Encoding and, for a fitted encoding, its tables - as the library
    takes it: (canonical name of the closed-form basis the kernel evaluates - the auxiliary basis of a split encoding, the family of a
    projected one; a Sahand-Legendre call ignores it -, its input range, whether the states are complex, the infix of the entry points
    mpst_encode_<infix>dataset / mpst_encode_<infix>values, (the options struct they take after eo or None, the arrays it points into:
    keep them alive over the call)).  Raises MPSTError(UNSUPPORTED) for what the device does not encode."""
    from .encodings import Encoding, model_encoding
    if kde is not None and orders is not None:
        raise ValueError("kde= and orders= belong to different encodings: pass one of them")
    rng = (-1.0, 1.0)
    if kde is not None or orders is not None:
        rng = tuple(basis.range) if isinstance(basis, Encoding) and basis.range else rng
        if kde is not None:
            return "Legendre_No_Norm", rng, False, "kde_", _kde_opts(kde, d, T)
        tab = getattr(orders, "orders", orders)
        if not isinstance(tab, dict) or tab.get("basis") not in ("Legendre_Norm", "Legendre_No_Norm", "Fourier"):
            raise ValueError("a projected encoding is encoded with the orders its fit selected: pass orders (fit_encoding(...)[1])")
        return tab["basis"], rng, tab["basis"] in COMPLEX_BASES, "proj_", _proj_opts(orders, d, T)
    split = False
    try:
        enc = basis if isinstance(basis, Encoding) else model_encoding(basis)
        split = enc.aux_enc is not None
        # canonical name; :Legendre is :Legendre_No_Norm (options.jl:245-246)
        basis, rng = (enc.aux_enc.name if split else enc.name), (enc.range or rng)
    except Exception:
        pass
    if basis not in L.BASIS:
        raise L.MPSTError(L.MPST_ERR_UNSUPPORTED, f"device-side encoding implements the closed-form bases {sorted(L.BASIS)}, split bases over them and - "
                                                  f"with kde= / orders=, their fitted encoder - the Sahand-Legendre and the projected bases, not {basis!r}")
    return basis, rng, basis in COMPLEX_BASES, "split_" if split else "", _split_opts(basis, d, T, bins) if split else (None, None)


class SweepEngine:
    def __init__(self, device: int = 0):
        self.lib = L.load()
        self.ctx = C.c_void_p()
        rc = self.lib.mpst_create(C.byref(self.ctx), device)
        if rc:
            raise L.MPSTError(rc, (self.lib.mpst_last_error(None) or b"").decode())
        self.T = self.d = self.C = 0
        self.N = [0, 0]
        self.dtype = np.dtype(np.float64)      # element type of the data sets and the MPS (mpst_set_dataset's dtype)

    # -- plumbing ---------------------------------------------------------------------
    def _chk(self, rc):
        if rc:
            msg = (self.lib.mpst_last_error(self.ctx) or b"").decode()
            raise (L.SVDError if rc == L.MPST_ERR_SVD else L.MPSTError)(rc, msg)

    def close(self):
        if getattr(self, "ctx", None) and self.ctx.value:
            self.lib.mpst_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ----------------------------------------------------------------
    def set_options(self, chi_max, eta=0.01, cutoff=1e-10, update_iters=1, loss="KLD", bbopt="TSGO",
                    rescale=(False, True), train_classes_separately=False, svd_alg=0, rebuild_caches=False, track_cost=False):
        if str(loss).upper() not in L.LOSS:
            raise L.MPSTError(L.MPST_ERR_UNSUPPORTED, f"loss {loss!r} unsupported by the array sweep")
        if str(bbopt).upper() not in L.OPT:
            raise L.MPSTError(L.MPST_ERR_UNSUPPORTED,
                              "Optim/OptimKit based solvers currently unimplemented for this version, "
                              "set 'use_legacy_ITensor=true' in MPSOptions to enable")
        o = L.mpst_options(int(chi_max), int(update_iters), L.LOSS[str(loss).upper()], L.OPT[str(bbopt).upper()],
                           int(bool(rescale[0])), int(bool(rescale[1])), int(bool(train_classes_separately)),
                           int(svd_alg), int(bool(rebuild_caches)), int(bool(track_cost)), float(eta), float(cutoff))
        self._iters = int(update_iters)
        self._chk(self.lib.mpst_set_options(self.ctx, C.byref(o)))

    def set_batch_hint(self, K):
        """This fit will be advanced in batches of about K (``sweep_batch``): fewer, longer gradient shares (mpst_set_batch_hint)."""
        self._chk(self.lib.mpst_set_batch_hint(self.ctx, int(K)))

    def set_dtype(self, dtype):
        """opts.dtype for data sets that are encoded on the device (mpst_set_dtype); set_dataset takes it from its array."""
        dt = np.dtype(dtype)
        self._chk(self.lib.mpst_set_dtype(self.ctx, DTYPES[dt]))
        self.dtype = dt
        self._dtype_fixed = True

    def set_dataset(self, which, phi, label_index, C_classes, global_counts=None, dtype=None):
        """``dtype``: element type the engine trains in (float64 / float32 / complex128 / complex64 = opts.dtype); default
        the array's own type."""
        dt = np.dtype(dtype) if dtype is not None else _dtype_of(phi)
        phi = np.ascontiguousarray(phi, dtype=dt)
        lab = np.ascontiguousarray(label_index, dtype=np.int32)
        N, T, d = phi.shape if phi.ndim == 3 and phi.size else (0, self.T, self.d)
        gc = None
        if global_counts is not None:
            gc = np.ascontiguousarray(global_counts, dtype=np.int64)
        self._chk(self.lib.mpst_set_dataset(
            self.ctx, which, phi.ctypes.data_as(C.c_void_p), lab.ctypes.data_as(C.POINTER(C.c_int32)), N, T, d,
            int(C_classes), DTYPES[dt], gc.ctypes.data_as(C.POINTER(C.c_int64)) if gc is not None else None))
        self.T, self.d, self.C = T, d, int(C_classes)
        self.N[which] = N
        self.dtype = dt

    def encode_dataset(self, which, X_sorted, label_index, C_classes, basis="Legendre_No_Norm", d=None, sigmoid_transform=True,
                       minmax=True, data_bounds=(0.0, 1.0), enc_range=(-1.0, 1.0), norms=None, rescale_out_of_bounds=True,
                       global_counts=None, sigmoid_fit=None, bins=None, kde=None, orders=None):
        """Preprocess + encode the raw (N, T) matrix on the device (mpst_encode_dataset).  ``X_sorted`` must already be
        sorted by class.  ``norms=None`` fits a training set (median/IQR on the host, min/max on the device) and
        returns ``(norms, seconds)``; with ``norms`` from the training fit the data is treated as a test set and
        ``(oob, seconds)`` comes back, ``oob`` in the format of transform_test_data (utils.jl:243-266).
        A split encoding (name or Encoding) goes through mpst_encode_split_dataset with ``bins``, the edges its fit produced
        (``fit_encoding(...)[1].bins``: (nbins + 1,) or (T, nbins + 1)); a Sahand-Legendre encoding through mpst_encode_kde_dataset
        with ``kde``, its fitted encoder (``fit_encoding(...)[1]``); a projected encoding through mpst_encode_proj_dataset with
        ``orders``, its fitted encoder or that encoder's ``orders`` tables."""
        from .encodings import Norms
        X = np.ascontiguousarray(X_sorted, dtype=np.float64)
        lab = np.ascontiguousarray(label_index, dtype=np.int32)
        N, T = X.shape
        d = int(d if d is not None else self.d)
        basis, _, cx, infix, (bopts, _keep) = _basis_request(basis, d, T, bins, kde, orders)
        eo = _encode_opts(basis, sigmoid_transform, minmax, data_bounds, enc_range, norms, rescale_out_of_bounds)
        if norms is None and sigmoid_transform:
            if sigmoid_fit is not None:                 # (median, iqr) fitted elsewhere, e.g. over all shards
                eo.median, eo.iqr = map(float, sigmoid_fit)
            else:
                eo.fit_sigmoid = 1                      # median / quartiles from a device sort of the values
        gc = np.ascontiguousarray(global_counts, dtype=np.int64) if global_counts is not None else None
        fix = np.zeros((N, 2)) if norms is not None else None
        sec = C.c_double()
        dp = C.POINTER(C.c_double)
        head = (self.ctx, which, X.ctypes.data_as(dp), lab.ctypes.data_as(C.POINTER(C.c_int32)), N, T, d, int(C_classes), C.byref(eo))
        tail = (gc.ctypes.data_as(C.POINTER(C.c_int64)) if gc is not None else None, fix.ctypes.data_as(dp) if fix is not None else None,
                C.byref(sec))
        own = () if bopts is None else (C.byref(bopts),)
        self._chk(getattr(self.lib, f"mpst_encode_{infix}dataset")(*head, *own, *tail))
        self.T, self.d, self.C = T, d, int(C_classes)
        self.N[which] = N
        self.dtype = self._ctx_dtype(cx)
        if norms is None:
            out = Norms(sigmoid=(eo.median, eo.iqr) if sigmoid_transform else None, minmax=(eo.lo, eo.hi) if minmax else None)
            return out, sec.value
        oob = [[i, float(fix[i, 0]), float(fix[i, 1])] for i in range(N) if fix[i, 0] != 0.0 or fix[i, 1] != 1.0]
        return oob, sec.value

    def encode_values(self, X, basis="Legendre_No_Norm", d=4, sigmoid_transform=False, minmax=False, data_bounds=(0.0, 1.0),
                      enc_range=None, norms=None, rescale_out_of_bounds=False, bins=None, kde=None, orders=None):
        """mpst_encode_values: the device preprocessing + encoding kernels on a raw (N, T) matrix, states back to the host -
        (N, T, d) float64 for the Legendre / Uniform bases, complex128 for "Fourier", "Stoudenmire", "Sahand".  Defaults: X is already in the encoding's
        domain (no transforms, identity range map); with transforms the [0, 1] data is mapped onto ``enc_range``
        (default: the basis' own range, (-1, 1) for Legendre / Fourier, (0, 1) for Stoudenmire / Sahand / Uniform).  ``norms`` as for encode_dataset (a test set) or None.
        A split encoding with its fitted ``bins`` goes through mpst_encode_split_values, a Sahand-Legendre encoding with its fitted
        encoder ``kde`` through mpst_encode_kde_values, a projected encoding with its fitted encoder ``orders`` through
        mpst_encode_proj_values (complex128 for projected Fourier), as in encode_dataset."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        N, T = X.shape
        basis, basis_range, cx, infix, (bopts, _keep) = _basis_request(basis, int(d), T, bins, kde, orders)
        if enc_range is None:
            enc_range = basis_range if (sigmoid_transform or minmax or norms is not None) else (0.0, 1.0)
        eo = _encode_opts(basis, sigmoid_transform, minmax, data_bounds, enc_range, norms, rescale_out_of_bounds)
        if norms is None:
            eo.fit_sigmoid = int(bool(sigmoid_transform))
        out = np.zeros((N, T, int(d)), dtype=np.complex128 if cx else np.float64)
        sec = C.c_double()
        own = () if bopts is None else (C.byref(bopts),)
        self._chk(getattr(self.lib, f"mpst_encode_{infix}values")(self.ctx, X.ctypes.data_as(C.POINTER(C.c_double)), N, T, int(d), C.byref(eo), *own,
                                                                 out.ctypes.data_as(C.c_void_p), None, C.byref(sec)))
        return out, sec.value

    def _ctx_dtype(self, cx):
        """element type after a device-side encoding: what set_dtype fixed, else the basis' own (float64 / complex128)"""
        if getattr(self, "_dtype_fixed", False):
            return self.dtype
        return np.dtype(np.complex128 if cx else np.float64)

    def get_encoded(self, which=0):
        phi = np.zeros((self.N[which], self.T, self.d), dtype=self.dtype)
        self._chk(self.lib.mpst_get_encoded(self.ctx, which, phi.ctypes.data_as(C.POINTER(C.c_double))))
        return phi

    def set_mps(self, W, label_site=None):
        T = len(W)
        if label_site is None:
            label_site = label_site_of(W)
        chi = np.array([W[0].shape[0]] + [t.shape[2] for t in W], dtype=np.int32)
        bufs = [_site_to_abi(t, self.dtype) for t in W]       # in the context's element type
        ptrs = (C.c_void_p * T)(*[b.ctypes.data for b in bufs])
        self._chk(self.lib.mpst_set_mps(self.ctx, ptrs, chi.ctypes.data_as(C.POINTER(C.c_int32)), T, int(label_site)))

    def get_chi(self):
        chi = np.zeros(self.T + 1, dtype=np.int32)
        ls = C.c_int32()
        self._chk(self.lib.mpst_get_chi(self.ctx, chi.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ls)))
        return chi, ls.value

    def get_mps(self):
        chi, ls = self.get_chi()
        bufs = []
        for j in range(self.T):
            n = self.d * chi[j] * chi[j + 1] * (self.C if j == ls else 1)
            bufs.append(np.zeros(int(n), dtype=self.dtype))
        ptrs = (C.c_void_p * self.T)(*[b.ctypes.data for b in bufs])
        self._chk(self.lib.mpst_get_mps(self.ctx, ptrs))
        return [_site_from_abi(bufs[j], int(chi[j]), self.d, int(chi[j + 1]), self.C if j == ls else 0)
                for j in range(self.T)]

    # -- the path ---------------------------------------------------------------------
    def build_caches(self):
        self._chk(self.lib.mpst_build_caches(self.ctx))

    def sweep(self):
        st = L.mpst_sweep_stats()
        self._chk(self.lib.mpst_sweep(self.ctx, C.byref(st)))
        return {"seconds": st.seconds, "max_chi": st.max_chi, "eig_sweeps_total": st.eig_sweeps_total,
                "eig_fallbacks": st.eig_fallbacks}

    def loss_trace(self):
        """(2(T-1), update_iters + 1): losses before every optimiser step and at the updated bond tensor (track_cost)."""
        out = np.zeros((2 * (self.T - 1), self._iters + 1))
        self._chk(self.lib.mpst_get_loss_trace(self.ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def bond_step(self, lid, going_left):
        dbg = L.mpst_bond_debug()
        self._chk(self.lib.mpst_bond_step(self.ctx, int(lid), int(bool(going_left)), C.byref(dbg)))
        return {"loss": dbg.loss, "grad_norm": dbg.grad_norm, "bt_new_norm": dbg.bt_norm, "chi": dbg.chi_new,
                "eig_sweeps": dbg.eig_sweeps, "S": np.array(dbg.spectrum[:dbg.n_spectrum])}

    def eval(self, which=0):
        mse, kld, acc = C.c_double(), C.c_double(), C.c_double()
        conf = np.zeros((self.C, self.C), dtype=np.int64)
        self._chk(self.lib.mpst_eval(self.ctx, which, C.byref(mse), C.byref(kld), C.byref(acc),
                                     conf.ctypes.data_as(C.POINTER(C.c_int64))))
        return mse.value, kld.value, acc.value, conf

    def classify(self, which=1, return_overlaps=False):
        N = self.N[which]
        pred = np.zeros(N, dtype=np.int32)
        yh = np.zeros((N, self.C), dtype=np.complex128 if self.dtype.kind == "c" else np.float64)     # overlaps are fp64 (pairs)
        self._chk(self.lib.mpst_classify(self.ctx, which, pred.ctypes.data_as(C.POINTER(C.c_int32)),
                                         yh.ctypes.data_as(C.POINTER(C.c_double))))
        return (pred, yh) if return_overlaps else pred

    @staticmethod
    def _traj_args(N, T, method, max_trials, u, num_trajectories, seed, row_id):
        """(K, u, seed, row_id array or None) of a call with ``num_trajectories``: u (N, K, T[, max_trials]) or, with u None, the
        device generator under ``seed`` with the caller's ``row_id`` (N,)."""
        K = int(num_trajectories)
        if K < 1:
            raise ValueError("num_trajectories must be at least 1")
        if int(method) not in (2, 4):
            raise ValueError("num_trajectories needs a sampling method (2 quantile, 4 inverse-transform sampling with rejection)")
        uu = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        if uu is not None:
            assert uu.size == N * K * T * (int(max_trials) if int(method) == 4 else 1)
        elif seed is None:
            raise ValueError("num_trajectories needs the uniform numbers u or a seed for the device generator")
        rid = None if row_id is None else np.ascontiguousarray(row_id, dtype=np.int64)
        if rid is not None:
            assert rid.shape == (N,)
        sd = int(seed or 0) & (2 ** 64 - 1)
        return K, uu, sd - 2 ** 64 if sd >= 2 ** 63 else sd, rid

    @staticmethod
    def _dist_args(missing, ngrid, method, levels, cdf_stride, num_trajectories):
        """(levels array or None, q (N, T, nq) or None, cdf_stride, cdf_rows, cdf (N, cdf_rows, ncdf) or None) of a call with
        ``levels`` / ``cdf_stride`` (mpst_impute_dist); raises ValueError on what the library would refuse."""
        lv = check_levels(levels)
        s = int(cdf_stride)
        if s < 0:
            raise ValueError("cdf_stride must not be negative")
        if int(method) != 0:
            raise ValueError("levels / cdf_stride are read off the median imputer's distribution: method must be 0 (median)")
        if num_trajectories is not None:
            raise ValueError("levels / cdf_stride cannot be combined with num_trajectories")
        N, T = missing.shape
        q = np.zeros((N, T, len(lv))) if lv is not None else None
        rows = int(missing.astype(bool).sum(axis=1).max()) if (s > 0 and N > 0) else 0
        cdf = np.zeros((N, rows, cdf_points(ngrid, s))) if s > 0 else None
        return lv, q, s, rows, cdf

    def _impute(self, entries, head, arrays, a, dist=None):
        """The call behind ``impute`` and ``impute_model``, which differ only in how the model is supplied: ``entries`` names their
        (plain, *_traj, *_dist) entry points, ``head`` holds the arguments between the context and the mask; ``arrays`` = (mask (N, T) uint8,
        grid values, grid states), contiguous; ``a``: their other arguments by name; ``dist``: ``_dist_args``' result where the caller ran it."""
        m, gx, gp = arrays
        N, T = m.shape
        dp = C.POINTER(C.c_double)
        ptr = lambda v, t=dp: None if v is None else v.ctypes.data_as(t)
        shape, mid, tail, more = (N, T), (), (), ()
        if a["levels"] is not None or a["cdf_stride"]:
            name = entries[2]
            lv, q, s, rows, cdf = dist or self._dist_args(m, len(gx), a["method"], a["levels"], a["cdf_stride"], a["num_trajectories"])
            tail, more = (0 if lv is None else len(lv), ptr(lv), ptr(q), s, rows, ptr(cdf)), (q, cdf)
        elif a["num_trajectories"] is not None:
            name = entries[1]
            K, uu, sd, rid = self._traj_args(N, T, a["method"], a["max_trials"], a["u"], a["num_trajectories"], a["seed"], a["row_id"])
            shape, mid = (N, K, T), (K, ptr(uu), sd, ptr(rid, C.POINTER(C.c_int64)))
        else:
            name = entries[0]
            uu = None if a["u"] is None else np.ascontiguousarray(a["u"], dtype=np.float64)
            if uu is not None:
                assert uu.size == N * T * (int(a["max_trials"]) if int(a["method"]) == 4 else 1)
            mid = (ptr(uu),)
        o = L.ImputeOpts(int(a["method"]), int(a["order"]), int(bool(a["get_wmad"])), int(a["max_trials"]), int(a["mean_basis"]),
                         int(gp.ndim == 3), float(a["rejection_threshold"]))          # a (T, ngrid, d) table: one per site
        x, err, sec = np.zeros(shape), np.zeros(shape), C.c_double()
        self._chk(getattr(self.lib, name)(self.ctx, *head, ptr(m, C.POINTER(C.c_uint8)), ptr(gx), C.cast(gp.ctypes.data, dp), len(gx),
                                          C.byref(o), *mid, ptr(x), ptr(err), C.byref(sec), *tail))
        return (x, err, sec.value) + more

    def impute(self, which, missing, grid_x, grid_phi, method=0, get_wmad=True, u=None, order=0, max_trials=1,
               rejection_threshold=0.0, mean_basis=1, num_trajectories=None, seed=None, row_id=None, levels=None, cdf_stride=0):
        """mpst_impute: (x, err, seconds); x / err are (N, T) with the imputed value / its uncertainty at every missing
        site.  method 0 median, 1 mode, 2 quantile of u (N, T), 3 mean, 4 inverse-transform sampling with rejection
        (u (N, T, max_trials)); order 0 forwards, 1 backwards.  With ``num_trajectories`` = K (mpst_impute_traj, sampling methods
        only) x / err are (N, K, T): K chains per instance from one conditioning, u (N, K, T[, max_trials]) or u None and the
        device generator keyed by ``seed`` and the caller's ``row_id`` (N,) (default: the index in the data set).
        With ``levels`` (up to 16 numbers inside (0, 1)) and / or ``cdf_stride`` >= 1 (mpst_impute_dist, median only) the return value is
        (x, err, seconds, q, cdf): q (N, T, nq) the grid value at every level of every missing site's conditional cdf (0 at known
        sites) or None, cdf (N, cdf_rows, ncdf) that cdf at the grid indices 0, s, 2s, ... and ngrid - 1, row r = the r-th missing
        site of the instance in ascending order, cdf_rows = the largest missing count, or None.
        ``grid_phi`` (ngrid, d) is one table for all sites; (T, ngrid, d) holds one per site (time-dependent encodings; grid_per_site
        of mpst_impute_opts): the densities are then read from the table, one instance per workgroup; method 3 (mean) is refused."""
        m = np.ascontiguousarray(missing, dtype=np.uint8)
        gx = np.ascontiguousarray(grid_x, dtype=np.float64)
        gp = np.ascontiguousarray(grid_phi, dtype=np.complex128 if self.dtype.kind == "c" else np.float64)   # grid states: fp64 (pairs)
        assert gp.shape in ((len(gx), self.d), (self.T, len(gx), self.d)) and m.shape == (self.N[which], self.T)
        args = dict(method=method, order=order, get_wmad=get_wmad, max_trials=max_trials, mean_basis=mean_basis,
                    rejection_threshold=rejection_threshold, u=u, num_trajectories=num_trajectories, seed=seed, row_id=row_id, levels=levels,
                    cdf_stride=cdf_stride)
        return self._impute(("mpst_impute", "mpst_impute_traj", "mpst_impute_dist"), (which,), (m, gx, gp), args)

    def impute_model(self, W, phi, label_index, missing, grid_x, grid_phi, method=0, get_wmad=True, u=None, order=0, max_trials=1,
                     rejection_threshold=0.0, mean_basis=None, compute="f64", label_site=None, num_trajectories=None, seed=None,
                     row_id=None, levels=None, cdf_stride=0):
        """mpst_impute_model_run: the imputation engine on a model handed over in one call.  ``W``: site tensors
        (Dl, d, Dr), the label site (Dl, d, Dr, C); ``phi`` (N, T, d) encoded known values; real or complex (then
        ``grid_phi`` is complex too).  ``compute`` "f64" or "f32" (fp32 chain contractions, fp64 densities).
        Returns (x, err, seconds); with ``num_trajectories`` = K (mpst_impute_model_traj) x / err are (N, K, T), see ``impute``;
        with ``levels`` / ``cdf_stride`` (mpst_impute_model_dist) (x, err, seconds, q, cdf), see ``impute``."""
        m = np.ascontiguousarray(missing, dtype=np.uint8)
        # (levels / cdf_stride are checked before the model's shapes)
        dist = self._dist_args(m, len(grid_x), method, levels, cdf_stride, num_trajectories) if levels is not None or cdf_stride else None
        cx = any(np.iscomplexobj(t) for t in W) or np.iscomplexobj(phi) or np.iscomplexobj(grid_phi)
        dt = np.complex128 if cx else np.float64
        model, keep = model_to_abi(W, np.asarray(phi, dtype=dt), compute, label_site)
        N, T, d = int(model.N), int(model.T), int(model.d)
        lab = np.ascontiguousarray(label_index, dtype=np.int32)
        assert m.shape == (N, T) and lab.shape == (N,)
        model.label_idx = lab.ctypes.data_as(C.POINTER(C.c_int32))
        gx = np.ascontiguousarray(grid_x, dtype=np.float64)
        gp = np.ascontiguousarray(grid_phi, dtype=dt)
        assert gp.shape in ((len(gx), d), (T, len(gx), d))
        if u is not None and num_trajectories is None:         # (also where levels / cdf_stride leave u unused)
            assert np.size(u) == N * T * (int(max_trials) if int(method) == 4 else 1)
        if mean_basis is None:
            mean_basis = 2 if cx else 1
        args = dict(method=method, order=order, get_wmad=get_wmad, max_trials=max_trials, mean_basis=mean_basis,
                    rejection_threshold=rejection_threshold, u=u, num_trajectories=num_trajectories, seed=seed, row_id=row_id, levels=levels,
                    cdf_stride=cdf_stride)
        return self._impute(("mpst_impute_model_run", "mpst_impute_model_traj", "mpst_impute_model_dist"), (C.byref(model),), (m, gx, gp),
                            args, dist)

    def marginal_model(self, W, phi, missing, compute="f64", label_site=None):
        """mpst_marginal_model: (logp (N, C), seconds), the log likelihood of the known values of every instance under every class
        with the sites where ``missing`` (N, T; None: none) is set marginalised; see ``marginal.marginal_model``."""
        from .marginal import marginal_model
        return marginal_model(self, W, phi, missing, compute=compute, label_site=label_site)

    def prefix_model(self, W, phi, compute="f64", label_site=None):
        """mpst_prefix_marginals: (logp (N, T + 1, C), seconds), the log likelihood of the first t values of every instance under
        every class with the sites from t on marginalised, t = 0 .. T; see ``prefix.prefix_model``."""
        from .prefix import prefix_model
        return prefix_model(self, W, phi, compute=compute, label_site=label_site)

    def segment_model(self, W, phi, max_width, label_site=None):
        """mpst_segment_marginals: (logp (N, T, max_width, C), lnorm (C,), seconds), the log likelihood of the values of the sites
        a .. a+w-1 alone under every class, every other site marginalised, for every start a and width w <= max_width; see
        ``segments.segment_model``."""
        from .segments import segment_model
        return segment_model(self, W, phi, max_width, label_site=label_site)

    def rolling_model(self, W, phi, label_index, max_horizon, x, grid_x, grid_phi, levels=None, get_wmad=True, label_site=None):
        """mpst_rolling_forecasts: (nll, pit, median, err, mean, q, seconds), (N, T, max_horizon) arrays with entry [i, t, h - 1] for the
        predictive distribution of site t + h - 1 given the first t values; ``label_index`` -1 asks for the class mixture; see
        ``rolling.rolling_forecasts_model``."""
        from .rolling import rolling_forecasts_model
        return rolling_forecasts_model(self, W, phi, label_index, max_horizon, x, grid_x, grid_phi, levels=levels, get_wmad=get_wmad,
                                       label_site=label_site)

    def site_conditionals(self, W, phi, label_index, x, grid_x, grid_phi, levels=None, get_wmad=True, compute="f64", label_site=None):
        """mpst_site_conditionals: the leave-one-out conditional p(x_t | x_{!=t}) of every site of every COMPLETE series, each under
        the class ``label_index[i]``; see ``conditionals.site_conditionals_model``.  Returns (nll, pit, median, err, q, seconds)."""
        from .conditionals import site_conditionals_model
        return site_conditionals_model(self, W, phi, label_index, x, grid_x, grid_phi, levels=levels, get_wmad=get_wmad, compute=compute,
                                       label_site=label_site)

    def marginal_conditionals(self, W, phi, label_index, missing, x, grid_x, grid_phi, levels=None, get_wmad=True, label_site=None):
        """mpst_marginal_conditionals: the distribution of every site, known or missing, of every series given the known values of
        its OTHER sites, the missing ones summed out (Born rule), each under the class ``label_index[i]``; see
        ``conditionals.marginal_conditionals_model``.  Returns a ``MarginalConditionals``."""
        from .conditionals import marginal_conditionals_model
        return marginal_conditionals_model(self, W, phi, label_index, missing, x, grid_x, grid_phi, levels=levels, get_wmad=get_wmad,
                                           label_site=label_site)

    def observed_conditionals(self, W, phi, label_index, model, x, grid_x, grid_phi, levels=None, get_wmad=True, label_site=None,
                              return_operators=False):
        """mpst_observed_conditionals: ``marginal_conditionals`` with a measurement - exact, missing, Gaussian noise, an interval or
        an operator - at every site (``model``: an ``observations.ObservationModel`` in the encoding's domain); see
        ``observations.observed_conditionals_model``.  Returns an ``ObservedConditionals``."""
        from .observations import observed_conditionals_model
        return observed_conditionals_model(self, W, phi, label_index, model, x, grid_x, grid_phi, levels=levels, get_wmad=get_wmad,
                                           label_site=label_site, return_operators=return_operators)

    def window_conditionals(self, W, phi, label_index, max_width, label_site=None):
        """mpst_window_conditionals: -ln P(x_t .. x_{t+w-1} | the rest) of every COMPLETE series, every start t and every width
        w <= ``max_width``, each under the class ``label_index[i]``; see ``conditionals.window_conditionals_model``.
        Returns (nll (N, T, max_width), seconds)."""
        from .conditionals import window_conditionals_model
        return window_conditionals_model(self, W, phi, label_index, max_width, label_site=label_site)

    def impute_phases(self):
        """(environment pass, density sweep) device seconds of the last imputation call; after ``site_conditionals``: (walk, grid phase);
        after ``window_conditionals``: (walk, window kernel); after ``marginal_conditionals``: (walk, grid phase); after ``segment_model``:
        (table kernels, walk kernel); after ``rolling_model``: (tables + rows + score, grid phase); after ``observed_conditionals``:
        (operators + walk, grid phase)."""
        out = np.zeros(2)
        self._chk(self.lib.mpst_get_impute_phases(self.ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return float(out[0]), float(out[1])

    def impute_info(self):
        """how the last imputation call ran: {"closed_form_densities": bool (Fourier / Legendre grid states on a uniform grid),
        "batched_sweep": bool (sixteen chains per workgroup), "env_workgroups": workgroups of the environment pass (one per
        instance), "chains": (instance, trajectory) pairs the sweep ran for}; after ``segment_model``: "env_workgroups" is the number of
        blocks of series the walk kernel was launched for and "chains" the (series, start) items it walked; after ``rolling_model``:
        the blocks of series and the blocks of targets of a block of series"""
        out = (C.c_int32 * 4)()
        self._chk(self.lib.mpst_get_impute_info(self.ctx, out, 4))
        return {"closed_form_densities": bool(out[0]), "batched_sweep": bool(out[1]), "env_workgroups": int(out[2]), "chains": int(out[3])}

    def normalize(self):
        self._chk(self.lib.mpst_normalize(self.ctx))

    # -- diagnostics ------------------------------------------------------------------
    def set_profile(self, mask):
        self._chk(self.lib.mpst_set_profile(self.ctx, int(mask)))

    def get_profile(self):
        us = np.zeros(16)
        cnt = np.zeros(16, dtype=np.int64)
        self._chk(self.lib.mpst_get_profile(self.ctx, us.ctypes.data_as(C.POINTER(C.c_double)),
                                            cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return {k: (us[i], int(cnt[i])) for i, k in enumerate(L.KERNEL_CLASSES)}

    def info(self):
        out = (C.c_int32 * 23)()
        self._chk(self.lib.mpst_get_info_n(self.ctx, out, 23))
        return {"four_launch_chain": bool(out[18]), "tail_redos": out[19], "tail_side_workgroups": bool(out[20]),
                "rebuild_side": bool(out[21]), "rebuild_side_steps": out[22],
                "subspace_attempted": out[16], "subspace_accepted": out[17], "fused": bool(out[0]), "large_bond": bool(out[1]), "nparts": out[2], "nchunks": out[3], "cap": out[4],
                "ranks": out[5], "graph": bool(out[6]), "library_eig_fallbacks": out[7], "persistent_tridiag_aborts": out[8],
                "xcd_local_misplaced": out[9], "sliced_bond_gemms": bool(out[10]), "grad_shares": out[11],
                "eig_merged": bool(out[12]), "large_bond_sweep_redos": out[13], "large_bond_verdict_per_sweep": bool(out[14]),
                "typed_kernels": bool(out[15]), "dtype": (out[15] - 1) if out[15] else L.F64}

    def eig_phases(self):
        us = np.zeros(6)
        self._chk(self.lib.mpst_get_eig_phases(self.ctx, us.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(("tridiag", "bisect", "eigvec", "backtransform", "verify", "tridiag_cycles"), us.tolist()))

    def tail_phases(self):
        """Stamps (us since its first tile workgroup started) of the last stamped k_bond_tail launch: that tile workgroup, the first
        workgroup of the next bond's tensor, the first back-split workgroup."""
        us = np.zeros(55)
        self._chk(self.lib.mpst_get_tail_phases(self.ctx, us.ctypes.data_as(C.POINTER(C.c_double))))
        if self.info()["tail_side_workgroups"]:
            # the S tile and the overlap product come from the side workgroups of k_eig_trivec: 15 stamps
            host = ("start", "candidates_requested", "side_results_requested", "bond_dims_known", "all_requested", "trace_published", "truncation",
                    "candidates_in_lds", "polished", "role_requested", "env_rows", "z_rowdot", "tile_done", "role_done", "stores_drained")
        else:
            # MPST_TAIL_PRE=0, both formed in the tail: 18 stamps, of which the 16 slots keep the first 16
            host = ("start", "candidates_requested", "factors_requested", "bond_dims_known", "all_requested", "factors_in_lds", "truncation",
                    "candidates_in_lds", "polished", "overlap_product_issued", "role_requested", "b1_passed", "s_tile_formed", "env_rows", "z_rowdot",
                    "tile_done", "role_done", "stores_drained")
        plain = tuple(k for k in host if k != "role_done")          # a workgroup without a role takes no such stamp
        pick = lambda names, x: {k: round(float(v), 2) for k, v in zip(names, x) if v >= 0 or k == "start"}
        # workgroup 0 (hosts a job of the next bond's tensor when the sweep goes on), the last workgroup (no role); the side workgroups of the
        # bond's k_eig_trivec launch ran before the tail: negative times
        return {"host_of_a_chain_job": pick(host, us[:16]), "plain_tile": pick(plain, us[16:32]),
                "side_workgroups": {"count": int(us[32]), "first_start": round(float(us[33]), 2), "last_start": round(float(us[34]), 2),
                                    "last_end": round(float(us[35]), 2)},
                "bonds_by_candidate_orthogonality": dict(zip(("below_1e-13", "below_1e-8", "below_3e-5", "above"), [int(x) for x in us[48:52]])),
                "all_workgroups": {"first_start": round(float(us[52]), 2), "last_start": round(float(us[54]), 2), "last_end": round(float(us[53]), 2)}}

    def selftest_mfma(self, A, B):
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        K = A.shape[1]
        out = np.zeros((16, 16))
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mpst_selftest_mfma(self.ctx, A.ctypes.data_as(dp), B.ctypes.data_as(dp), K,
                                              out.ctypes.data_as(dp)))
        return out

    def selftest_eig(self, G, alg=0):
        """mpst_selftest_eig: one solve of the bond eigensolver on the symmetric positive semi-definite ``G`` (n <= 128: the solver of
        the fused chain; larger: the large-bond solvers).  Returns ``(lam, E, info)``: ``lam`` descending (n entries), column k of
        ``E`` (n x n) vector k, ``info`` the route: -1 tridiagonal route verified on the device, 0 its verification handed over to
        Jacobi, > 0 sweeps of the Jacobi path asked for; n > 128: -3 blocked solver, -2 multi-workgroup Jacobi.  Delivered are the
        min(n, 32) largest pairs on the tridiagonal route (min(n, 64) with bit 3), everything on a Jacobi route (zero vectors for zero
        eigenvalues) and min(n, 128) pairs above 128; the rest is zero.  ``alg`` is a bit field:

        * bits 0-1: 0 tridiagonal route with its fallback, 1 Jacobi alone; n > 128: 0 blocked solver (Jacobi if its verification asks
          for it), 2 Jacobi alone.
        * bit 2 (4): pair mode, n even.  ``G = [[A, -B], [B, A]]`` embeds the Hermitian ``A + iB``; ``lam`` holds every eigenvalue of
          it twice (``lam[2k] == lam[2k + 1]``), column ``2k`` of ``E`` the computed vector ``u`` (complex: ``E[:n//2, 2k] + 1j *
          E[n//2:, 2k]``) and column ``2k + 1`` its partner ``J u = (-u_im, u_re)``.
        * bit 3 (8), n <= 128: up to 64 eigenpairs; vectors only for pairs above 1e-13 of the largest.
        * bit 4 (16), n <= 128: through the gated launcher of the subspace solver's Rayleigh-Ritz problem with an open gate (always the
          tridiagonal route with 64 pairs: bits 0-2 must be 0).
        * bit 5 (32), with bit 4: closed gate.  ``lam``, ``E`` and ``info`` are filled with -7 on the device first and must come back
          untouched.

        Bit 3 or 4 with n > 128, bit 5 without bit 4, bit 4 with bits 0-2 and higher bits raise MPSTError(MPST_ERR_INVALID)."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        n = G.shape[0]
        lam = np.zeros(n)
        E = np.zeros((n, n))
        sw = C.c_int32()
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mpst_selftest_eig(self.ctx, G.ctypes.data_as(dp), n, alg, lam.ctypes.data_as(dp),
                                             E.ctypes.data_as(dp), C.byref(sw)))
        return lam, E, sw.value


def sweep_batch(engines):
    """mpst_sweep_batch: one sweep of K independent fits of the same shape in ONE launch chain (every launch carries all K
    fits).  ``engines``: SweepEngines prepared like for ``sweep()`` (options, data, MPS, build_caches).  Returns one stats dict per
    engine; ``seconds`` is the device time of the whole batch.  Raises MPSTError(MPST_ERR_UNSUPPORTED) for fits outside the
    headline chain or of different shapes - drive those with ``sweep()`` one by one."""
    lib = L.load()
    K = len(engines)
    arr = (C.c_void_p * K)(*[e.ctx.value for e in engines])
    st = (L.mpst_sweep_stats * K)()
    rc = lib.mpst_sweep_batch(arr, K, st)
    if rc:
        try:
            engines[0]._chk(rc)
        except L.SVDError as err:        # which fits failed (the others are intact): fit_batch goes on with those
            err.svd_status = [int(s.svd_status) for s in st]
            raise
    return [{"seconds": s.seconds, "max_chi": s.max_chi, "eig_sweeps_total": s.eig_sweeps_total, "eig_fallbacks": s.eig_fallbacks} for s in st]


def sweep_batch_multi(engines, groups=None):
    """mpst_sweep_batch_multi: one sweep of K independent fits dealt over several devices - ``groups[k]`` names the group of engine k
    (default: its device); every group is one ``sweep_batch`` launch chain on its own host thread, all groups run concurrently, no
    collective.  Returns one stats dict per engine (``seconds`` = device time of its group)."""
    lib = L.load()
    K = len(engines)
    arr = (C.c_void_p * K)(*[e.ctx.value for e in engines])
    g = None if groups is None else (C.c_int32 * K)(*[int(x) for x in groups])
    st = (L.mpst_sweep_stats * K)()
    rc = lib.mpst_sweep_batch_multi(arr, K, g, st)
    if rc:
        engines[0]._chk(rc)
    return [{"seconds": s.seconds, "max_chi": s.max_chi, "eig_sweeps_total": s.eig_sweeps_total, "eig_fallbacks": s.eig_fallbacks} for s in st]


def classify_batch(engines, which=1, return_overlaps=False):
    """mpst_classify_batch: K models scored on their own data sets ``which`` in two kernel launches for the whole batch (one walks
    every chain, one forms the losses) instead of T + 2 launches per model.  ``engines``: Float64 SweepEngines on one device
    with the same T, d, C and d * chi <= 128; set sizes and bond dimensions may differ.  Returns one dict per engine:
    ``pred`` (N_k,) class slots, ``mse`` / ``kld`` / ``acc`` as ``eval``, ``conf`` (C, C) [truth][prediction], and ``yhat``
    (N_k, C) overlaps with ``return_overlaps``.  The engines' training caches are left alone.  Raises
    MPSTError(MPST_ERR_UNSUPPORTED) for fits outside these limits - score those with ``classify`` / ``eval``."""
    lib = L.load()
    K = len(engines)
    Cn = engines[0].C
    arr = (C.c_void_p * K)(*[e.ctx.value for e in engines])
    preds = [np.zeros(e.N[which], dtype=np.int32) for e in engines]
    pp = (C.c_void_p * K)(*[p.ctypes.data for p in preds])
    yh, yp = None, None
    if return_overlaps:
        yh = [np.zeros((e.N[which], Cn)) for e in engines]
        yp = (C.c_void_p * K)(*[y.ctypes.data for y in yh])
    loss3 = np.zeros((K, 3))
    conf = np.zeros((K, Cn, Cn), dtype=np.int64)
    rc = lib.mpst_classify_batch(arr, K, int(which), pp, yp, loss3.ctypes.data_as(C.POINTER(C.c_double)),
                                 conf.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc:
        engines[0]._chk(rc)
    out = []
    for k in range(K):
        r = {"pred": preds[k], "mse": float(loss3[k, 0]), "kld": float(loss3[k, 1]), "acc": float(loss3[k, 2]), "conf": conf[k]}
        if return_overlaps:
            r["yhat"] = yh[k]
        out.append(r)
    return out


def comm_library():
    """Which librccl the HIP library has bound (it is loaded at run time, never linked): path + how it was found, the
    library's ncclGetVersion code and the NCCL_VERSION_CODE the HIP library was compiled against."""
    lib = L.load()
    buf = C.create_string_buffer(1024)
    ver, built = C.c_int32(0), C.c_int32(0)
    rc = lib.mpst_comm_library(buf, 1024, C.byref(ver), C.byref(built))
    return {"ok": rc == 0, "library": buf.value.decode(), "version": ver.value, "built_against": built.value}
