"""What the model queries answer to a malformed ``mpst_impute_model``: every entry point that takes one, handed a model that is wrong in
exactly one way through raw ctypes, returns the error code and the message pinned here, and the next valid call on the same context
gives the bits of a fresh context.  The model is the smallest with an inner bond: T = 3, d = 2, chi = (1, 2, 2, 1), C = 2, N = 2,
real fp64, five grid values.  One assertion more: after a marginal call ``impute_phases()`` is (its device seconds, 0)."""
import ctypes as C

import numpy as np
import pytest

import mpstime_jl_amd as mt
from mpstime_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

T, D, NCLS, N, NGRID = 3, 2, 2, 2, 5
CHI = (1, 2, 2, 1)
dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)

_rng = np.random.default_rng(20261019)
SITES = [_rng.standard_normal((CHI[j], D, CHI[j + 1]) + ((NCLS,) if j == T - 1 else ())) for j in range(T)]
_ang = _rng.uniform(0.0, np.pi, (N, T))
PHI = np.ascontiguousarray(np.stack([np.cos(_ang), np.sin(_ang)], axis=2))
LABELS = np.array([0, 1], dtype=np.int32)
MISSING = np.array([[0, 1, 0], [1, 0, 1]], dtype=np.uint8)
X_OBS = np.ascontiguousarray(np.cos(_ang))
GRID_X = np.linspace(-1.0, 1.0, NGRID)
GRID_PHI = np.ascontiguousarray(np.stack([GRID_X, np.sqrt(1.0 - 0.75 * GRID_X ** 2)], axis=1))
LEVEL = np.array([0.5])
for _a in SITES + [PHI, LABELS, MISSING, X_OBS, GRID_X, GRID_PHI, LEVEL]:
    _a.setflags(write=False)

# malformation -> (what it does to the struct's fields, the message every entry point answers; the code is MPST_ERR_INVALID)
MALFORMED = {
    "chi[0]=2": (dict(chi={0: 2}), "chi[0] and chi[T] must be 1"),
    "chi[1]=0": (dict(chi={1: 0}), "chi[1] < 1"),
    "site[1]=NULL": (dict(null_site=1), "site[1] is NULL"),
    "label_site=T": (dict(label_site=T), "label_site out of range"),
    "N=0": (dict(N=0), "empty model or data"),
}


class Model:
    """the mpst_impute_model of the module's arrays, with one field changed; the buffers live with the object"""

    def __init__(self, chi=None, null_site=None, label_site=T - 1, N=N):
        self.bufs = [np.asfortranarray(np.transpose(t, (1, 0, 2) + ((3,) if t.ndim == 4 else ()))) for t in SITES]
        self.ptrs = (C.c_void_p * T)(*[None if j == null_site else b.ctypes.data for j, b in enumerate(self.bufs)])
        self.chi = np.array(CHI, dtype=np.int32)
        for j, v in (chi or {}).items():
            self.chi[j] = v
        self.struct = L.ImputeModel(N, T, D, NCLS, label_site, 0, 0, C.cast(self.ptrs, C.POINTER(C.c_void_p)), self.chi.ctypes.data_as(i32p),
                                    PHI.ctypes.data_as(C.c_void_p), LABELS.ctypes.data_as(i32p))


def _impute_args(method):
    o = L.ImputeOpts(method, 0, 1, 1, 1, 0, 0.0)
    return o, (MISSING.ctypes.data_as(C.POINTER(C.c_uint8)), GRID_X.ctypes.data_as(dp), C.c_void_p(GRID_PHI.ctypes.data), NGRID, C.byref(o))


def run(eng, m):
    o, head = _impute_args(0)
    x, err, sec = np.zeros((N, T)), np.zeros((N, T)), C.c_double()
    rc = eng.lib.mpst_impute_model_run(eng.ctx, C.byref(m.struct), *head, None, x.ctypes.data_as(dp), err.ctypes.data_as(dp), C.byref(sec))
    return rc, (x, err)


def traj(eng, m):
    o, head = _impute_args(2)
    x, err, sec = np.zeros((N, 2, T)), np.zeros((N, 2, T)), C.c_double()
    rc = eng.lib.mpst_impute_model_traj(eng.ctx, C.byref(m.struct), *head, 2, None, 7, None, x.ctypes.data_as(dp), err.ctypes.data_as(dp),
                                        C.byref(sec))
    return rc, (x, err)


def dist(eng, m):
    o, head = _impute_args(0)
    x, err, q, cdf, sec = np.zeros((N, T)), np.zeros((N, T)), np.zeros((N, T, 1)), np.zeros((N, 2, NGRID)), C.c_double()
    rc = eng.lib.mpst_impute_model_dist(eng.ctx, C.byref(m.struct), *head, x.ctypes.data_as(dp), err.ctypes.data_as(dp), C.byref(sec), 1,
                                        LEVEL.ctypes.data_as(dp), q.ctypes.data_as(dp), 1, 2, cdf.ctypes.data_as(dp))
    return rc, (x, err, q, cdf)


def marginal(eng, m):
    logp, sec = np.zeros((N, NCLS)), C.c_double()
    rc = eng.lib.mpst_marginal_model(eng.ctx, C.byref(m.struct), MISSING.ctypes.data_as(C.POINTER(C.c_uint8)), logp.ctypes.data_as(dp), C.byref(sec))
    return rc, (logp,)


def site_conditionals(eng, m):
    o = L.SiteCondOpts(0, 1, 1, 0, LEVEL.ctypes.data_as(dp))
    nll, pit, med, err, q, sec = [np.zeros((N, T)) for _ in range(4)] + [np.zeros((N, T, 1)), C.c_double()]
    rc = eng.lib.mpst_site_conditionals(eng.ctx, C.byref(m.struct), X_OBS.ctypes.data_as(dp), GRID_X.ctypes.data_as(dp), C.c_void_p(GRID_PHI.ctypes.data),
                                        NGRID, C.byref(o), nll.ctypes.data_as(dp), pit.ctypes.data_as(dp), med.ctypes.data_as(dp),
                                        err.ctypes.data_as(dp), q.ctypes.data_as(dp), C.byref(sec))
    return rc, (nll, pit, med, err, q)


def entanglement(eng, m):
    bee, see = np.zeros((NCLS, T)), np.zeros((NCLS, T))
    rc = eng.lib.mpst_entanglement(eng.ctx, C.byref(m.struct), bee.ctypes.data_as(dp), see.ctypes.data_as(dp))
    return rc, (bee, see)


def see_variation(eng, m):
    out, sec = np.zeros((N, T, T)), C.c_double()
    rc = eng.lib.mpst_see_variation(eng.ctx, C.byref(m.struct), 0, out.ctypes.data_as(dp), C.byref(sec))
    return rc, (out,)


ENTRIES = {"mpst_impute_model_run": run, "mpst_impute_model_traj": traj, "mpst_impute_model_dist": dist, "mpst_marginal_model": marginal,
           "mpst_site_conditionals": site_conditionals, "mpst_entanglement": entanglement, "mpst_see_variation": see_variation}
PAIRS = [(e, bad) for e in ENTRIES for bad in MALFORMED if not (e == "mpst_entanglement" and bad == "N=0")]      # (it needs no phi)


@pytest.fixture(scope="module")
def eng():
    e = mt.SweepEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fresh():
    """entry point -> the outputs of the valid call, each on a context of its own that has seen nothing else"""
    out = {}
    for name, call in ENTRIES.items():
        e = mt.SweepEngine(0)
        try:
            rc, arrays = call(e, Model())
            assert rc == 0, (name, rc, e.lib.mpst_last_error(e.ctx))
        finally:
            e.close()
        assert all(np.all(np.isfinite(a)) for a in arrays) and any(np.any(a != 0.0) for a in arrays), name
        out[name] = arrays
    return out


@pytest.mark.parametrize("entry,bad", PAIRS)
def test_one_wrong_field_by_code_and_message(eng, fresh, entry, bad):
    change, text = MALFORMED[bad]
    rc, _ = ENTRIES[entry](eng, Model(**change))
    msg = eng.lib.mpst_last_error(eng.ctx).decode()
    assert rc == L.MPST_ERR_INVALID and msg == text, (rc, msg)
    rc, arrays = ENTRIES[entry](eng, Model())
    assert rc == 0, eng.lib.mpst_last_error(eng.ctx)
    assert len(arrays) == len(fresh[entry]) and all(np.array_equal(a, b) for a, b in zip(arrays, fresh[entry]))


def test_phases_after_a_marginal_call_are_its_own(eng):
    rc, _ = run(eng, Model())           # an imputation first: both of its phases ran
    assert rc == 0
    logp, seconds = eng.marginal_model(SITES, PHI, MISSING)
    assert seconds > 0.0
    assert eng.impute_phases() == (seconds, 0.0)
