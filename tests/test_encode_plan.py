"""The encoding planner (csrc/mpst_encode_plan.h) on the CPU: tests/encode_plan_main.cpp, which includes nothing but that header, is
compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program.  Every table it is handed is a heap
array of exactly the documented length, so a check or a table builder that reads past one fails the run.

Tables: what encode_tables returns - the arrays the kernels index - against NumPy: the projected bases' sorted orders and slots, the
Sahand-Legendre pack with its zero-site flags, the split bases' edges and stride; every table inside its vector.
Rejections: every case tests/test_gpu_split.py::test_split_abi_errors, test_gpu_kde.py::test_kde_abi_errors,
test_gpu_proj.py::test_proj_abi_errors and test_gpu_encode.py send to the library, with the code those tests expect, and the limit
cases they expect to pass."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")

INVALID, UNSUPPORTED = -1, -2
LN, LNN, FOURIER, STOUDENMIRE, SAHAND, UNIFORM = range(6)          # MPST_BASIS_*


def _list(a):
    return ",".join(repr(float(v)) if np.asarray(a).dtype.kind == "f" else str(int(v)) for v in np.asarray(a).ravel())


def _case(kind, *head, null=False, **tables):
    return ":".join([kind] + [str(h) for h in head] + [f"{k}={_list(v)}" for k, v in tables.items() if v is not None] + (["null"] if null else []))


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def _proj_cases():
    rng = np.random.default_rng(5)
    out = {}
    for name, T, d, basis, orders in (
            ("unsorted", 3, 4, LNN, [[5, 3, 9, 1], [2, 7, 0, 4], [112, 8, 6, 7]]),
            ("repeated", 2, 4, LN, [[3, 1, 3, 1], [2, 2, 2, 2]]),
            ("fourier_negative", 2, 5, FOURIER, [[0, 1, -1, 2, -2], [-80, 80, 0, -3, -3]]),
            ("d1", 3, 1, LNN, [[4], [0], [2]]),
            ("d16", 2, 16, LN, rng.integers(0, 113, (2, 16))),
            ("T1", 1, 3, FOURIER, [[2, -2, 0]])):
        o = np.asarray(orders, dtype=np.int32)
        inv = rng.uniform(0.2, 1.5, T) if basis == LN else None
        out[name] = (_case("proj", T, d, basis, int(np.abs(o).max()), orders=o, inv=inv), o, inv)
    return out


def _kde_cases():
    rng = np.random.default_rng(6)
    out = {}
    for name, T, d, K, per_site, zero in (("per_site", 4, 3, 9, 1, None), ("shared", 4, 3, 9, 0, None), ("zero_site", 3, 2, 5, 1, 1),
                                          ("npoints3", 2, 4, 3, 1, None), ("shared_zero", 3, 2, 4, 0, 0)):
        S = T if per_site else 1
        tab = dict(lo=rng.uniform(-1, 0, S), step=rng.uniform(0.1, 0.3, S), minx=rng.uniform(0.01, 0.1, S), scale=rng.uniform(0.5, 2, S),
                   coef=rng.uniform(0, 1, (S, K + 2)), cvecs=rng.normal(size=(S, d, d)))
        if zero is not None:
            tab["cvecs"][zero] = 0.0
        out[name] = (_case("kde", T, d, K, per_site, **tab), tab, S)
    return out


def _split_cases():
    rng = np.random.default_rng(7)
    out = {}
    for name, T, nbins, aux, per_site in (("shared_1", 3, 1, 2, 0), ("per_site_1", 3, 1, 2, 1), ("shared_512", 2, 512, 1, 0), ("per_site_512", 2, 512, 1, 1),
                                          ("per_site_3", 5, 3, 2, 1)):
        bins = np.sort(rng.uniform(-1, 1, ((T if per_site else 1), nbins + 1)), axis=1)
        out[name] = (_case("split", T, nbins * aux, LNN, aux, nbins, per_site, bins=bins), bins, nbins + 1 if per_site else 0)
    return out


PROJ, KDE, SPLIT = _proj_cases(), _kde_cases(), _split_cases()

# ---- rejections: (case, expected code) ---------------------------------------------------------------------------------------------
_up = [-1.0, 0.0, 1.0]
_ord = [[1, 3, 5], [2, 1, 4]]
_inv = [0.7, 0.9]


def _kde(T=2, d=3, npoints=5, per_site=1, null=False, zero_site=None, **over):
    """the tables of test_kde_abi_errors' shape: site 1 has zero coefficients - and, with ``zero_site``, that value in its other tables,
    which are not read -; a scalar replaces site 0's entry, None drops the table"""
    rng = np.random.default_rng(8)
    dd = max(d, 1)
    tab = dict(lo=rng.uniform(-1, 0, T), step=rng.uniform(0.1, 0.3, T), coef=rng.uniform(0, 1, (T, npoints + 2)), minx=rng.uniform(0.01, 0.1, T),
               scale=rng.uniform(0.5, 2, T), cvecs=rng.normal(size=(T, dd, dd)))
    tab["cvecs"][1] = 0.0
    if zero_site is not None:
        for k in ("lo", "step", "coef", "minx", "scale"):
            tab[k][1] = zero_site
    for k, v in over.items():
        if v is None:
            tab[k] = None
        else:
            tab[k][0] = v
    return _case("kde", T, d, npoints, per_site, null=null, **tab)


def _proj(basis=LN, orders=_ord, inv=_inv, max_order=5, d=3, null=False):
    o = None if orders is None else np.resize(np.asarray(orders, dtype=np.int32), (2, d))
    return _case("proj", 2, d, basis, max_order, null=null, orders=o, inv=inv)


REJECTS = [
    # test_gpu_encode.py
    (_case("closed", STOUDENMIRE, 3), INVALID), (_case("closed", SAHAND, 3), INVALID), (_case("closed", 9, 4), UNSUPPORTED),
    (_case("closed", -1, 4), UNSUPPORTED),
    # test_split_abi_errors
    (_case("split", 2, 5, LNN, 2, 2, 0, bins=_up), INVALID),                                   # d != nbins * aux_dim
    (_case("split", 2, 4, LNN, 2, 2, 0, bins=[-1.0, 0.5, 0.0]), INVALID),                      # decreasing edges
    (_case("split", 2, 6, STOUDENMIRE, 3, 2, 0, bins=[0.0, 0.5, 1.0]), UNSUPPORTED),           # Stoudenmire needs aux_dim 2
    (_case("split", 2, 6, SAHAND, 3, 2, 0, bins=[0.0, 0.5, 1.0]), UNSUPPORTED),                # Sahand needs an even aux_dim
    (_case("split", 2, 4, LNN, 2, 2, 0), INVALID),                                             # NULL bins
    (_case("split", 2, 4, null=True), INVALID),                                                # NULL options
    (_case("split", 2, 4, LNN, 2, 0, 0, bins=_up), INVALID),                                   # nbins < 1
    (_case("split", 2, 1026, LNN, 2, 513, 0, bins=np.linspace(-1, 1, 514)), INVALID),          # nbins > 512
    (_case("split", 2, 4, 9, 2, 2, 0, bins=_up), UNSUPPORTED),                                 # an auxiliary basis outside the six
    (_case("split", 2, 4, LNN, 2, 2, 2, bins=_up), INVALID),                                   # per_site
    (_case("split", 0, 4, LNN, 2, 2, 0, bins=_up), INVALID),                                   # T < 1
    # test_kde_abi_errors
    (_kde(npoints=2), INVALID), (_kde(per_site=2), INVALID), (_kde(null=True), INVALID), (_kde(d=0), INVALID), (_kde(d=17), INVALID),
] + [(_kde(**{k: None}), INVALID) for k in ("lo", "step", "coef", "minx", "scale", "cvecs")
] + [(_kde(**{k: v}), INVALID) for k in ("step", "scale", "minx") for v in (0.0, -1.0, np.inf, np.nan)
] + [
    # test_proj_abi_errors
    (_proj(orders=[[1, 3, 6], [2, 1, 4]]), INVALID), (_proj(orders=[[1, -1, 5], [2, 1, 4]]), INVALID), (_proj(max_order=4), INVALID),
    (_proj(max_order=-1), INVALID), (_proj(max_order=7 * 16 + 1), INVALID),
    (_proj(basis=FOURIER, orders=[[0, 81, -1], [2, 1, 4]], max_order=81), INVALID),
    (_proj(basis=FOURIER, orders=[[0, 3, -4], [2, 1, 3]], max_order=3), INVALID),
    (_proj(orders=None), INVALID), (_proj(inv=None), INVALID),
    (_proj(inv=[0.3, 0.0]), INVALID), (_proj(inv=[-1.0, 0.3]), INVALID), (_proj(inv=[np.inf, 0.3]), INVALID), (_proj(inv=[0.3, np.nan]), INVALID),
    (_proj(basis=STOUDENMIRE), INVALID), (_proj(basis=UNIFORM), INVALID), (_proj(basis=-1), INVALID), (_proj(basis=6), INVALID),
    (_proj(null=True), INVALID), (_proj(basis=LNN, d=0), INVALID), (_proj(basis=LNN, d=17), INVALID),
    (_proj(orders=[[1, 3, 113], [2, 1, 4]], max_order=113), INVALID),
]
ACCEPTS = [
    _case("closed", STOUDENMIRE, 2), _case("closed", SAHAND, 4), _case("closed", LN, 3), _case("closed", UNIFORM, 3), _case("closed", FOURIER, 5),
    _case("split", 2, 4, LNN, 2, 2, 0, bins=_up),
    _case("split", 2, 4, STOUDENMIRE, 2, 2, 0, bins=_up), _case("split", 2, 8, SAHAND, 4, 2, 0, bins=_up),
    _kde(), _kde(npoints=3), _kde(zero_site=np.nan),
    _proj(), _proj(basis=LNN, inv=None),                                                       # no norms for the unnormalised families
    _proj(basis=FOURIER, orders=[[0, 80, -80], [2, 1, -1]], inv=None, max_order=80),           # the limits themselves
    _proj(basis=LNN, orders=[[112, 0, 5], [2, 1, 4]], inv=None, max_order=112),
]


@pytest.fixture(scope="module")
def doc(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("encode_plan") / "encode_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "encode_plan_main.cpp"), "-o", exe])
    args = [c[0] for c in list(PROJ.values()) + list(KDE.values()) + list(SPLIT.values())] + [c for c, _ in REJECTS] + ACCEPTS
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    got = {c["case"]: c for c in json.loads(out)["cases"]}
    assert set(got) == set(args)
    return got


def _table(c, name, vec):
    off, n = c["spans"][name]
    assert 0 <= off and 0 <= n and off + n <= len(c[vec]), (name, off, n, len(c[vec]))
    return np.array(c[vec][off:off + n])


def _inside(c, present):
    """every table of `present` lies inside its vector, the others are absent, and nothing is uploaded that no table covers"""
    for name, (off, n) in c["spans"].items():
        if name in present:
            _table(c, name, present[name])
        else:
            assert (off, n) == (-1, 0), name
    for vec in ("f64", "i32"):
        assert sum(c["spans"][k][1] for k, v in present.items() if v == vec) == len(c[vec])


@pytest.mark.parametrize("name", sorted(PROJ))
def test_projected_orders_and_slots(doc, name):
    case, orders, inv = PROJ[name]
    c = doc[case]
    T, d = orders.shape
    assert c["code"] == 0 and c["aux_dim"] == d and c["is_complex"] == int(c["family"] == FOURIER)
    _inside(c, {"proj_tab": "i32", **({"proj_inv": "f64"} if inv is not None else {})})
    tab = _table(c, "proj_tab", "i32").reshape(T, 2, d)
    for t in range(T):
        slot = np.argsort(orders[t], kind="stable")
        assert np.array_equal(tab[t, 1], slot) and np.array_equal(tab[t, 0], orders[t][slot]), t
        assert sorted(tab[t, 1]) == list(range(d))                          # a permutation: every slot written once, none out of range
    if inv is not None:
        assert np.array_equal(_table(c, "proj_inv", "f64"), inv)


@pytest.mark.parametrize("name", sorted(KDE))
def test_kde_pack_and_zero_flags(doc, name):
    case, tab, S = KDE[name]
    c = doc[case]
    assert c["code"] == 0 and c["family"] == LNN and c["is_complex"] == 0
    names = ("lo", "step", "minx", "scale", "coef", "cvecs")
    _inside(c, {**{"kde_" + k: "f64" for k in names}, "kde_zero": "i32"})
    assert np.array_equal(np.array(c["f64"]), np.concatenate([tab[k].ravel() for k in names]))          # the pack, in the kernel's order
    for k in names:
        assert np.array_equal(_table(c, "kde_" + k, "f64"), tab[k].ravel()), k
    assert np.array_equal(_table(c, "kde_zero", "i32"), [int(np.all(tab["cvecs"][s] == 0)) for s in range(S)])
    if "zero" in name:
        assert sum(c["i32"]) == 1


@pytest.mark.parametrize("name", sorted(SPLIT))
def test_split_edges_and_stride(doc, name):
    case, bins, stride = SPLIT[name]
    c = doc[case]
    assert c["code"] == 0 and c["family"] == LNN and c["aux_dim"] == int(case.split(":")[4])
    _inside(c, {"bins": "f64"})
    assert np.array_equal(_table(c, "bins", "f64"), bins.ravel()) and c["bin_stride"] == stride


def test_rejections(doc):
    for case, code in REJECTS:
        c = doc[case]
        assert c["code"] == code and c["text"], case
        assert "spans" not in c


def test_accepted_limit_cases(doc):
    for case in ACCEPTS:
        assert doc[case]["code"] == 0 and doc[case]["text"] == "", case


def test_messages_the_callers_match_on(doc):
    assert "d = 2" in doc[_case("closed", STOUDENMIRE, 3)]["text"] and "even" in doc[_case("closed", SAHAND, 3)]["text"]
    assert doc[_kde(null=True)]["text"] == "NULL density-estimate options or table"
    assert doc[_proj(null=True)]["text"] == "NULL projected-basis options or order table"
    assert doc[_case("split", 2, 4, null=True)]["text"] == "NULL split options or bin edges"
