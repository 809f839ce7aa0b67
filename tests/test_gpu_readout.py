"""The classifier read-out with the label index on EVERY site: mpst_eval, mpst_classify, mpst_classify_batch and mpst_normalize
against the long-double reference of tests/readout_ref.py.

A case is a seeded Gaussian chain with a ragged bond profile (readout_ref.ragged_chain) and random unit product states
(marginal_ref.random_states), loaded with set_options / set_dataset / set_mps(W, label_site=p): no sweep, no build_caches, so that no
case depends on a training kernel.  Set 1 holds all N series, set 0 every second one with labels of its own.

Bounds (the ones the suite already holds these quantities to):
    overlaps  float64 / complex128: 1e-11 of the largest overlap (test_gpu_tuning._check_scores)   float32 / complex64: 2e-5
    mse, kld  float64 / complex128: 1e-10 of max(1, |reference|)                                  float32 / complex64: 2e-5
    accuracy, confusion counts and the prediction of every series: exact.
Exact predictions are a property of the inputs: every case asserts that the relative gap between the two largest |overlaps| of
every series of the reference exceeds 100 x the overlap bound of its element type.  The seeds in SEEDS were chosen on the CPU for
that (the first seed from 1 upwards that satisfies it); no series is ever left out.
For the fp32 types the inputs are rounded to the element type first and the reference runs on the rounded inputs.
Measured errors: docs/lab/readout_label_site_notes.md (run with -s for the figures of every case)."""
import collections
import functools
import types

import numpy as np
import pytest

from oracle import ref_complex as RC
from oracle import ref_numpy as R
from tests import readout_ref as RR
from tests.marginal_ref import random_states

pytestmark = pytest.mark.gpu

OV_BOUND = {"f64": 1e-11, "f32": 2e-5}
LOSS_BOUND = {"f64": 1e-10, "f32": 2e-5}
# variant: element type the engine runs in, MPST_TYPED set, the row of the bounds
VARIANTS = {"plain": ("float64", False, "f64"), "typed-float64": ("float64", True, "f64"), "float32": ("float32", False, "f32"),
            "complex128": ("complex128", False, "f64"), "complex64": ("complex64", False, "f32")}
TYPED = ["typed-float64", "float32", "complex128", "complex64"]

Spec = collections.namedtuple("Spec", "name dims d C p N elem scaling special comp seed")
INPUTS = []          # (spec, row of the bounds): every input of this module, for the seed search on the CPU

# first seed from 1 upwards whose reference satisfies the gap condition of every variant the input runs in; inputs not listed: 1
SEEDS = {"T9/p8/N45/float32": 3, "T9/p8/N45/complex64": 3}


def key_of(name, p, N, elem, scaling, special):
    return "/".join(str(x) for x in (name, f"p{p}", f"N{N}", elem, scaling, special) if x is not None)


def ids(specs):
    return [key_of(s.name, s.p, s.N, s.elem, s.scaling, s.special) for s in specs]


def spec(name, dims, d, C, p, N=45, variant="plain", elem=None, scaling=None, special=None, comp=None):
    elem = elem or VARIANTS[variant][0]
    if comp is not None:
        comp = comp[np.dtype(elem).kind == "c"]
    s = Spec(name, tuple(dims), d, C, p, N, elem, scaling, special, comp, SEEDS.get(key_of(name, p, N, elem, scaling, special), 1))
    INPUTS.append((s, VARIANTS[variant][2]))
    return s


@functools.lru_cache(maxsize=None)
def build(s):
    """The inputs of a case and their reference, computed once and shared (read-only) by every test that names the same spec."""
    dt = np.dtype(s.elem)
    cx = dt.kind == "c"
    big = np.complex128 if cx else np.float64
    T = len(s.dims) - 1
    scale = None
    if s.scaling == "a":                      # 4 left of the label, 1/4 right of it: both chains leave fp32, the overlaps stay
        scale = [4.0 if j < s.p else (0.25 if j > s.p else 1.0) for j in range(T)]
    elif s.scaling == "b":                    # 1/4 everywhere: overlaps ~ 2^-2T
        scale = [0.25] * T
    if s.comp is not None:                    # sites j with j % m < n are doubled: the long chain's own drift taken out (LONG)
        scale = [f * (2.0 if j % s.comp[0] < s.comp[1] else 1.0) for j, f in enumerate(scale)]
    rng = np.random.default_rng(s.seed)
    W = RR.ragged_chain(list(s.dims), s.d, s.C, s.p, cx, rng, scale)
    if s.special == "tie":                    # three overlaps of bit-equal magnitude
        W[s.p][..., 1] = -W[s.p][..., 0]
        W[s.p][..., 2] = W[s.p][..., 0]
    phi = random_states(s.N, T, s.d, cx, rng)
    W = [t.astype(dt).astype(big) for t in W]
    phi = phi.astype(dt).astype(big)
    if s.special == "absent":                 # class 1 of 3 has no series in set 1
        labels = np.sort(2 * (np.arange(s.N) % 2))
    else:
        labels = np.sort(np.arange(s.N) % s.C)
    y = RR.overlaps_ld(W, phi)
    phi0 = phi[::2]
    labels0 = np.sort(np.arange(len(phi0)) % s.C)
    for a in W + [phi, labels, labels0, y]:
        a.setflags(write=False)
    return types.SimpleNamespace(spec=s, W=W, phi=phi, labels=labels, ref=RR.readout_from(y, labels), phi0=phi0, labels0=labels0,
                                 ref0=RR.readout_from(y[::2], labels0), T=T)


def assert_gap(case, kind):
    gap = float(case.ref["gap"].min())
    assert gap > 100 * OV_BOUND[kind], f"{case.spec}: smallest gap {gap:.2e}: take another seed"


def engine_for(engine_cls, variant, monkeypatch):
    if VARIANTS[variant][1]:
        monkeypatch.setenv("MPST_TYPED", "1")           # the Float64 specialisation of the typed kernels
    else:
        monkeypatch.delenv("MPST_TYPED", raising=False)
    return engine_cls(0)


def load(eng, case, variant):
    s = case.spec
    dt = np.dtype(VARIANTS[variant][0])
    eng.set_options(chi_max=max(s.dims))
    eng.set_dataset(0, case.phi0.astype(dt), case.labels0, s.C)
    eng.set_dataset(1, case.phi.astype(dt), case.labels, s.C)
    eng.set_mps([t.astype(dt) for t in case.W], label_site=s.p)
    assert eng.info()["typed_kernels"] == (variant != "plain")


def loss_errors(mse, kld, ref):
    m, k = float(ref["mse_mean"]), float(ref["kld_mean"])
    return abs(mse - m) / max(1.0, abs(m)), abs(kld - k) / max(1.0, abs(k))


def check_readout(eng, case, variant, tag):
    """classify, eval and get_chi of a loaded engine on both data sets; returns the worst overlap and loss errors"""
    kind = VARIANTS[variant][2]
    worst = [0.0, 0.0]
    for which, ref in ((1, case.ref), (0, case.ref0)):
        pred, yh = eng.classify(which, return_overlaps=True)
        mse, kld, acc, conf = eng.eval(which)
        ymax = np.abs(ref["y"]).max()
        eo = float(np.abs(yh - ref["y"]).max() / ymax)
        em, ek = loss_errors(mse, kld, ref)
        wrong = int(np.count_nonzero(pred != ref["pred"]))
        print(f"readout {tag} {variant} {ids([case.spec])[0]}"
              f" set {which}: overlaps {eo:.2e} of {float(ymax):.3e}, mse {em:.2e}, kld {ek:.2e}, wrong predictions {wrong}")
        assert yh.shape == ref["y"].shape and eo < OV_BOUND[kind]
        assert np.isfinite(kld) and em < LOSS_BOUND[kind] and ek < LOSS_BOUND[kind]
        assert wrong == 0
        assert np.array_equal(eng.classify(which), pred)
        assert acc == ref["acc"] and np.array_equal(conf, ref["conf"]), (acc, ref["acc"], conf, ref["conf"])
        worst = [max(worst[0], eo), max(worst[1], em, ek)]
    chi, ls = eng.get_chi()
    assert chi.tolist() == list(case.spec.dims) and ls == case.spec.p
    return worst


def run_single(engine_cls, monkeypatch, s, variant, tag):
    case = build(s)
    assert_gap(case, VARIANTS[variant][2])
    eng = engine_for(engine_cls, variant, monkeypatch)
    try:
        load(eng, case, variant)
        return check_readout(eng, case, variant, tag)
    finally:
        eng.close()


# ---- the profiles ------------------------------------------------------------------------------------------------------------------
T2 = ("T2", [1, 3, 1], 3, 2)                                   # the shortest chain set_dataset accepts
T7 = ("T7", [1, 2, 3, 5, 17, 33, 9, 1], 3, 3)
T9 = ("T9", [1, 2, 4, 8, 16, 32, 64, 64, 2, 1], 2, 16)         # label tensor 64 x 2 x 2 on site 7, 16 x 2 x 32 on site 4
T3 = ("T3d16", [1, 8, 8, 1], 16, 1)
T4 = ("T4", [1, 4, 32, 4, 1], 4, 2)                            # d chi = 128
LONG = ("T200", [1, 2] + [4] * 197 + [2, 1], 2, 2)
# A Gaussian chain of this profile contracted with unit states drifts: 2^-124 ... 2^-126 over the 200 real sites, 2^-12 ... 2^-16 over
# the complex ones (measured on the reference).  Doubling the sites j with j % 8 < 5 (real: 125 sites) or j % 16 == 0 (complex: 13)
# takes the drift out, so that the overlaps are what the scalings (a) and (b) below make of numbers of order 0.1 ... 1.
LONG_COMP = ((8, 5), (16, 1))

# ---- group A: fp64 read-out --------------------------------------------------------------------------------------------------------
GROUP_A = ([spec(*T2, p) for p in (0, 1)] + [spec(*T7, p) for p in (0, 1, 3, 5, 6)] + [spec(*T7, 3, N=n) for n in (1, 15, 17, 300, 1030)]
           + [spec(*T9, p) for p in (0, 4, 7, 8)] + [spec(*T3, p) for p in (0, 1, 2)] + [spec(*T4, p) for p in (1, 2)])


@pytest.mark.parametrize("s", GROUP_A, ids=ids(GROUP_A))
def test_fp64_readout_at_every_label_site(engine_cls, monkeypatch, s):
    """k_env in both directions with the chainR ping-pong, k_eval_final with either side empty or both present, k_eval_reduce on one
    series, on partial tiles, on more than one block of k_eval_final (N = 300) and through its strided loop (N = 1030)."""
    run_single(engine_cls, monkeypatch, s, "plain", "A")


ABSENT = spec(*T7, 3, special="absent")


def test_fp64_readout_with_a_class_absent_from_the_test_set(engine_cls, monkeypatch):
    case = build(ABSENT)
    assert np.bincount(case.labels, minlength=3).tolist() == [23, 0, 22]
    run_single(engine_cls, monkeypatch, ABSENT, "plain", "A")
    assert not case.ref["conf"][1].any() and case.ref["conf"].sum() == 45         # what the engine's confusion counts were held to


# ---- group B: the typed read-out ---------------------------------------------------------------------------------------------------
GROUP_B = [(spec(*prof, p, variant=v), v) for prof in (T7, T9) for p in (0, (len(prof[1]) - 1) // 2, len(prof[1]) - 2) for v in TYPED]


@pytest.mark.parametrize("s,variant", GROUP_B, ids=[f"{v}-{i}" for (s, v), i in zip(GROUP_B, ids([s for s, _ in GROUP_B]))])
def test_typed_readout_at_the_ends_and_in_the_middle(engine_cls, monkeypatch, s, variant):
    """k_tenv from both ends, k_teval_final with Lc / Rc and their exponents, k_teval_reduce, in all four element types"""
    run_single(engine_cls, monkeypatch, s, variant, "B")


GROUP_B_LONG = [(spec(*LONG, p, N=17, variant=v, elem=e, scaling=sc, comp=LONG_COMP), v) for p in (0, 100, 199) for sc in ("a", "b")
                for v, e in (("float32", None), ("complex64", None), ("plain", "float32"))]


@pytest.mark.parametrize("s,variant", GROUP_B_LONG, ids=[f"{v}-{i}" for (s, v), i in zip(GROUP_B_LONG, ids([s for s, _ in GROUP_B_LONG]))])
def test_long_chain_exponents_come_from_both_sides(engine_cls, monkeypatch, s, variant):
    """T = 200: (a) sites left of the label times 4, right of it times 1/4: the left chain grows to 2^2p and the right one shrinks to
    2^-2(T-1-p), both outside fp32 at p = 100, where the overlaps stay of order 0.1 ... 1 (with the label on an end only one chain
    exists and the overlaps go with it); (b) every site times 1/4: every overlap is ~2^-400, whose square is still a normal double.
    fp32 and complex64 carry the power-of-two exponents of both chains into k_teval_final; the plain fp64 path on the fp32-rounded
    real input is the control."""
    case = build(s)
    lg = float(np.log2(np.abs(case.ref["y"]).max()))
    want = 2 * (s.p - (case.T - 1 - s.p)) if s.scaling == "a" else -2 * case.T
    print(f"readout B-long {ids([s])[0]}: largest overlap 2^{lg:.1f}, the scaling alone gives 2^{want}")
    assert abs(lg - want) < 8 and abs(2 * lg) < 1000, (lg, want)         # a property of the input: y^2 is a normal double
    run_single(engine_cls, monkeypatch, s, variant, "B-long")


# ---- group C: mpst_classify_batch --------------------------------------------------------------------------------------------------
def batch_case(tag, specs, engine_cls, monkeypatch):
    """one classify_batch call over the engines of ``specs`` (plain fp64): against the reference and against classify / eval of
    every engine (as test_gpu_tuning._check_scores)"""
    import mpstime_jl_amd as mt
    cases = [build(s) for s in specs]
    for c in cases:
        assert_gap(c, "f64")
    monkeypatch.delenv("MPST_TYPED", raising=False)
    engines = []
    try:
        for c in cases:
            e = engine_cls(0)
            engines.append(e)
            load(e, c, "plain")
        res = mt.classify_batch(engines, 1, return_overlaps=True)
        for r, e, c in zip(res, engines, cases):
            ref = c.ref
            ymax = np.abs(ref["y"]).max()
            eo = float(np.abs(r["yhat"] - ref["y"]).max() / ymax)
            em, ek = loss_errors(r["mse"], r["kld"], ref)
            wrong = int(np.count_nonzero(r["pred"] != ref["pred"]))
            print(f"readout {tag} classify_batch {ids([c.spec])[0]} dims {list(c.spec.dims)}: overlaps {eo:.2e} of {float(ymax):.3e}, mse {em:.2e}, "
                  f"kld {ek:.2e}, wrong predictions {wrong}")
            assert r["yhat"].shape == ref["y"].shape and eo < OV_BOUND["f64"] and em < LOSS_BOUND["f64"] and ek < LOSS_BOUND["f64"]
            assert wrong == 0 and r["acc"] == ref["acc"] and np.array_equal(r["conf"], ref["conf"])
            pred, yh = e.classify(1, return_overlaps=True)
            mse, kld, acc, conf = e.eval(1)
            assert np.array_equal(r["pred"], pred) and np.abs(r["yhat"] - yh).max() < 1e-11 * float(ymax)
            assert abs(r["mse"] - mse) <= 1e-10 * abs(mse) and abs(r["kld"] - kld) <= 1e-10 * abs(kld)
            assert r["acc"] == acc and np.array_equal(r["conf"], conf)
            chi, ls = e.get_chi()
            assert chi.tolist() == list(c.spec.dims) and ls == c.spec.p
    finally:
        for e in engines:
            e.close()


# K = 5 jobs that share T, d, C and differ in label site, set size and bond profile (Dout 1, 15, 16, 17, 33, 42: d cap <= 128 caps d = 3
# at 42); the grid is sized for N = 45, so the workgroups of the smaller sets return early
BATCH7 = [spec("B7j0", [1, 3, 9, 15, 16, 17, 3, 1], 3, 3, 0, N=1), spec("B7j1", [1, 1, 3, 9, 17, 33, 3, 1], 3, 3, 1, N=16),
          spec("B7j2", [1, 3, 9, 27, 33, 16, 3, 1], 3, 3, 3, N=17), spec("B7j3", [1, 2, 6, 16, 42, 15, 1, 1], 3, 3, 5, N=45),
          spec("B7j4", [1, 3, 5, 15, 17, 33, 9, 1], 3, 3, 6, N=33)]
# the widths of 48 and above need d = 2
BATCH9 = [spec("B9j0", [1, 2, 4, 8, 16, 48, 63, 64, 2, 1], 2, 3, 0, N=17), spec("B9j1", [1, 2, 4, 16, 48, 64, 63, 17, 2, 1], 2, 3, 4, N=45),
          spec("B9j2", [1, 2, 4, 8, 16, 33, 64, 48, 2, 1], 2, 3, 8, N=33)]
# k-step edges, the label in the middle of [1, D, D, D, D, 1]: both walks and the label-site product contract over Z = D d.
# D = 3: Z = 9, no multiple of 4, three k-steps (odd); D = 11: Z = 33, nine; D = 5: Z = 15, four (even); d = 4, D = 32: Z = 128
KSTEP3 = [spec(f"KsD{D}", [1, D, D, D, D, 1], 3, 2, 2, N=17) for D in (3, 11, 5)]
KSTEP128 = [spec("KsZ128", [1, 32, 32, 32, 32, 1], 4, 2, 2, N=17)]
# the full-size site tensor 64 x 2 x 64 (8192 entries: every thread's 32-entry share is live) on site 2: left of the label (p = 3),
# right of it (p = 1: the transposed park) and as the label tensor itself (p = 2, C = 2)
FULL = [spec("Full", [1, 2, 64, 64, 2, 1], 2, 2, p, N=17) for p in (3, 1, 2)]
# d = 16, capacity 8: all 256 threads stage site vectors; one class and sixteen
D16C1 = [spec("D16C1", [1, 8, 8, 1], 16, 1, p, N=17) for p in (0, 1, 2)]
D16C16 = [spec("D16C16", [1, 8, 8, 1], 16, 16, p, N=17) for p in (0, 1, 2)]
TWO = [spec(*T2, p, N=17) for p in (0, 1)]
LONG_BATCH = [spec(*LONG, p, N=17, scaling="a", comp=LONG_COMP) for p in (0, 100, 199)]
BATCHES = {"ragged-T7": BATCH7, "ragged-T9": BATCH9, "ksteps-d3": KSTEP3, "kstep-Z128": KSTEP128, "full-size-tensor": FULL, "d16-C1": D16C1,
           "d16-C16": D16C16, "two-sites": TWO, "T200-scaled": LONG_BATCH}


@pytest.mark.parametrize("name", list(BATCHES))
def test_classify_batch_at_every_label_site(engine_cls, monkeypatch, name):
    """k_score_walk_b: the right-hand walk (transposed park, the s Dp + a order of the Khatri-Rao rows), the hand-over of the left
    rows, the label-site dot with right-hand rows, either side empty; its column tiles, k-steps, odd-step tail and full-size tensor"""
    batch_case("C", BATCHES[name], engine_cls, monkeypatch)


# ---- group D: ties and signs -------------------------------------------------------------------------------------------------------
TIES = {v: spec(*T7, 3, variant=v, special="tie") for v in VARIANTS}


def assert_tied(case):
    mag = np.abs(case.ref["y"])
    assert np.array_equal(mag[:, 1], mag[:, 0]) and np.array_equal(mag[:, 2], mag[:, 0]) and mag.min() > 0
    assert np.array_equal(case.ref["y"][:, 1], -case.ref["y"][:, 0])
    assert not case.ref["pred"].any() and not case.ref["conf"][:, 1:].any()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ties_go_to_the_first_class(engine_cls, monkeypatch, variant):
    """Class slices W_1 = -W_0, W_2 = W_0: three overlaps of equal magnitude per series, every prediction is class 0 (the first
    largest), in eval and classify of every element type"""
    case = build(TIES[variant])
    assert_tied(case)
    eng = engine_for(engine_cls, variant, monkeypatch)
    try:
        load(eng, case, variant)
        check_readout(eng, case, variant, "D")
        for which, n in ((1, 45), (0, 23)):
            pred, yh = eng.classify(which, return_overlaps=True)
            assert not pred.any() and np.array_equal(np.abs(yh[:, 1]), np.abs(yh[:, 0])) and np.array_equal(yh[:, 2], yh[:, 0])
            conf = eng.eval(which)[3]
            assert not conf[:, 1:].any() and conf[:, 0].sum() == n
    finally:
        eng.close()


def test_ties_go_to_the_first_class_in_classify_batch(engine_cls, monkeypatch):
    import mpstime_jl_amd as mt
    case = build(TIES["plain"])
    assert_tied(case)
    monkeypatch.delenv("MPST_TYPED", raising=False)
    eng = engine_cls(0)
    try:
        load(eng, case, "plain")
        r = mt.classify_batch([eng], 1, return_overlaps=True)[0]
        eo = float(np.abs(r["yhat"] - case.ref["y"]).max() / np.abs(case.ref["y"]).max())
        print(f"readout D classify_batch ties: overlaps {eo:.2e}")
        assert eo < OV_BOUND["f64"]
        assert not r["pred"].any() and np.array_equal(r["yhat"][:, 1], -r["yhat"][:, 0]) and np.array_equal(r["yhat"][:, 2], r["yhat"][:, 0])
        assert np.array_equal(r["conf"], case.ref["conf"]) and r["acc"] == case.ref["acc"]
    finally:
        eng.close()


# ---- group E: mpst_normalize -------------------------------------------------------------------------------------------------------
NORM_SPECS = {(p, v): spec(*T7, p, variant=v) for p in (0, 3) for v in VARIANTS}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("p", [0, 3])
def test_normalize_with_the_label_off_the_last_site(engine_cls, monkeypatch, p, variant):
    """k_norm2 / k_tnorm2 with the class sum on site p, the scale kernels with the C-fold tensor there.  The norm afterwards is 1 to
    1e-12 (fp32 types 1e-5: tests/test_gpu_parity.py, tests/test_gpu_typed.py); every site tensor is the input times ONE scalar: to
    4 eps of the element type, relative to the tensor's largest entry (eps / 2 each for the rounded division on the device, for the
    scalar estimated here as a double and for the product with it in this check, 2 eps together with the estimate's own error;
    measured 0.9 ... 1.9 eps in the fp64 types, 0.3 ... 0.4 in the fp32 ones, where only the first term is of that size)."""
    s = NORM_SPECS[(p, variant)]
    case = build(s)
    elem, _, kind = VARIANTS[variant]
    big = np.complex128 if np.dtype(elem).kind == "c" else np.float64
    eng = engine_for(engine_cls, variant, monkeypatch)
    try:
        load(eng, case, variant)
        eng.normalize()
        Wn = [np.asarray(t).astype(big) for t in eng.get_mps()]
        chi, ls = eng.get_chi()
    finally:
        eng.close()
    assert chi.tolist() == list(s.dims) and ls == p
    assert [t.shape for t in Wn] == [t.shape for t in case.W]
    norm = (RC if big is np.complex128 else R).mps_norm(Wn)
    num = sum(float(np.real(np.vdot(a, b))) for a, b in zip(case.W, Wn))
    scalar = num / sum(float(np.real(np.vdot(a, a))) for a in case.W)
    want = R.mps_norm(case.W) ** (-1.0 / case.T)
    dev = max(float(np.abs(b - scalar * a).max() / np.abs(scalar * a).max()) for a, b in zip(case.W, Wn))
    eps = float(np.finfo(np.dtype(elem)).eps)
    print(f"readout E {variant} p = {p}: norm - 1 = {norm - 1.0:.2e}, scalar {scalar!r} (norm^(-1/T) = {want!r}), sites off by {dev:.2e} ({dev / eps:.2f} eps)")
    assert abs(norm - 1.0) < (1e-12 if kind == "f64" else 1e-5)
    assert dev <= 4 * eps
    assert abs(scalar - want) <= (1e-12 if kind == "f64" else 1e-5) * want
