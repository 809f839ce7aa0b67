"""The host side of the prefix marginals, without a GPU: the NumPy decision rule, accuracy curve and score differences of
mpstime.jl_amd/prefix.py on hand-made lp arrays, and the planner (csrc/mpst_prefix_plan.h: prefix_plan) through
tests/prefix_plan_main.cpp, which includes nothing but that header, is compiled with the host compiler under AddressSanitizer and UBSan
and run as a stand-alone program.  The planner's expected figures are literals worked out by hand from the byte formula in the comment
above the function -

    tables       ((label_site + 1) C + (T - label_site)) * cap^2 zw * 8 + (T + 1) C * 8   (+ 3 C cap^2 zw * 8 on the big route)
    per series   ((C + 1) cap zw + (T + 1) C) * 8
    chunk        floor((budget - tables) / per series), in 1 .. min(N, floor((2^30 - 1) / (T + 1))); below N: whole tiles of 16, at least one

with budget = min(48 GB, free / 2), or the override in GB with a floor of 0.001; tables beyond the budget are NOMEM."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from mpstime_jl_amd import prefix

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")
GB = 1 << 30


# ---- the NumPy functions ------------------------------------------------------------------------------------------------------------
def lp_from_posteriors(p):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(p, dtype=np.float64))


# three series, T = 3, two classes: posteriors of class 0 at t = 0 .. 3
LP = lp_from_posteriors([[[0.5, 0.5], [0.6, 0.4], [0.95, 0.05], [0.2, 0.8]],        # sure of class 0 at t = 2, changes its mind at T
                         [[0.5, 0.5], [0.5, 0.5], [0.3, 0.7], [0.1, 0.9]],          # a tie at t = 1; reaches 0.9 at T only
                         [[0.5, 0.5], [0.45, 0.55], [0.4, 0.6], [0.35, 0.65]]])     # never sure


def test_posteriors_are_the_softmax_and_a_dead_row_is_nan():
    post = prefix.posteriors_from(LP + 7.0)                                         # a common factor per row cancels
    assert np.abs(post[0, 2] - [0.95, 0.05]).max() <= 1e-15 and np.abs(post.sum(axis=2) - 1.0).max() <= 1e-15
    lp = np.array(LP)
    lp[1, 2] = -np.inf
    post = prefix.posteriors_from(lp)
    assert np.all(np.isnan(post[1, 2])) and not np.any(np.isnan(np.delete(post.reshape(-1, 2), 1 * 4 + 2, axis=0)))
    one_dead = np.array(LP)
    one_dead[0, 1, 1] = -np.inf
    assert np.array_equal(prefix.posteriors_from(one_dead)[0, 1], [1.0, 0.0])


def test_the_decision_rule():
    cls, length, post = prefix.early_decisions(LP, threshold=0.9)
    assert cls.tolist() == [0, 1, 1] and length.tolist() == [2, 3, 3]               # series 2: no prefix qualifies, the arg-max at T
    assert np.abs(post - [[0.95, 0.05], [0.1, 0.9], [0.35, 0.65]]).max() <= 1e-15
    # the threshold is met with equality, and t = 0 counts when min_length allows it
    cls, length, _ = prefix.early_decisions(LP, threshold=0.5, min_length=0)
    assert length.tolist() == [0, 0, 0] and cls.tolist() == [0, 0, 0]               # ties go to the lowest class index
    cls, length, _ = prefix.early_decisions(LP, threshold=0.5, min_length=1)
    assert length.tolist() == [1, 1, 1] and cls.tolist() == [0, 0, 1]
    cls, length, _ = prefix.early_decisions(LP, threshold=0.0, min_length=3)
    assert length.tolist() == [3, 3, 3] and cls.tolist() == [1, 1, 1]
    # never reached
    cls, length, _ = prefix.early_decisions(LP, threshold=2.0)
    assert length.tolist() == [3, 3, 3] and np.array_equal(cls, np.argmax(LP[:, 3], axis=1))


def test_a_nan_row_never_qualifies():
    lp = np.array(LP)
    lp[0, 2] = -np.inf                                                              # the posterior row at t = 2 is NaN
    cls, length, post = prefix.early_decisions(lp, threshold=0.7)
    assert length[0] == 3 and cls[0] == 1 and np.abs(post[0] - [0.2, 0.8]).max() <= 1e-15
    lp[0, 3] = -np.inf                                                              # ... and at T: the arg-max of an all -inf row is class 0
    cls, length, post = prefix.early_decisions(lp, threshold=0.7)
    assert length[0] == 3 and cls[0] == 0 and np.all(np.isnan(post[0]))
    assert (cls[1:].tolist(), length[1:].tolist()) == ([1, 1], [2, 3])


def test_min_length_outside_the_series_is_an_error():
    with pytest.raises(ValueError):
        prefix.early_decisions(LP, min_length=4)
    with pytest.raises(ValueError):
        prefix.early_decisions(LP, min_length=-1)
    with pytest.raises(ValueError):
        prefix.early_decisions(LP[0])


def test_the_accuracy_curve():
    # arg-max per (series, t): [[0, 0, 0, 1], [0, 0, 1, 1], [0, 1, 1, 1]] (ties: class 0)
    assert np.array_equal(prefix.accuracy_curve_from(LP, np.array([1, 1, 1])), [0.0, 1 / 3, 2 / 3, 1.0])
    assert np.array_equal(prefix.accuracy_curve_from(LP, np.array([0, 1, -1])), [1 / 3, 1 / 3, 2 / 3, 1 / 3])
    assert np.all(np.isnan(prefix.accuracy_curve_from(LP[:0], np.zeros(0, dtype=int))))
    with pytest.raises(ValueError):
        prefix.accuracy_curve_from(LP, np.array([0, 1]))


def test_the_score_differences():
    lp = lp_from_posteriors([[[0.5, 0.25], [0.25, 0.125], [0.125, 0.125]],
                             [[0.5, 0.25], [0.5, 0.0625], [0.0, 0.03125]]])          # (2, T + 1 = 3, 2); the last class-0 entry is -inf
    s = prefix.causal_scores_from(lp, np.array([0, 1]))
    assert np.allclose(s, [[np.log(2), np.log(2)], [np.log(4), np.log(2)]], rtol=0, atol=1e-15)
    assert np.allclose(s.sum(axis=1), [lp[0, 0, 0] - lp[0, 2, 0], lp[1, 0, 1] - lp[1, 2, 1]], rtol=0, atol=1e-15)
    s = prefix.causal_scores_from(lp, np.array([0, 0]))
    assert s[1, 0] == 0.0 and s[1, 1] == np.inf                                     # the later prefix has zero likelihood
    mix = prefix.causal_scores_from(lp)                                             # ln(sum_c l_c(t)) - ln(sum_c l_c(t + 1))
    want = np.log([[0.75 / 0.375, 0.375 / 0.25], [0.75 / 0.5625, 0.5625 / 0.03125]])
    assert np.allclose(mix, want, rtol=0, atol=1e-15)
    dead = np.full((1, 3, 2), -np.inf)
    assert np.all(np.isnan(prefix.causal_scores_from(dead))) and np.all(np.isnan(prefix.causal_scores_from(dead, np.array([1]))))
    with pytest.raises(ValueError):
        prefix.causal_scores_from(lp, np.array([0, 2]))


# ---- the planner --------------------------------------------------------------------------------------------------------------------
def _p(N=100, T=10, C=3, ls=9, cap=4, zw=1, big=0, free=200 * GB, override="-"):
    return "p:" + ":".join(str(v) for v in (N, T, C, ls, cap, zw, big, free, override))


CUT = dict(N=136, T=64, C=3, ls=63)         # tests/test_gpu_prefix.py: test_blocks_do_not_change_the_result
# case -> (tables, table bytes, bytes per series, NOMEM, series per launch, tiles)
CASES = {
    # a table is 4 * 4 * 8 = 128 bytes, the logs 11 * 3 * 8 = 264, a series (4 * 4 + 33) * 8 = 392; everything fits: min(N, .)
    _p(ls=0): (13, 13 * 128 + 264, 392, 0, 100, 7),                                 # label first: 1 * 3 + 10 tables
    _p(ls=5): (23, 23 * 128 + 264, 392, 0, 100, 7),                                 # middle: 6 * 3 + 5
    _p(ls=9): (31, 31 * 128 + 264, 392, 0, 100, 7),                                 # last: 10 * 3 + 1
    _p(N=1, T=1, C=1, ls=0, cap=1): (2, 2 * 8 + 16, (2 + 2) * 8, 0, 1, 1),
    # the override's floor of 1 073 741.8 bytes: 193 tables of 24 * 24 * 8 = 4608 and 1560 of logs are 890 904; 182 837 are left for
    # series of (4 * 24 + 195) * 8 = 2328: 78.5, four whole tiles
    _p(cap=24, override="0.001", **CUT): (193, 890904, 2328, 0, 64, 4),
    _p(cap=24, override="0", **CUT): (193, 890904, 2328, 0, 64, 4),
    # cap = 26: 193 * 5408 + 1560 = 1 045 304 fit, 28 437 are left for series of 2392: 11.9 - below one tile: one tile
    _p(cap=26, override="0.001", **CUT): (193, 1045304, 2392, 0, 16, 1),
    # cap = 32: 193 * 8192 + 1560 = 1 582 616 do not fit: NOMEM, not a cut over t
    _p(cap=32, override="0.001", **CUT): (193, 1582616, (4 * 32 + 195) * 8, 1, 0, 0),
    # ... and fit 0.002 GB = 2 147 483.6: 564 867 left / 2584 = 218.6, N = 136
    _p(cap=32, override="0.002", **CUT): (193, 1582616, 2584, 0, 136, 9),
    # complex, big route: 4 * 3 + 3 = 15 tables of 72 * 72 * 2 * 8 = 82 944, 168 of logs, 3 * 3 more matrices of scratch
    _p(N=40, T=6, C=3, ls=3, cap=72, zw=2, big=1): (15, 15 * 82944 + 168 + 9 * 82944, (4 * 72 * 2 + 21) * 8, 0, 40, 3),
    _p(N=40, T=6, C=3, ls=3, cap=72, zw=2, big=0): (15, 15 * 82944 + 168, 4776, 0, 40, 3),
    # half of the free memory: (5 368 709 120 - 1 648 208) / 2384 = 2 251 283.9, whole tiles: 140 705 of them
    _p(N=10 ** 7, T=100, C=2, ls=99, cap=32, free=10 * GB): (201, 201 * 8192 + 1616, 2384, 0, 2251280, 140705),
    # (series, prefix) pairs in 30 bits: floor((2^30 - 1) / (2^20 + 1)) = 1023, whole tiles: 1008
    _p(N=5000, T=1 << 20, C=1, ls=0, cap=1, override="1000"): ((1 << 20) + 1, 2 * ((1 << 20) + 1) * 8, ((1 << 20) + 3) * 8, 0, 1008, 63),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("prefix_plan") / "prefix_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "prefix_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + list(CASES), check=True, capture_output=True, text=True).stdout)
    assert (doc["PREFIX_TILE"], doc["PREFIX_ENV_BIG_MATS"]) == (16, 3)
    return {c["case"]: c for c in doc["cases"]}


def test_plan_figures(plans):
    assert set(plans) == set(CASES)
    for name, want in CASES.items():
        p = plans[name]
        got = (p["mats"], p["table_bytes"], p["per_bytes"], p["nomem"]) + ((p["chunk"], p["tiles"]) if not p["nomem"] else (0, 0))
        assert got == want, name


@pytest.mark.parametrize("name", list(CASES))
def test_plan_invariants(plans, name):
    p = plans[name]
    N, T, C, ls = (int(x) for x in name.split(":")[1:5])
    assert p["slots_ok"] == 1 and p["mats"] == (ls + 1) * C + (T - ls)
    if p["nomem"]:
        return
    assert p["covered"] == N and p["largest"] <= p["chunk"] and p["nblocks"] == -(-N // p["chunk"])
    assert p["ragged"] == 0                         # every block but the last is whole tiles
    assert p["tiles"] == -(-p["chunk"] // 16) and (p["chunk"] == N or p["chunk"] % 16 == 0)
