"""The host side of the segment marginals, without a GPU: the NumPy functions of mpstime.jl_amd/segments.py on hand-made lp arrays, and
the planner (csrc/mpst_segment_plan.h: segment_plan) through tests/segment_plan_main.cpp, which includes nothing but that header, is
compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program.  The planner's expected figures are
literals worked out by hand from the byte formula in the comment above the function -

    tables       (T + 1)(C + 1) * cap^2 zw * 8 + 2 (T + 1) C * 8   (+ (2 * 3 C + 5 walk_wgs) cap^2 zw * 8 on the big route)
    walk_wgs     min(N T, 4 compute units), on the big route min(N T, 2 compute units)
    per series   T max_width C * 8
    chunk        floor((budget - tables) / per series), in 1 .. min(N, floor((2^30 - 1) / (T max_width))); below N: whole tiles of 16, at
                 least one

with budget = min(48 GB, free / 2), or the override in GB with a floor of 0.001; tables beyond the budget are NOMEM."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from mpstime_jl_amd import prefix, segments

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")
GB = 1 << 30
NAN, INF = np.nan, np.inf


# ---- the NumPy functions ------------------------------------------------------------------------------------------------------------
def lp_of(p):
    """(N, T, max_width, 2) ln of the posteriors (p, 1 - p) of class 0 given as (N, T, max_width); NaN stays NaN"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.stack([p, 1.0 - p], axis=-1))


# two series, T = 3, max_width = 2: posteriors of class 0 at [start][width - 1]; start 2 has no width 2
P = [[[0.6, 0.9], [0.9, 0.7], [0.9, NAN]],          # 0.9 three times: the shortest (width 1) wins, then the earliest (start 1)
     [[0.2, 0.5], [0.5, 0.1], [0.4, NAN]]]          # class 1 peaks at (1, 2) with 0.9; class 0 at 0.5: (1, 1) before (0, 2)
LP = lp_of(P)


def test_the_triangle():
    assert segments.valid_triangle(3, 2).tolist() == [[True, True], [True, True], [True, False]]
    assert segments.valid_triangle(2, 2).tolist() == [[True, True], [True, False]]
    with pytest.raises(ValueError):
        segments.best_segment_from(LP[:, :, :1, :].reshape(2, 1, 3, 2))         # max_width > T
    with pytest.raises(ValueError):
        segments.accuracy_map_from(LP[0], np.zeros(3, dtype=int))


def test_posteriors_are_the_softmax_and_a_dead_row_is_nan():
    post = prefix.posteriors_from(LP + 7.0)                                     # a common factor per row cancels
    assert np.abs(post[0, 1, 0] - [0.9, 0.1]).max() <= 1e-15 and np.all(np.isnan(post[:, 2, 1]))
    dead = np.array(LP)
    dead[0, 0, 1] = -INF
    assert np.all(np.isnan(prefix.posteriors_from(dead)[0, 0, 1]))


def test_the_best_segment_and_its_tie_rules():
    b = segments.best_segment_from(LP, np.array([0, 1]))
    assert (b.start.tolist(), b.width.tolist()) == ([1, 1], [1, 2]) and np.abs(b.posterior - [0.9, 0.9]).max() <= 1e-15
    b = segments.best_segment_from(LP, np.array([0, 0]))
    assert (b.start[1], b.width[1]) == (1, 1) and abs(b.posterior[1] - 0.5) <= 1e-15
    # a value outside the triangle never wins, whatever it holds
    big = np.array(LP)
    big[:, 2, 1] = [0.0, -50.0]
    assert segments.best_segment_from(big, np.array([0, 1])).start.tolist() == [1, 1]
    # a dead row (-inf in every class) has no posterior and is skipped; a series of dead rows gives (0, 1, NaN)
    dead = np.array(LP)
    dead[0, 1, 0] = -INF
    dead[1] = -INF
    b = segments.best_segment_from(dead, np.array([0, 1]))
    assert (b.start[0], b.width[0]) == (2, 1) and (b.start[1], b.width[1]) == (0, 1) and np.isnan(b.posterior[1])
    with pytest.raises(ValueError):
        segments.best_segment_from(LP, np.array([0, 2]))


def test_y_given_against_y_inferred():
    # inferred: the arg-max class of the widest segment from the first site, lp[:, 0, max_width - 1]: class 0 (0.9) and class 0 (a tie at 0.5)
    assert segments.class_index_from(LP).tolist() == [0, 0]
    inferred, given = segments.best_segment_from(LP), segments.best_segment_from(LP, np.array([0, 0]))
    assert all(np.array_equal(a, b) for a, b in zip(inferred, given))
    other = segments.best_segment_from(LP, np.array([1, 1]))
    assert (other.start.tolist(), other.width.tolist()) == ([0, 1], [1, 2]) and np.abs(other.posterior - [0.4, 0.9]).max() <= 1e-15
    assert np.array_equal(segments.evidence_from(LP, None, 2), segments.evidence_from(LP, np.array([0, 0]), 2), equal_nan=True)


def test_the_evidence():
    ev = segments.evidence_from(LP, np.array([0, 1]), 1)
    assert ev.shape == (2, 3)
    want = np.log([[0.6 / 0.4, 9.0, 9.0], [0.8 / 0.2, 1.0, 0.6 / 0.4]])
    assert np.abs(ev - want).max() <= 1e-14
    ev2 = segments.evidence_from(LP, np.array([0, 1]), 2)
    assert np.all(np.isnan(ev2[:, 2])) and np.abs(ev2[:, :2] - np.log([[9.0, 0.7 / 0.3], [1.0, 9.0]])).max() <= 1e-14
    # three classes: the others are summed; a dead rival leaves the live one, a dead class of its own is -inf, both dead NaN
    with np.errstate(divide="ignore"):
        lp3 = np.log(np.array([[[[0.5, 0.25, 0.125]], [[0.5, 0.0, 0.25]]], [[[0.0, 0.5, 0.5]], [[0.0, 0.0, 0.0]]]]))   # (2, 2, 1, 3)
    ev3 = segments.evidence_from(lp3, np.array([0, 0]), 1)
    assert abs(ev3[0, 0] - np.log(0.5 / 0.375)) <= 1e-14 and abs(ev3[0, 1] - np.log(2.0)) <= 1e-14
    assert ev3[1, 0] == -INF and np.isnan(ev3[1, 1])
    assert segments.evidence_from(lp3[..., :1], np.array([0, 0]), 1)[0, 0] == INF          # one class: nothing to weigh it against
    with pytest.raises(ValueError):
        segments.evidence_from(LP, np.array([0, 1]), 3)


def test_the_accuracy_map():
    # arg-max per (series, start, width): series 0: class 0 everywhere; series 1: [[1, 0 (tie)], [0 (tie), 1], [1, -]]
    m = segments.accuracy_map_from(LP, np.array([0, 1]))
    assert np.array_equal(m, [[1.0, 0.5], [0.5, 1.0], [1.0, NAN]], equal_nan=True)
    m = segments.accuracy_map_from(LP, np.array([-1, 0]))                                   # an unknown label matches no class
    assert np.array_equal(m, [[0.0, 0.5], [0.5, 0.0], [0.0, NAN]], equal_nan=True)
    dead = np.array(LP)
    dead[1, 0, 0] = -INF                                                                    # an all -inf row predicts class 0
    assert segments.accuracy_map_from(dead, np.array([0, 0]))[0, 0] == 1.0
    empty = segments.accuracy_map_from(LP[:0], np.zeros(0, dtype=int))
    assert empty.shape == (3, 2) and np.all(np.isnan(empty))
    with pytest.raises(ValueError):
        segments.accuracy_map_from(LP, np.array([0]))


# ---- the planner --------------------------------------------------------------------------------------------------------------------
def _s(N=100, T=10, C=3, ls=9, cap=4, zw=1, mw=4, big=0, cus=8, free=200 * GB, override="-"):
    return "s:" + ":".join(str(v) for v in (N, T, C, ls, cap, zw, mw, big, cus, free, override))


CUT = dict(N=136, T=24, C=3, ls=23, mw=8, cus=256)      # tests/test_gpu_segments.py: test_blocks_do_not_change_the_result
BIGNUM = dict(N=1000, T=100, C=2, ls=50, cap=128, zw=2, mw=16, big=1, cus=256)
# case -> (tables, walk workgroups, table bytes, bytes per series, NOMEM, series per launch)
CASES = {
    # 11 * 4 = 44 tables wherever the label sits; a table is 4 * 4 * 8 = 128 bytes, the logs 2 * 11 * 3 * 8 = 528, a series brings
    # 10 * 4 * 3 * 8 = 960 bytes; 8 compute units keep 32 workgroups of the walk
    _s(ls=0): (44, 32, 44 * 128 + 528, 960, 0, 100),
    _s(ls=5): (44, 32, 44 * 128 + 528, 960, 0, 100),
    _s(ls=9): (44, 32, 44 * 128 + 528, 960, 0, 100),
    _s(N=1, T=1, C=1, ls=0, cap=1, mw=1): (4, 1, 4 * 8 + 32, 8, 0, 1),                      # one item: one workgroup
    # T = 100, chi = 32, C = 2, widths up to 16: 303 tables of 8192 bytes and 3232 of logs; 25 600 bytes per series; 1024 workgroups
    _s(N=256, T=100, C=2, ls=99, cap=32, mw=16, cus=256): (303, 1024, 303 * 8192 + 3232, 25600, 0, 256),
    # the override's floor of 1 073 741.8 bytes: 100 tables of 24 * 24 * 8 = 4608 and 1200 of logs are 462 000; 611 741 are left for
    # series of 24 * 8 * 3 * 8 = 4608: 132.7, eight whole tiles
    _s(cap=24, override="0.001", **CUT): (100, 1024, 462000, 4608, 0, 128),
    _s(cap=24, override="0", **CUT): (100, 1024, 462000, 4608, 0, 128),
    # cap = 36: 100 * 10 368 + 1200 = 1 038 000 fit, 35 741 are left: 7.7 series - below one tile: one tile
    _s(cap=36, override="0.001", **CUT): (100, 1024, 1038000, 4608, 0, 16),
    # cap = 40: 100 * 12 800 + 1200 = 1 281 200 do not fit: NOMEM, the tables are never cut
    _s(cap=40, override="0.001", **CUT): (100, 1024, 1281200, 4608, 1, 0),
    # ... and fit 0.002 GB = 2 147 483.6: 866 283 left / 4608 = 187.9, N = 136
    _s(cap=40, override="0.002", **CUT): (100, 1024, 1281200, 4608, 0, 136),
    # complex, big route on 4 compute units: 7 * 4 = 28 tables of 72 * 72 * 2 * 8 = 82 944, 336 of logs; 2 * 3 * 3 matrices of scratch
    # for the table kernels and 5 for each of the 8 workgroups of the walk: 58 more
    _s(N=40, T=6, C=3, ls=3, cap=72, zw=2, mw=6, big=1, cus=4): (28, 8, 86 * 82944 + 336, 864, 0, 40),
    _s(N=40, T=6, C=3, ls=3, cap=72, zw=2, mw=6, big=0, cus=4): (28, 16, 28 * 82944 + 336, 864, 0, 40),
    # the scratch is per RESIDENT workgroup: 512 of them at 5 * 128 * 128 * 2 * 8 = 1 310 720 bytes are 671 MB whatever N T is; with
    # the 303 tables, the 12 matrices of the table kernels and the logs 753 667 232 bytes: NOMEM under 0.5 GB, all 1000 series under 1 GB
    _s(override="0.5", **BIGNUM): (303, 512, (303 + 12 + 2560) * 262144 + 3232, 25600, 1, 0),
    _s(override="1", **BIGNUM): (303, 512, 753667232, 25600, 0, 1000),
    # half of the free memory: (5 368 709 120 - 2 485 408) / 25 600 = 209 618.1, whole tiles: 209 616
    _s(N=10 ** 7, T=100, C=2, ls=99, cap=32, mw=16, cus=256, free=10 * GB): (303, 1024, 2485408, 25600, 0, 209616),
    # entries of a block and class in 30 bits: floor((2^30 - 1) / 2^24) = 63, whole tiles: 48
    _s(N=5000, T=1 << 16, C=1, ls=0, cap=1, mw=1 << 8, cus=256, override="1000"): (131074, 1024, 131074 * 8 + 2 * 65537 * 8, (1 << 24) * 8, 0, 48),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("segment_plan") / "segment_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "segment_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + list(CASES), check=True, capture_output=True, text=True).stdout)
    assert (doc["SEGMENT_TILE"], doc["SEGMENT_BIG_MATS"], doc["SEGMENT_WGS_PER_CU"], doc["SEGMENT_BIG_WGS_PER_CU"]) == (16, 5, 4, 2)
    return {c["case"]: c for c in doc["cases"]}


def test_plan_figures(plans):
    assert set(plans) == set(CASES)
    for name, want in CASES.items():
        p = plans[name]
        got = (p["mats"], p["walk_wgs"], p["table_bytes"], p["per_bytes"], p["nomem"], 0 if p["nomem"] else p["chunk"])
        assert got == want, name


@pytest.mark.parametrize("name", list(CASES))
def test_plan_invariants(plans, name):
    p = plans[name]
    N, T, C = (int(x) for x in name.split(":")[1:4])
    assert p["slots_ok"] == 1 and p["mats"] == (T + 1) * (C + 1)
    if p["nomem"]:
        return
    assert p["covered"] == N and p["largest"] <= p["chunk"] and p["nblocks"] == -(-N // p["chunk"])
    assert p["ragged"] == 0                         # every block but the last is whole tiles
    assert p["chunk"] == N or p["chunk"] % 16 == 0
