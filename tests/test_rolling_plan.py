"""The planner of the rolling-origin forecasts (csrc/mpst_rolling_plan.h: rolling_plan) without a GPU, through
tests/rolling_plan_main.cpp, which includes nothing but that header, is compiled with the host compiler under AddressSanitizer and
UBSan and run as a stand-alone program.  The expected figures are literals worked out by hand from the byte formula in the comment
above the function, with mat = cap^2 zw * 8 and pairs = d (d + 1) / 2 -

    fixed        prefix tables * mat + (T + 1) C * 8  (+ 3 C mat on the big route)  + table_wgs * mat,  table_wgs = min(1024, T C pairs)
    per target   H C pairs * mat
    per series   (T C (cap zw + 1) + T H (d^2 zw + outputs)) * 8
    tblock       floor((budget - fixed) / 2 / per target) in 1 .. T
    chunk        floor((budget - fixed - tblock * per target) / per series) in 1 .. min(N, floor((2^30 - 1) / (T H))); below N: whole
                 tiles of 16, at least one
    grid_wgs     min(chunk T H, 4096)

with budget = min(48 GB, free / 2), or the override in GB with a floor of 0.001; `fixed` beyond the budget is NOMEM."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")
GB = 1 << 30


def _r(N, T, C, ls, cap, d, zw, H, outputs, big=0, free=200 * GB, override="-"):
    return "r:" + ":".join(str(v) for v in (N, T, C, ls, cap, d, zw, H, outputs, big, free, override))


TIMING = dict(N=256, T=100, C=2, ls=99, cap=32, d=4, zw=1, H=16, outputs=8)
CUT = dict(N=40, T=9, C=2, ls=8, cap=16, d=4, zw=1, H=9, outputs=8)         # tests/test_gpu_rolling.py: the forced blocks
BIG = dict(N=5, T=6, C=2, ls=2, cap=72, d=4, zw=2, H=3, outputs=8, big=1)
# case -> (fixed bytes, bytes per target, bytes per series, table workgroups, NOMEM, targets per block, series per block, grid workgroups,
#          blocks of targets)
CASES = {
    # one block of targets.  mat = 8192, 10 pairs, 1024 of the 2000 chains resident; 201 prefix tables and 1616 bytes of logs:
    # 1225 * 8192 + 1616; a target keeps 16 * 2 * 10 = 320 matrices; a series (100 * 2 * 33 + 1600 * 24) * 8
    _r(**TIMING): (10036816, 2621440, 360000, 1024, 0, 100, 256, 4096, 1),
    # several: 0.25 GB = 268 435 456; 258 398 640 left, half of it / 2 621 440 = 49.3; 129 948 080 remain / 360 000 = 360.9: all 256
    _r(override="0.25", **TIMING): (10036816, 2621440, 360000, 1024, 0, 49, 256, 4096, 3),
    # H = 1.  mat = 392, 180 chains; 15 prefix tables (label at 4 of 9): 195 * 392 + 160; a target 20 matrices; a series
    # (9 * 2 * 8 + 9 * 17) * 8
    _r(40, 9, 2, 4, 7, 4, 1, 1, 1): (76600, 7840, 2376, 180, 0, 9, 40, 360, 1),
    # H = T, complex.  mat = 2304, 6 pairs, 180 chains; 31 prefix tables: 211 * 2304 + 264; a target 180 matrices; a series
    # (10 * 3 * 25 + 100 * 26) * 8
    _r(17, 10, 3, 9, 12, 3, 2, 10, 8): (486408, 414720, 26800, 180, 0, 10, 17, 1700, 1),
    # the big route.  mat = 82 944, 120 chains; 10 prefix tables, 2 * 3 matrices of the environment kernel's scratch: 136 * 82 944 + 112;
    # a target 60 matrices; a series (6 * 2 * 145 + 18 * 40) * 8
    _r(**BIG): (11280496, 4976640, 19680, 120, 0, 6, 5, 90, 1),
    # NOMEM: 0.01 GB = 10 737 418 bytes do not hold them
    _r(override="0.01", **BIG): (11280496, 4976640, 19680, 120, 1, 0, 0, 0, 0),
    # the chunk override at its floor of 1 073 741.8 bytes.  mat = 2048; 19 prefix tables: 199 * 2048 + 160 = 407 712; a target
    # 9 * 20 * 2048 = 368 640 is more than half of the 666 029 left: one target per block; 297 389 remain for series of
    # (9 * 2 * 17 + 81 * 24) * 8 = 18 000: 16.5 - one tile
    _r(override="0.001", **CUT): (407712, 368640, 18000, 180, 0, 1, 16, 1296, 9),
    # ... 0.004 GB = 4 294 967: 3 887 255 left, half / 368 640 = 5.3: two blocks of targets; 2 044 055 remain: all 40 series
    _r(override="0.004", **CUT): (407712, 368640, 18000, 180, 0, 5, 40, 3240, 2),
    # triples of a block in 30 bits: floor((2^30 - 1) / (2^12 * 2^8)) = 1023, whole tiles: 1008
    _r(5000, 1 << 12, 1, 0, 1, 1, 1, 1 << 8, 1, override="1000"): (4097 * 8 + 4097 * 8 + 1024 * 8, 256 * 8, (4096 * 2 + (1 << 20) * 2) * 8, 1024, 0,
                                                                   4096, 1008, 4096, 1),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rolling_plan") / "rolling_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "rolling_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + list(CASES), check=True, capture_output=True, text=True).stdout)
    assert (doc["ROLLING_TILE"], doc["ROLLING_MAX_TABLE_WORKGROUPS"], doc["ROLLING_MAX_GRID_WORKGROUPS"]) == (16, 1024, 4096)
    return {c["case"]: c for c in doc["cases"]}


def test_plan_figures(plans):
    assert set(plans) == set(CASES)
    for name, want in CASES.items():
        p = plans[name]
        got = (p["fixed_bytes"], p["target_bytes"], p["per_bytes"], p["table_wgs"], p["nomem"]) + \
              ((0, 0, 0, 0) if p["nomem"] else (p["tblock"], p["chunk"], p["grid_wgs"], p["tblocks"]))
        assert got == want, name


@pytest.mark.parametrize("name", list(CASES))
def test_plan_invariants(plans, name):
    p = plans[name]
    N, T = (int(x) for x in name.split(":")[1:3])
    assert p["pairs_ok"] == 1
    if p["nomem"]:
        return
    assert p["covered"] == N and p["largest"] <= p["chunk"] and p["nblocks"] == -(-N // p["chunk"])
    assert p["ragged"] == 0 and (p["chunk"] == N or p["chunk"] % 16 == 0)
    assert p["tcovered"] == T and 1 <= p["tblock"] <= T and p["tblocks"] == -(-T // p["tblock"])
