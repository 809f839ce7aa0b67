"""The planner of the marginal site conditionals (csrc/mpst_query_plan.h: margcond_plan_block) on the CPU: tests/margcond_plan_main.cpp,
which includes nothing but that header, is compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone
program.  The expected figures below are literals worked out by hand from the byte formula in the comment above the function -

    per instance    T * (cap * cap * zw + d * d * zw + outputs) * 8  (+ 5 * cap * cap * zw * 8 on the big route)
    chunk    = floor(budget / per instance), in 1 .. min(N, floor((2^30 - 1) / T)); whole instances, no rounding
    grid_wgs = min(chunk * T, 4096)

with budget = min(48 GB, free / 2), or the override in GB with a floor of 0.001 - and every clamp is the binding one in at least one
case; the comments say where and show the sum."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")

GB = 1 << 30


def _m(N, T=10, cap=4, d=2, zw=1, outputs=5, big=0, free=200 * GB, override="-"):
    return "m:" + ":".join(str(v) for v in (N, T, cap, d, zw, outputs, big, free, override))


LONG = dict(T=100, cap=64, d=4, outputs=7)              # 100 * (4096 + 16 + 7) * 8 = 3 295 200 bytes per instance; the defaults come to 2000
HUGE = dict(T=8, cap=128, d=4, zw=2, outputs=2)         # 8 * (32 768 + 32 + 2) * 8 = 2 099 328; big route: + 5 * 32 768 * 8 = 3 410 048
# case -> (instances per launch, grid workgroups, bytes per instance)
CASES = {
    _m(5): (5, 50, 2000),                                               # everything fits: min(N, .); 50 pairs < 4096
    _m(1): (1, 10, 2000),
    _m(3, zw=2, outputs=1): (3, 30, 3280),                              # complex: 10 * (32 + 8 + 1) * 8
    _m(2000, override="0"): (536, 4096, 2000),                          # the override's floor, 1 073 741.8 / 2000 = 536.9; 5360 pairs: the 4096 cap
    _m(40, T=1000, cap=128, d=4, zw=2, outputs=6, override="0"): (1, 1000, 262448000),     # not one instance fits: the floor of one
    _m(5000, T=1 << 20, override="1000"): (1023, 4096, 209715200),      # 5120 fit, N = 5000, chunk * T < 2^30: floor((2^30 - 1) / 2^20) = 1023
    _m(200000, free=10 * GB, **LONG): (1629, 4096, 3295200),            # half of the free memory: 5 368 709 120 / 3 295 200 = 1629.3
    _m(1000000, **LONG): (15640, 4096, 3295200),                        # the 48 GB cap: 51 539 607 552 / 3 295 200 = 15 640.8
    _m(1000, override="0.01", **LONG): (3, 300, 3295200),               # the override: 10 737 418.2 / 3 295 200 = 3.3; 300 pairs
    _m(100, override="0.01", big=1, **HUGE): (3, 24, 3410048),          # big route: the workgroup's five matrices count, 3.1
    _m(100, override="0.01", big=0, **HUGE): (5, 40, 2099328),          # the same sizes on the LDS route: 5.1
    _m(100, override="0", big=1, **HUGE): (1, 8, 3410048),              # big route, not one instance fits
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("margcond_plan") / "margcond_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "margcond_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + list(CASES), check=True, capture_output=True, text=True).stdout)
    assert (doc["MARGCOND_BIG_MATS"], doc["MARGCOND_MAX_GRID_WORKGROUPS"]) == (5, 4096)
    return {c["case"]: c for c in doc["cases"]}


def test_binding_clamps(plans):
    assert set(plans) == set(CASES)
    for name, want in CASES.items():
        assert (plans[name]["chunk"], plans[name]["grid_wgs"], plans[name]["per_bytes"]) == want, name


@pytest.mark.parametrize("name", list(CASES))
def test_block_invariants(plans, name):
    p, N, T = plans[name], int(name.split(":")[1]), int(name.split(":")[2])
    assert p["covered"] == N and p["largest"] <= p["chunk"] and p["nblocks"] == -(-N // p["chunk"])
    assert 1 <= p["chunk"] <= N
    assert p["chunk"] * T < 1 << 30
    assert 1 <= p["grid_wgs"] <= min(p["chunk"] * T, 4096)
