"""The planner of the observed conditionals (csrc/mpst_observed_plan.h: observed_plan_block) on the CPU: tests/observed_plan_main.cpp,
which includes nothing but that header, is compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone
program.  The expected figures below are literals worked out by hand from the byte formula in the comment above the function -

    per instance    (T * (cap * cap * zw + 2 * d * d * zw + outputs) + 1) * 8  (+ 5 * cap * cap * zw * 8 on the big route)
                    the storage of the marginal conditionals, the operator of every site (the second d * d * zw) and logev (the 1)
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


def _o(N, T=10, cap=4, d=2, zw=1, outputs=5, big=0, free=200 * GB, override="-"):
    return "o:" + ":".join(str(v) for v in (N, T, cap, d, zw, outputs, big, free, override))


LONG = dict(T=100, cap=64, d=4, outputs=7)              # (100 * (4096 + 32 + 7) + 1) * 8 = 3 308 008 bytes per instance; the defaults: (10 * 29 + 1) * 8 = 2328
HUGE = dict(T=8, cap=128, d=4, zw=2, outputs=2)         # (8 * (32 768 + 64 + 2) + 1) * 8 = 2 101 384; big route: + 5 * 32 768 * 8 = 3 412 104
# case -> (instances per launch, grid workgroups, bytes per instance)
CASES = {
    _o(5): (5, 50, 2328),                                               # everything fits: min(N, .); 50 pairs < 4096
    _o(1): (1, 10, 2328),
    _o(3, zw=2, outputs=1): (3, 30, 3928),                              # complex: (10 * (32 + 16 + 1) + 1) * 8
    _o(2000, override="0"): (461, 4096, 2328),                          # the override's floor, 1 073 741.8 / 2328 = 461.2; 4610 pairs: the 4096 cap
    _o(40, T=1000, cap=128, d=4, zw=2, outputs=6, override="0"): (1, 1000, 262704008),     # not one instance fits: the floor of one
    _o(5000, T=1 << 20, override="2000"): (1023, 4096, 243269640),      # 8827 fit, N = 5000, chunk * T < 2^30: floor((2^30 - 1) / 2^20) = 1023
    _o(200000, free=10 * GB, **LONG): (1622, 4096, 3308008),            # half of the free memory: 5 368 709 120 / 3 308 008 = 1622.9
    _o(1000000, **LONG): (15580, 4096, 3308008),                        # the 48 GB cap: 51 539 607 552 / 3 308 008 = 15 580.3
    _o(1000, override="0.01", **LONG): (3, 300, 3308008),               # the override: 10 737 418.2 / 3 308 008 = 3.2; 300 pairs
    _o(100, override="0.01", big=1, **HUGE): (3, 24, 3412104),          # big route: the workgroup's five matrices count, 3.1
    _o(100, override="0.01", big=0, **HUGE): (5, 40, 2101384),          # the same sizes on the LDS route: 5.1
    _o(100, override="0", big=1, **HUGE): (1, 8, 3412104),              # big route, not one instance fits
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("observed_plan") / "observed_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "observed_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + list(CASES), check=True, capture_output=True, text=True).stdout)
    assert (doc["MARGCOND_BIG_MATS"], doc["OBSERVED_MAX_GRID_WORKGROUPS"]) == (5, 4096)
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
