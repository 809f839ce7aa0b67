"""The planner of the window conditionals (csrc/mpst_query_plan.h: window_plan_block) on the CPU: tests/window_plan_main.cpp, which
includes nothing but that header, is compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program.
The expected figures below are literals worked out by hand from the byte formula in the comment above the function -

    per instance    T * (2 * cap * zw + max_width) * 8
    per workgroup   4 * cap * cap * zw * 8                      (big route only)
    chunk   = floor((big ? 3/4 : 1) * budget / per instance), in 1 .. min(N, floor(2^30 / T)); below N: whole tiles of 16, at least one
    win_wgs = min(chunk * T, 4096); big route: also <= 1024 and <= floor(budget / 4 / per workgroup); at least 1

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
TILE = 16


def _w(N, T=10, cap=4, zw=1, mw=4, big=0, free=200 * GB, override="-"):
    return "w:" + ":".join(str(v) for v in (N, T, cap, zw, mw, big, free, override))


LONG = dict(T=100, cap=64, mw=16)               # 100 * (128 + 16) * 8 = 115 200 bytes per instance; the default sizes come to 960
HUGE = dict(T=8, cap=128, zw=2, mw=4, big=1)    # 8 * (512 + 4) * 8 = 33 024 per instance, 4 * 128 * 128 * 2 * 8 = 1 048 576 per workgroup
# case -> (instances per launch, walk workgroups, window workgroups)
CASES = {
    _w(5): (5, 1, 50),                                          # N below one tile: min(N, .); 50 pairs < 4096
    _w(1): (1, 1, 10),
    _w(2000, override="0"): (1104, 69, 4096),                   # the override's floor, 1 073 741.8 / 960 = 1118.5: whole tiles, 69 * 16
    _w(40, T=1000, cap=128, zw=2, mw=16, override="0"): (16, 1, 4096),      # 4 224 000 bytes: not one instance fits, the floor of one tile
    _w(5000, T=1 << 20, override="1000"): (1024, 64, 4096),     # 10 666 fit, N = 5000, the 2^30 / T cap: 1024
    _w(200000, free=10 * GB, **LONG): (46592, 2912, 4096),      # half of the free memory: 5 368 709 120 / 115 200 = 46 603.4 -> 2912 tiles
    _w(1000000, **LONG): (447392, 27962, 4096),                 # the 48 GB cap: 51 539 607 552 / 115 200 = 447 392.4, whole tiles as it is
    _w(1000, override="0.01", **LONG): (80, 5, 4096),           # the override: 10 737 418.2 / 115 200 = 93.2 -> 5 tiles
    _w(100, override="0.01", **HUGE): (100, 7, 2),              # big route: 0.75 * 10 737 418.2 / 33 024 = 243.9 >= N; scratch: 2 684 354.6 / 1 048 576 = 2.6
    _w(100, override="0", **HUGE): (16, 1, 1),                  # big route: 805 306.4 / 33 024 = 24.4 -> one tile; not one workgroup's scratch fits: 1
    _w(100000, T=100, cap=128, mw=16, big=1, free=10 * GB): (18496, 1156, 1024),   # the 3/4 share: 4 026 531 840 / 217 600 = 18 504.3 (24 672 without); 2560 workgroups' scratch fit: the cap of 1024
    _w(100000, T=100, cap=128, mw=16, big=0, free=10 * GB): (24672, 1542, 4096),   # the same sizes on the LDS route: the whole budget, 24 672.3
    _w(3, big=1, **{k: v for k, v in HUGE.items() if k != "big"}): (3, 1, 24),      # big route, everything fits: the pairs themselves
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("window_plan") / "window_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "window_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + list(CASES), check=True, capture_output=True, text=True).stdout)
    assert (doc["SITECOND_TILE"], doc["WINDOW_BIG_MATS"], doc["WINDOW_MAX_WORKGROUPS"], doc["WINDOW_MAX_BIG_WORKGROUPS"]) == (TILE, 4, 4096, 1024)
    return {c["case"]: c for c in doc["cases"]}


def test_binding_clamps(plans):
    assert set(plans) == set(CASES)
    for name, want in CASES.items():
        assert (plans[name]["chunk"], plans[name]["tiles"], plans[name]["win_wgs"]) == want, name


@pytest.mark.parametrize("name", list(CASES))
def test_block_invariants(plans, name):
    p, N, T, big = plans[name], int(name.split(":")[1]), int(name.split(":")[2]), int(name.split(":")[6])
    pos = 0
    for i0, count in p["blocks"]:
        assert i0 == pos and 0 < count <= p["chunk"]
        pos += count
    assert pos == N and all(count == p["chunk"] for _, count in p["blocks"][:-1])
    assert 1 <= p["chunk"] <= N or p["chunk"] == TILE
    if p["chunk"] < N:
        assert p["chunk"] % TILE == 0 and p["chunk"] >= TILE
    assert p["chunk"] * T < 1 << 31
    assert p["tiles"] == -(-p["chunk"] // TILE)
    assert 1 <= p["win_wgs"] <= min(p["chunk"] * T, 1024 if big else 4096)
