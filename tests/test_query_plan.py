"""The query planner (csrc/mpst_query_plan.h) on the CPU: tests/query_plan_main.cpp, which includes nothing but that header, is
compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program.  Its figures must equal
tests/golden/query_plan.json field by field - recorded from the statements of impute_plan_order, impute_plan_chunk, run_marginal and
run_sitecond as they were before the planner was split out of mpst_api.hip - and satisfy the invariants the launches rely on, which
are checked independently of that file.  Every clamp of the arithmetic is the binding one in at least one case; the comments say where."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")

GB = 1 << 30
TILE = 16


def _imp(N, K=1, T=10, cap=4, zw=1, esz=8, maxm=1, ngrid=64, welems=0, cdf_inst=0, nq=0, u_trials=0, site_grid=0, dist=0, free=200 * GB,
         override="-"):
    return "i:" + ":".join(str(v) for v in (N, K, T, cap, zw, esz, maxm, ngrid, welems, cdf_inst, nq, u_trials, site_grid, dist, free, override))


def _sc(N, T=10, cap=4, d=4, zw=1, free=200 * GB, override="-"):
    return "s:" + ":".join(str(v) for v in (N, T, cap, d, zw, free, override))


def _mrg(N, welems=0, esz=8, free=200 * GB):
    return "m:%d:%d:%d:%d" % (N, welems, esz, free)


BIG = dict(maxm=100, cap=64)        # 3 277 824 bytes per instance; the default sizes come to 1152
# case -> instances per launch (None: the NOMEM verdict); the binding clamp in the comment
IMPUTE = {
    _imp(20000, **BIG): 12288,                              # budget = the 48 GB cap (15724 fit), rounded to 4096
    _imp(20000, free=10 * GB, **BIG): 1637,                 # budget = half of the free memory; below 4096: not rounded
    _imp(1000, override="1", **BIG): 327,                   # budget = the override
    _imp(2000, override="0"): 932,                          # override "0": the floor of 0.001 GB
    _imp(1): 1,                                             # N = 1
    _imp(100): 100,                                         # N below what fits: min(N, .)
    _imp(3, override="0", **BIG): 1,                        # one instance is larger than the budget: max(1, .)
    _imp(20000, override="0.01"): 8192,                     # 9320 fit; chunk < N: rounded to 4096 ...
    _imp(9000, override="0.01"): 9000,                      # ... chunk = N: not rounded
    _imp(5000, K=4, u_trials=3, override="0.01"): 1121,     # K > 1, uniforms from the caller: x_out, err_out and u come off the budget
    _imp(5000, K=4, override="0.01"): 1973,                 # K > 1, seeded: x_out and err_out only
    _imp(10, K=4, T=1000, u_trials=3, override="0"): 1,     # K > 1: the deduction clamps the budget to one instance
    _imp(20000, nq=3, override="0.01"): 4096,               # nq > 0: q_out comes off the budget (8192 without)
    _imp(2000, nq=16, T=1000, override="0"): 1,             # nq > 0: clamps the budget to one instance
    _imp(2000, site_grid=2560, override="0"): 914,          # a per-site table comes off the budget (932 without)
    _imp(2000, site_grid=1 << 20, override="0"): 1,         # a per-site table clamps the budget to one instance
    _imp(2000, cdf_inst=170, override="0"): 427,            # cdf rows are part of per_bytes
    _imp(3, dist=1, free=1 << 20, **BIG): None,             # dist: one instance exceeds 0.9 of the free memory: NOMEM
    _imp(3, dist=0, free=1 << 20, **BIG): 1,                # the same sizes without dist: no verdict
    _imp(1 << 21, K=1024, override="100000"): 1 << 20,      # the 2^30 / K cap
    _imp(20000, cap=128, welems=65536, free=10 * GB): 4096,  # welems > 0 is part of per_bytes (8179 fit)
    _imp(20000, zw=2, esz=4, free=10 * GB, **BIG): 1637,    # complex fp32: as many bytes as real fp64
}
ORDER = {
    "o:4:0:0:0010,1000,0000,0100": [1, 3, 0, 2],            # forwards; nothing missing: key T, last
    "o:4:1:0:0010,1000,0000,0100": [0, 3, 1, 2],            # backwards
    "o:4:0:0:0100,1000,0110,1001": [1, 3, 0, 2],            # ties keep the caller's order
    "o:4:0:1:0100,1000,0110,1001": [0, 1, 2, 3],            # the keep-caller-order switch
}
# case -> (instances per launch, walk workgroups, grid-phase workgroups)
SITECOND = {
    _sc(5): (5, 1, 50),                                                     # N below one tile; pairs < 4096
    _sc(2000, override="0"): (1488, 93, 4096),                              # 1491 fit: rounded down to whole tiles; pairs > 4096
    _sc(40, T=1000, cap=128, zw=2, override="0"): (16, 1, 4096),            # not one instance fits: the floor of one tile
    _sc(5000, T=1 << 20, override="1000"): (1024, 64, 4096),                # the 2^30 / T cap
    _sc(200000, T=100, cap=64, free=10 * GB): (97248, 6078, 4096),          # budget = half of the free memory (97259 fit)
    _sc(1000000, T=100, cap=64): (933680, 58355, 4096),                     # budget = the 48 GB cap (933688 fit)
}
MARGINAL = {
    _mrg(1000): 1000,                                       # welems = 0: one block
    _mrg(100000, welems=131072): 49152,                     # welems > 0, budget = the 48 GB cap
    _mrg(100000, welems=131072, free=10 * GB): 5120,        # welems > 0, budget = half of the free memory
    _mrg(100, welems=131072, free=1 << 20): 1,              # not one instance fits: max(1, .)
}
CDF = {"c:64:1": 64, "c:64:4": 17, "c:5:0": 0, "c:2:1": 2}
CASES = list(IMPUTE) + list(ORDER) + list(SITECOND) + list(MARGINAL) + list(CDF)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("query_plan") / "query_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "query_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + CASES, check=True, capture_output=True, text=True).stdout)
    assert doc["SITECOND_TILE"] == TILE
    return {c["case"]: c for c in doc["cases"]}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "query_plan.json")) as f:
        return {c["case"]: c for c in json.load(f)["cases"]}


def test_plans_equal_the_recorded_figures(plans, golden):
    assert set(plans) == set(CASES) and set(CASES) <= set(golden)
    for name in CASES:
        assert set(plans[name]) == set(golden[name]), name
        for field, ref in golden[name].items():
            assert plans[name][field] == ref, (name, field)


def test_binding_clamps(plans):
    for name, chunk in IMPUTE.items():
        assert plans[name]["nomem"] == (1 if chunk is None else 0), name
        assert plans[name].get("chunk") == chunk, name
    assert plans[_imp(100)]["per_bytes"] == 1152
    for name, order in ORDER.items():
        assert plans[name]["order"] == order, name
    for name, want in SITECOND.items():
        assert (plans[name]["chunk"], plans[name]["tiles"], plans[name]["grid_wgs"]) == want, name
    for name, chunk in MARGINAL.items():
        assert plans[name]["chunk"] == chunk, name
    for name, points in CDF.items():
        assert plans[name]["points"] == points, name


def _tiles_exactly(p, N):
    pos = 0
    for i0, count in p["blocks"]:
        assert i0 == pos and 0 < count <= p["chunk"]
        pos += count
    assert pos == N
    assert all(count == p["chunk"] for _, count in p["blocks"][:-1])


@pytest.mark.parametrize("name", [n for n, chunk in IMPUTE.items() if chunk is not None])
def test_imputation_block_invariants(plans, name):
    p, N, K = plans[name], int(name.split(":")[1]), int(name.split(":")[2])
    _tiles_exactly(p, N)
    assert p["chunk"] * K <= 1 << 30
    if p["chunk"] < N and p["chunk"] > 4096:
        assert p["chunk"] % 4096 == 0


@pytest.mark.parametrize("name", list(SITECOND))
def test_site_conditional_block_invariants(plans, name):
    p, N, T = plans[name], int(name.split(":")[1]), int(name.split(":")[2])
    _tiles_exactly(p, N)
    if p["chunk"] < N:
        assert p["chunk"] % TILE == 0 and p["chunk"] >= TILE
    assert p["tiles"] == -(-p["chunk"] // TILE)
    assert p["grid_wgs"] == max(1, min(p["chunk"] * T, 4096))


@pytest.mark.parametrize("name", list(MARGINAL))
def test_marginal_block_invariants(plans, name):
    _tiles_exactly(plans[name], int(name.split(":")[1]))


@pytest.mark.parametrize("name", list(ORDER))
def test_order_is_a_permutation(plans, name):
    order = plans[name]["order"]
    assert sorted(order) == list(range(len(order)))
