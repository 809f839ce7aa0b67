"""The model overlaps plan (csrc/mpst_overlap_plan.h) on the CPU: tests/overlap_plan_main.cpp, which includes nothing but that header
(and through it the query budget of mpst_query_plan.h), compiled with the host compiler and run as a stand-alone program: the padded
sizes and the route, the pair order (most expensive first, ties in the caller's order) and the blocks, which respect the budget."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")
GB = 1 << 30


def size_case(d, cap, planes=1, cmax=2, P=6, free=200 * GB, override="-"):
    return "v:" + ":".join(str(v) for v in (d, cap, planes, cmax, P, free, override))


def order_case(T, d, p, chis, ncls):
    return "o:%d:%d:%d:%s:%s" % (T, d, p, "/".join(",".join(map(str, c)) for c in chis), ",".join(map(str, ncls)))


HEAD = dict(d=4, cap=32)                # the headline model
SCRATCH = dict(d=6, cap=72)             # the global-scratch case of tests/test_gpu_overlap.py
SHAPES = [HEAD, SCRATCH, dict(d=6, cap=12), dict(d=5, cap=20), dict(d=3, cap=8), dict(d=3, cap=1), dict(d=8, cap=128), dict(d=16, cap=64)]
BUDGETS = ["0", "0.001", "0.002", "0.01", "0.1", "1", "48", "1000"]
SIZES = [size_case(planes=pl, **s) for s in SHAPES for pl in (1, 2)] + \
        [size_case(planes=pl, P=528, override=b, **s) for s in SHAPES for pl in (1, 2) for b in BUDGETS] + \
        [size_case(P=528, free=f, **s) for s in SHAPES for f in (1 << 20, 1 << 28, 10 * GB, 288 * GB)] + \
        [size_case(P=1 << 22, cmax=1, **HEAD)]
CHI_A = [1, 6, 7, 7, 7, 7, 7, 7, 7, 6, 1]
CHI_B = [1, 6, 12, 12, 12, 12, 12, 12, 12, 6, 1]
CHI_W = [1, 6, 36, 40, 40, 40, 40, 40, 36, 6, 1]
ORDERS = [order_case(10, 6, 5, [CHI_A, CHI_B, CHI_B], [3, 3, 3]), order_case(10, 6, 5, [CHI_A, CHI_W, CHI_B], [3, 3, 3]),
          order_case(10, 6, 9, [CHI_B, CHI_B], [2, 16]), order_case(1, 3, 0, [[1, 1]], [2])]
CASES = SIZES + ORDERS


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("overlap_plan") / "overlap_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "overlap_plan_main.cpp"), "-o", exe])
    doc = json.loads(subprocess.run([exe] + CASES, check=True, capture_output=True, text=True).stdout)
    out = {c["case"]: c for c in doc["cases"]}
    out["_doc"] = doc
    return out


def _fields(name):
    f = name.split(":")
    return dict(d=int(f[1]), cap=int(f[2]), planes=int(f[3]), cmax=int(f[4]), P=int(f[5]), free=int(f[6]), override=f[7])


def test_sizes_and_routes(plans):
    lim = plans["_doc"]["OVERLAP_LDS_BYTES"]
    assert lim <= 160 * 1024 - 2048                          # beside the kernel's static LDS
    for name in SIZES:
        p, s = plans[name], _fields(name)
        assert p["pad"] % 16 == 0 and s["cap"] <= p["pad"] < s["cap"] + 16 and p["ld"] == p["pad"] + 2
        assert p["env"] == p["pad"] * p["ld"] and p["x"] == p["pad"] * s["d"] * p["pad"]
        assert p["state_bytes"] == s["planes"] * (3 * p["env"] + p["x"]) * 8
        assert p["lds"] == (1 if p["state_bytes"] <= lim else 0)
        assert p["pair_bytes"] == s["cmax"] ** 2 * s["planes"] * 8 + 16 + (0 if p["lds"] else p["state_bytes"])
    # the routes of the device tests: the headline model and every chi <= 20 case in LDS, real and complex; chi 72 in global scratch
    assert plans[size_case(**HEAD)]["lds"] == 1 and plans[size_case(**HEAD)]["state_bytes"] == (3 * 32 * 34 + 32 * 4 * 32) * 8
    assert plans[size_case(planes=2, **HEAD)]["lds"] == 1
    for s in (dict(d=6, cap=12), dict(d=5, cap=20), dict(d=3, cap=8)):
        assert plans[size_case(planes=2, **s)]["lds"] == 1
    assert plans[size_case(**SCRATCH)]["lds"] == 0 and plans[size_case(planes=2, **SCRATCH)]["state_bytes"] == 2 * (3 * 80 * 82 + 80 * 6 * 80) * 8


@pytest.mark.parametrize("name", SIZES)
def test_blocks_respect_the_budget(plans, name):
    p, s = plans[name], _fields(name)
    budget = min(48 * GB, s["free"] // 2) if s["override"] == "-" else max(0.001, float(s["override"])) * GB
    assert 1 <= p["block"] <= min(s["P"], plans["_doc"]["OVERLAP_MAX_BLOCK"])
    assert p["block"] * p["pair_bytes"] <= budget or p["block"] == 1                  # over the budget only as a single pair
    if p["block"] < min(s["P"], plans["_doc"]["OVERLAP_MAX_BLOCK"]):
        assert (p["block"] + 1) * p["pair_bytes"] > budget                            # and as many as fit


def test_the_floor_of_the_budget_cuts_the_scratch_route_to_single_pairs(plans):
    """What tests/test_gpu_overlap.py runs under: complex chi 72 is one pair per launch, real two; the LDS route is not cut at six pairs."""
    assert plans[size_case(planes=2, P=528, override="0", **SCRATCH)]["block"] == 1
    assert plans[size_case(planes=1, P=528, override="0", **SCRATCH)]["block"] == 2
    assert plans[size_case(P=528, override="0", **HEAD)]["block"] == 528
    assert plans[size_case(P=1 << 22, cmax=1, **HEAD)]["block"] == plans["_doc"]["OVERLAP_MAX_BLOCK"]
    for s in SHAPES:
        blocks = [plans[size_case(planes=2, P=528, override=b, **s)]["block"] for b in BUDGETS]
        assert all(x <= y for x, y in zip(blocks, blocks[1:])), blocks                # monotone in the budget


def _pad(c):
    return (c + 15) // 16 * 16


def _cost(ca, cb, T, d, p, ncb):
    tot = 0.0
    for j in range(T):
        al, ar, bl, br = _pad(ca[j]), _pad(ca[j + 1]), _pad(cb[j]), _pad(cb[j + 1])
        ia, oa, ib, ob = (al, ar, bl, br) if j <= p else (ar, al, br, bl)
        tot += (ia * ib * d * ob + oa * ia * d * ob) * (ncb if j == p else 1)
    return tot


def test_pair_order(plans):
    a = plans[ORDERS[0]]                                      # pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); 7 and 12 both pad to 16: all ties
    assert len(set(a["cost"])) == 1 and a["order"] == [0, 1, 2, 3, 4, 5]
    assert a["cost"][0] == _cost(CHI_A, CHI_B, 10, 6, 5, 3)
    b = plans[ORDERS[1]]                                      # model 1 is the wide one: (1,1) first, then its pairs, the narrow ones last
    assert b["order"][0] == 3 and set(b["order"][1:3]) == {1, 4} and b["order"][3:] == [0, 2, 5]
    assert b["cost"][1] == _cost(CHI_A, CHI_W, 10, 6, 5, 3) and b["cost"][3] == _cost(CHI_W, CHI_W, 10, 6, 5, 3)
    assert all(b["cost"][x] >= b["cost"][y] for x, y in zip(b["order"], b["order"][1:]))
    c = plans[ORDERS[2]]                                      # the label site counts once per class of b: (1,1) and (0,1) before (0,0)
    assert c["order"] == [1, 2, 0] and c["cost"][1] == c["cost"][2] > c["cost"][0]
    assert plans[ORDERS[3]]["order"] == [0] and plans[ORDERS[3]]["cost"][0] == 2 * (16 * 16 * 3 * 16) * 2
    for name in ORDERS:
        assert sorted(plans[name]["order"]) == list(range(len(plans[name]["cost"])))
