"""The pair analysis plan (csrc/mpst_query_plan.h: pair_plan, pair_state_in_lds and what they are made of) on the CPU:
tests/pair_plan_main.cpp compiled alone with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program."""
import pytest

from tests import pair_plan as PP

GB = PP.GB

# the shapes of tests/test_gpu_pair.py and the flagship of profiles/pair_analysis_timing.py
CHI20 = dict(C=3, T=12, d=4, cap=20)            # 2 * 10 * 20 * 24 * 8 = 76 800 bytes of state: LDS
CHI72 = dict(C=2, T=6, d=2, cap=72)             # 2 * 3 * 72 * 76 * 8 = 262 656 bytes: global scratch
CHI40 = dict(C=2, T=12, d=4, cap=40)            # the blocks-and-placement case
FLAG = dict(C=2, T=100, d=4, cap=32)
BUDGETS = ["0", "0.001", "0.002", "0.004", "0.01", "0.05", "0.2", "1", "8", "48", "1000"]
SHAPES = [CHI20, CHI72, CHI40, FLAG, dict(C=1, T=1, d=3, cap=1), dict(C=2, T=100, d=11, cap=16), dict(C=10, T=200, d=16, cap=128)]
CASES = [PP.case(**s) for s in SHAPES] + [PP.case(override=b, **s) for s in SHAPES for b in BUDGETS] + \
        [PP.case(store_rho=False, override=b, **s) for s in SHAPES for b in ("0", "1")] + \
        [PP.case(free=f, **s) for s in SHAPES for f in (1 << 20, 1 << 28, 10 * GB, 288 * GB)]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = PP.build(tmp_path_factory.mktemp("pair_plan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    doc, plans = PP.run(exe, CASES)
    assert doc["PAIR_LDS_BYTES"] <= 160 * 1024 - 2048 and doc["PAIR_MAX_WORKGROUPS"] >= 256
    plans["_doc"] = doc
    return plans


def _shape(name):
    f = name.split(":")
    return dict(C=int(f[1]), T=int(f[2]), d=int(f[3]), cap=int(f[4]), store=f[5] == "1", block=int(f[6]))


def test_routes(plans):
    """One shape of the device tests on each route, and the figures the route is decided from."""
    a, b = plans[PP.case(**CHI20)], plans[PP.case(**CHI72)]
    assert a["lds"] == 1 and a["state_bytes"] == 76800 and a["ld"] == 20 and a["stride"] == 24 and a["tiles"] == 2
    assert b["lds"] == 0 and b["state_bytes"] == 262656 and b["tiles"] == 5
    assert plans[PP.case(**CHI40)]["lds"] == 0
    assert plans[PP.case(**FLAG)]["lds"] == 0 and plans[PP.case(**FLAG)]["state_bytes"] == 184320      # 2 * 10 * 32 * 36 * 8
    lim = plans["_doc"]["PAIR_LDS_BYTES"]
    for name in CASES:
        p, s = plans[name], _shape(name)
        npair = s["d"] * (s["d"] + 1) // 2
        assert p["ld"] % 4 == 0 and s["cap"] <= p["ld"] < s["cap"] + 4 and p["stride"] >= p["ld"] and 16 * p["tiles"] >= p["ld"]
        assert p["state_bytes"] == 2 * npair * p["ld"] * p["stride"] * 8
        assert p["lds"] == (1 if p["state_bytes"] <= lim else 0)
        fro = npair * p["tiles"] * s["d"] ** 2 * 8
        assert p["workgroup_bytes"] == fro + (0 if p["lds"] else p["state_bytes"])


@pytest.mark.parametrize("name", CASES)
def test_blocks_are_whole_rows_and_the_cap_is_never_zero(plans, name):
    p, s = plans[name], _shape(name)
    row0 = p["row0"]
    assert row0[0] == 0 and row0[-1] == s["T"] and all(a < b for a, b in zip(row0, row0[1:]))      # whole rows, each once, none empty
    assert 1 <= p["workgroups"] <= min(s["C"] * s["T"], plans["_doc"]["PAIR_MAX_WORKGROUPS"])
    if not s["store"]:
        assert row0 == [0, s["T"]] and p["rho_bytes"] == 0
        return
    row = lambda i: s["C"] * (s["T"] - 1 - i) * s["d"] ** 4 * 8
    sizes = [sum(row(i) for i in range(a, b)) for a, b in zip(row0, row0[1:])]
    assert p["rho_bytes"] == max(sizes)
    for (a, b), size in zip(zip(row0, row0[1:]), sizes):
        assert size <= s["block"] or b == a + 1                     # over the limit only as a single row
        if b < s["T"] and name.endswith(":%d:-" % (200 * GB)):      # greedy under the block limit (the budget's eighth is larger here)
            assert size + row(b) > s["block"]


@pytest.mark.parametrize("shape", SHAPES)
def test_cap_is_monotone_in_the_budget(plans, shape):
    for store in (True, False):
        names = [PP.case(override=b, **shape) for b in BUDGETS] if store else [PP.case(store_rho=False, override=b, **shape) for b in ("0", "1")]
        wgs = [plans[n]["workgroups"] for n in names]
        assert all(a <= b for a, b in zip(wgs, wgs[1:])), wgs
        nblocks = [len(plans[n]["row0"]) - 1 for n in names]
        assert all(a >= b for a, b in zip(nblocks, nblocks[1:])), nblocks
    free = [plans[PP.case(free=f, **shape)]["workgroups"] for f in (1 << 20, 1 << 28, 10 * GB, 288 * GB)]
    assert all(a <= b for a, b in zip(free, free[1:])), free


def test_a_small_budget_cuts_blocks_and_lowers_the_cap(plans):
    """The override the device test runs under: at least two blocks and fewer workgroups than chains, neither without it."""
    small, full = plans[PP.case(override="0.001", **CHI40)], plans[PP.case(**CHI40)]
    assert len(small["row0"]) - 1 >= 2 and small["workgroups"] < CHI40["C"] * CHI40["T"]
    assert len(full["row0"]) - 1 == 1 and full["workgroups"] == CHI40["C"] * CHI40["T"]
    # the flagship: 9900 pairs of 2 KB are one block; d = 11 at T = 100 is cut under the 512 MB limit
    assert plans[PP.case(**FLAG)]["row0"] == [0, 100]
    big = plans[PP.case(C=2, T=100, d=11, cap=16)]
    assert len(big["row0"]) - 1 >= 3 and big["rho_bytes"] <= PP.AN_BLOCK_BYTES
