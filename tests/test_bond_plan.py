"""The host decisions of the per-bond launch chain (csrc/mpst_bond_plan.h) on the CPU: tests/bond_plan_main.cpp, which includes
nothing but that header, is compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program.
Every line it prints must equal the restatement below: the bond order of a sweep and each bond's environment step, the rows a
step reads against the rows that are valid, the row pointers, the chosen instantiation of k_yhat_s / k_grad_s, and the two lists
of instantiations themselves (the X-macros the launchers expand)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")

SWEEP_T = (2, 3, 4, 7)
ROWS = [(-1, 10, 8), (0, 10, 8), (3, 10, 4), (2, 7, 16), (6, 96 * 12, 8)]
# (d, cap, MPST_YS_V1) -> row of YHAT_S_LIST; (d, waves) -> row of GRAD_S_LIST
YHAT_LIST = [(2, 1, 1), (2, 1, 0), (2, 0, 0), (4, 0, 0)]
GRAD_LIST = [(2, 1, 0, 256, 8, 512), (1, 2, 0, 256, 8, 512), (1, 1, 25, 256, 4, 256), (1, 1, 25, 256, 8, 512), (1, 1, 0, 256, 8, 512)]
YHAT_ROWS = {(4, 32, 0): (2, 1, 1), (4, 12, 0): (2, 1, 1), (4, 12, 1): (2, 1, 0), (4, 11, 0): (2, 1, 0), (3, 10, 0): (2, 0, 0),
             (16, 3, 0): (2, 0, 0), (2, 40, 0): (4, 0, 0), (2, 33, 1): (4, 0, 0)}
GRAD_ROWS = {(2, 8): (2, 1, 0, 256, 8, 512), (3, 8): (2, 1, 0, 256, 8, 512), (4, 8): (1, 1, 25, 256, 8, 512), (4, 4): (1, 1, 25, 256, 4, 256),
             (5, 8): (1, 1, 0, 256, 8, 512), (8, 8): (1, 1, 0, 256, 8, 512), (9, 8): (1, 2, 0, 256, 8, 512), (16, 8): (1, 2, 0, 256, 8, 512)}


def step_restated(site, left, T):
    """(site, left_side, prev_site, prev_bond, out_bond, out_site): LE[site] from LE[site - 1], RE[site] from RE[site + 1]."""
    if left:
        return (site, 1, site - 1 if site > 0 else -1, site, site + 1, site)
    return (site, 0, site + 1 if site < T - 1 else -1, site + 1, site, site)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bond_plan") / "bond_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "bond_plan_main.cpp"), "-o", exe])
    args = ["slot:%d,%d" % (T, k) for T in SWEEP_T for k in range(2 * (T - 1))]
    args += ["env:%d,%d,%d" % (T, j, left) for T in SWEEP_T for j in range(T) for left in (0, 1)]
    args += ["row:%d,%d,%d" % r for r in ROWS]
    args += ["yhat:%d,%d,%d" % k for k in YHAT_ROWS] + ["grad:%d,%d" % k for k in GRAD_ROWS] + ["lists"]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    got = {"slot": {}, "env": {}, "row": {}, "yhat": {}, "grad": {}}
    for line in out.splitlines():
        w = line.split()
        x = tuple(None if t == "null" else int(t) for t in w[1:])
        if w[0] in ("yhat_list", "grad_list"):
            got[w[0]] = x
        else:
            nkey = {"slot": 2, "env": 3, "row": 3, "yhat": 3, "grad": 2}[w[0]]
            got[w[0]][x[:nkey]] = x[nkey:]
    return got


@pytest.mark.parametrize("T", SWEEP_T)
def test_sweep_order_and_the_step_of_every_bond(plan, T):
    nb = T - 1
    order = list(range(nb - 1, -1, -1)) + list(range(nb))
    for k, lid in enumerate(order):
        left = 1 if k < nb else 0
        nxt = order[k + 1] if k + 1 < 2 * nb else -1
        chains = 0 if k in (nb - 1, 2 * nb - 1) else 1         # not at the turning point, not at the last slot
        got = plan["slot"][(T, k)]
        assert got[:4] == (lid, left, nxt, chains), (T, k)
        site, left_side, prev_site, prev_bond, out_bond, out_site = got[4:]
        # going left the step writes RE[lid + 1], going right LE[lid]
        assert (left_side, out_site, site) == ((0, lid + 1, lid + 1) if left else (1, lid, lid)), (T, k)
        assert got[4:] == step_restated(site, left_side, T), (T, k)
        assert (prev_site == -1) == (site == (0 if left_side else T - 1)), (T, k)       # T = 2: both ends on the one bond
    assert len(plan["slot"]) == sum(2 * (t - 1) for t in SWEEP_T)


@pytest.mark.parametrize("T", SWEEP_T)
def test_every_bond_of_a_sweep_reads_valid_environment_rows(plan, T):
    """From a cache build at label site T - 1 (LE[0 .. T-2]) through a whole sweep: an update of bond (lid, lid + 1) changes both
    site tensors, which invalidates LE[j >= lid] and RE[j <= lid + 1]; the bond's step then writes one row."""
    valid = {1: set(range(T - 1)), 0: set()}
    for k in range(2 * (T - 1)):
        lid = plan["slot"][(T, k)][0]
        assert lid - 1 < 0 or lid - 1 in valid[1], (T, k, "LE[lid-1]")
        assert lid + 2 > T - 1 or lid + 2 in valid[0], (T, k, "RE[lid+2]")
        valid[1] -= set(range(lid, T))
        valid[0] -= set(range(0, lid + 2))
        site, left_side, prev_site, prev_bond, out_bond, out_site = plan["slot"][(T, k)][4:]
        assert prev_site == -1 or prev_site in valid[left_side], (T, k, "the step's previous row")
        valid[left_side].add(out_site)
    assert valid[1] == set(range(T - 1))          # as the build at T - 1 left it: the next sweep starts from the same rows


@pytest.mark.parametrize("T", SWEEP_T)
def test_cache_builder_steps_read_valid_rows(plan, T):
    """construct_caches around label site ls: left steps at sites 0 .. ls-1 ascending (capped at T-2), right steps at sites
    T-1 .. ls+1 descending (floored at 1) - the loops of enqueue_caches, restated - with the steps the header gives them."""
    for ls in sorted({0, T - 1, T // 2}):
        valid = {1: set(), 0: set()}
        steps = [(j, 1) for j in range(0, min(ls, T - 1))] + [(j, 0) for j in range(T - 1, max(ls, 0), -1)]
        for j, left in steps:
            got = plan["env"][(T, j, left)]
            assert got == step_restated(j, left, T), (T, ls, j, left)
            assert got[2] == -1 or got[2] in valid[left], (T, ls, j, left)
            valid[left].add(got[5])
        assert valid[1] == set(range(min(ls, T - 1))) and valid[0] == set(range(ls + 1, T)), (T, ls)
        assert all(1 <= j for j, left in steps if not left) and all(j <= T - 2 for j, left in steps if left)


def test_row_pointers(plan):
    for site, stride, esz in ROWS:
        want = (None, None) if site < 0 else (site * stride * 8, site * stride * esz)
        assert plan["row"][(site, stride, esz)] == want, (site, stride, esz)


def test_variant_rows_and_the_lists_they_index(plan):
    yl, gl = plan["yhat_list"], plan["grad_list"]
    assert yl[0] == 4 and [yl[1 + 3 * r:4 + 3 * r] for r in range(4)] == YHAT_LIST
    assert gl[0] == 5 and [gl[1 + 6 * r:7 + 6 * r] for r in range(5)] == GRAD_LIST
    for key, row in YHAT_ROWS.items():
        assert YHAT_LIST[plan["yhat"][key][0]] == row, key
    for key, row in GRAD_ROWS.items():
        assert GRAD_LIST[plan["grad"][key][0]] == row, key
