"""The grouping of mpst_sweep_batch_multi (csrc/mpst_batch_groups.h) on the CPU: tests/batch_groups_main.cpp, which includes nothing
but that header, is compiled with the host compiler under AddressSanitizer and UBSan and run as a stand-alone program.  Every case
must equal the restatement below: groups in order of first appearance, each with its members' positions, and the first group above
the limit rejected."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")

MAX_GROUP = 64
CASES = {
    "one context": [3],
    "all keys equal": [2] * 7,
    "alternating": [0, 1, 0, 1, 0, 1],
    "first appearance, negative keys": [7, -3, 7, 5, -3],
    "512 distinct keys": [(k * 37) % 512 - 100 for k in range(512)],
    "64 in one group": [1] + [0] * 64 + [1],
    "65 in one group": [1] + [0] * 65 + [1],
    "a later group above the limit": [4] * 3 + [9] * 65 + [4] * 2,
}


def restated(keys, max_group):
    groups = {}                                   # (dicts keep the order of insertion)
    for k, key in enumerate(keys):
        groups.setdefault(key, []).append(k)
    above = [g for g, members in enumerate(groups.values()) if len(members) > max_group]
    return {"keys": list(groups), "index": list(groups.values()), "rejected": above[0] if above else -1}


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("batch_groups") / "batch_groups")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "batch_groups_main.cpp"), "-o", exe])
    args = ["%d:%s" % (MAX_GROUP, ",".join(map(str, keys))) for keys in CASES.values()]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    return dict(zip(CASES, json.loads(out)))


@pytest.mark.parametrize("name", CASES)
def test_groups_equal_the_restatement(planned, name):
    assert planned[name] == restated(CASES[name], MAX_GROUP)


def test_the_cases_cover_what_they_name():
    want = {name: restated(keys, MAX_GROUP) for name, keys in CASES.items()}
    assert want["first appearance, negative keys"]["keys"] == [7, -3, 5]
    assert want["first appearance, negative keys"]["index"] == [[0, 2], [1, 4], [3]]
    assert len(want["512 distinct keys"]["keys"]) == 512
    assert want["64 in one group"]["rejected"] == -1 and want["65 in one group"]["rejected"] == 1
    assert want["a later group above the limit"]["rejected"] == 1
