"""The pair analysis plan (csrc/mpst_query_plan.h: pair_plan) for the tests: tests/pair_plan_main.cpp, which includes nothing but
that header, compiled with the host compiler and run as a stand-alone program."""
import json
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mpstime.jl_amd", "csrc")

GB = 1 << 30
AN_BLOCK_BYTES = 512 << 20          # csrc/mpst_analysis.hip: the store of rho_ij of one block


def case(C, T, d, cap, store_rho=True, block_bytes=AN_BLOCK_BYTES, free=200 * GB, override=None):
    return "p:" + ":".join(str(v) for v in (C, T, d, cap, int(store_rho), block_bytes, free, "-" if override is None else override))


def build(directory, flags=()):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), "pair_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(HERE, "pair_plan_main.cpp"), "-o", exe])
    return exe


def run(exe, cases):
    doc = json.loads(subprocess.run([exe] + list(cases), check=True, capture_output=True, text=True).stdout)
    return doc, {c["case"]: c for c in doc["cases"]}
