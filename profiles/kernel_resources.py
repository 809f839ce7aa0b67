#!/usr/bin/env python3
"""One line per kernel from a compile log taken with -Rpass-analysis=kernel-resource-usage (make mpst_impute.o EXTRA=-Rpass-analysis=...):
VGPRs, AGPRs, scratch bytes per lane, SGPR / VGPR spills, occupancy (waves per SIMD) and static LDS bytes, sorted by name.
usage: kernel_resources.py build.log [regex on the demangled name]   (default: the imputation sweep, k_imp_left / k_imp_leftb)"""
import re
import subprocess
import sys

KEYS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"),
        ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def main(log, pattern=r"\bk_imp_leftb?<"):
    kernels, cur = {}, None
    for ln in open(log):
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+(.+?): (\d+))\s+\[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1):
            cur = kernels.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2)] = int(m.group(3))
    names = subprocess.check_output(["c++filt"] + list(kernels), text=True).split("\n")
    rows = sorted((re.sub(r"^void mpst::|\(.*$", "", d), kernels[k]) for k, d in zip(kernels, names) if re.search(pattern, d))
    print(f"{len(rows)} kernels")
    for name, r in rows:
        print(f"{name:48s} " + " ".join(f"{short}={r[key]}" for key, short in KEYS))
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
