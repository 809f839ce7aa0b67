#!/usr/bin/env python3
"""Compare the gfx950 code objects inside two builds of one object file, symbol by symbol: the code bytes of every function, the
kernel descriptors, and the per-kernel metadata (registers, scratch, LDS, kernarg size).  A refactor of host code must leave them
equal; a change in the order the kernels are emitted in moves the descriptors' code offsets and nothing else.
usage: compare_code_objects.py parent/mpst_impute.o branch/mpst_impute.o"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ("agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|kernarg_segment_size|"
          "max_flat_workgroup_size|sgpr_spill_count|vgpr_spill_count|wavefront_size|uses_dynamic_stack")


def extract(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}"])
    return co


def load(path):
    data = open(path, "rb").read()
    secs = {}
    for ln in subprocess.check_output([f"{LLVM}/llvm-readelf", "-SW", path], text=True).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", ln)
        if m:
            secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
    syms = {}
    for ln in subprocess.check_output([f"{LLVM}/llvm-readelf", "-sW", path], text=True).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit() and not f[7].startswith("__hip_cuid_"):   # (named after a hash of the build path)
            name, addr, size, (sec, saddr, soff) = f[7], int(f[1], 16), int(f[2]), secs[int(f[6])]
            off = addr - saddr + soff
            syms[name] = (f[3], b"" if sec == ".bss" else data[off:off + size])
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", path], text=True)
    kernels = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        kernels[re.search(r"\.name:\s+(\S+)", blk).group(1)] = dict(re.findall(rf"\.({FIELDS}):\s+(\S+)", blk))
    return data, syms, kernels


def demangle(name):
    try:
        return subprocess.check_output(["c++filt", name], text=True).strip()
    except OSError:
        return name


def main(a_obj, b_obj):
    with tempfile.TemporaryDirectory() as tmp:
        (da, a, ka), (db, b, kb) = load(extract(a_obj, tmp, "a")), load(extract(b_obj, tmp, "b"))
    print(f"code objects byte-identical: {da == db} ({len(da)} / {len(db)} bytes)")
    print(f"symbols: {len(a)} / {len(b)}, same names: {set(a) == set(b)}")
    funcs = [n for n in a if a[n][0] == "FUNC"]
    print(f"functions: {len(funcs)}, with identical code bytes: {sum(1 for n in funcs if n in b and a[n][1] == b[n][1])}")
    for n in funcs:          # which ones differ, and what of their metadata moved
        if n in b and a[n][1] != b[n][1]:
            moved = ", ".join(f"{k} {ka[n].get(k)} -> {kb[n].get(k)}" for k in ka.get(n, {}) if n in kb and ka[n].get(k) != kb[n].get(k))
            print(f"  differs: {demangle(n)}: {len(a[n][1])} -> {len(b[n][1])} code bytes" + (f"; {moved}" if moved else ""))
    for n in sorted(set(a) ^ set(b)):
        print(f"  only in {'the first' if n in a else 'the second'}: {demangle(n)}")
    ok = set(a) == set(b) and all(a[n][1] == b[n][1] for n in funcs)
    for n in a:
        if n in b and a[n][0] == "OBJECT" and a[n][1] != b[n][1]:
            idx = [i for i in range(min(len(a[n][1]), len(b[n][1]))) if a[n][1][i] != b[n][1][i]]
            only_entry = n.endswith(".kd") and len(a[n][1]) == len(b[n][1]) and all(16 <= i < 24 for i in idx)   # kernel_code_entry_byte_offset
            ok = ok and only_entry
            if not only_entry:
                print(f"  object {n}: differing bytes at {idx[:8]}")
    print(f"kernels: {len(ka)} / {len(kb)}, per-kernel metadata equal: {ka == kb}, emitted in the same order: {list(ka) == list(kb)}")
    print("EQUAL DEVICE CODE" if ok and ka == kb else "DEVICE CODE DIFFERS")
    return 0 if ok and ka == kb else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
