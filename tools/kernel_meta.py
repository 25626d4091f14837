#!/usr/bin/env python3
"""The code objects' metadata of every kernel in a built libx264gpu.so (no GPU needed): VGPRs, AGPRs, SGPRs, scratch, spilled VGPRs / SGPRs, LDS.
  tools/kernel_meta.py LIB                 one line a kernel (demangled name, the seven numbers)
  tools/kernel_meta.py LIB --against OLD   the kernels of OLD whose numbers differ in LIB or that LIB lacks (exit status 1 if there are any), then the kernels new in LIB
The library's device code is taken out with llvm-objcopy / clang-offload-bundler and read with llvm-readelf --notes (all from the ROCm LLVM beside hipcc)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size")
HEAD = ("VGPRs", "AGPRs", "SGPRs", "scratch", "spilled VGPRs", "spilled SGPRs", "LDS")


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib, arch="gfx950"):
    """{demangled kernel name: tuple of FIELDS}; a name that several translation units define (anonymous namespaces) gets " #2", " #3" in the order of the units"""
    raw = {}
    with tempfile.TemporaryDirectory() as d:
        fat, one, co = os.path.join(d, "fat.bin"), os.path.join(d, "one.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "unused")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]          # one bundle a translation unit
        for i, at in enumerate(starts):
            open(one, "wb").write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--input=" + one, "--output=" + co])
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
            cur = None
            for line in notes.splitlines() + ["  - end"]:
                if line.startswith("  - ") or not line.startswith("    "):          # the next kernel's entry, or the end of the list
                    if cur and ".name" in cur:
                        n, k = cur[".name"], 1
                        while (n if k == 1 else f"{n} #{k}") in raw:
                            k += 1
                        raw[n if k == 1 else f"{n} #{k}"] = tuple(cur.get(f, 0) for f in FIELDS)
                    cur = {} if line.startswith("  - ") else None
                m = re.match(r"(?:  - |    )(\.[a-z_]+):\s*(\S*)\s*$", line)
                if cur is not None and m and (m.group(1) in FIELDS or m.group(1) == ".name"):
                    cur[m.group(1)] = m.group(2) if m.group(1) == ".name" else int(m.group(2))
    names = sorted(raw)
    filt = os.path.join(LLVM, "llvm-cxxfilt")
    dem = subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(n.split(" ")[0] for n in names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) + n[len(n.split(" ")[0]):]: raw[n] for n, d in zip(names, dem)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--against")
    a = ap.parse_args()
    new = kernels(a.lib)
    if not a.against:
        for n in sorted(new):
            print(n, *new[n])
        return 0
    old = kernels(a.against)
    bad = [n for n in sorted(old) if new.get(n) != old[n]]
    for n in bad:
        print("DIFFERS", n, old[n], "->", new.get(n))
    print(f"{len(old)} kernels in {a.against}: {len(old) - len(bad)} with identical metadata in {a.lib}, {len(bad)} differ or are missing ({', '.join(HEAD)})")
    for n in sorted(set(new) - set(old)):
        print("NEW", n, *new[n])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
