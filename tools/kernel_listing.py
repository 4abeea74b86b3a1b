#!/usr/bin/env python3
"""Device-code listing of .hip files, for showing that a host-side change left the kernels alone.

Per file: every defined FUNC symbol of the gfx950 code object as (mangled name, size in bytes), sorted, then the sorted
table of kernel_resources.py.  --full prints those lines.  The default prints one line per kernel template: how many
instantiations, their code bytes together, and a SHA-256 over the template's lines of the full listing -- equal digests
mean the same instantiations with the same names, code sizes and resources, whatever order they were instantiated in.

    python tools/kernel_listing.py [--full] nbody_cosmological_simulation_amd/csrc/nb_small.hip [more .hip files]
"""
import collections
import hashlib
import os
import subprocess
import sys
import tempfile

ROCM = "/opt/rocm"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "-I" + ROCM + "/include"]      # csrc/Makefile's CXXFLAGS


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def base(demangled):
    return demangled.replace("void ", "").replace("(anonymous namespace)::", "").split("<")[0].split("(")[0].strip()


def main():
    full = "--full" in sys.argv
    here = os.path.dirname(os.path.abspath(__file__))
    for src in (a for a in sys.argv[1:] if a != "--full"):
        with tempfile.TemporaryDirectory() as tmp:
            bundle, obj = os.path.join(tmp, "dev.o"), os.path.join(tmp, "gfx950.o")
            run([ROCM + "/bin/hipcc", *FLAGS, "--offload-device-only", "-c", src, "-o", bundle])
            run([ROCM + "/llvm/bin/clang-offload-bundler", "--type=o", "--unbundle", "--targets=hip-amdgcn-amd-amdhsa--gfx950",
                 "--input=" + bundle, "--output=" + obj])
            fields = (line.split() for line in run([ROCM + "/llvm/bin/llvm-readelf", "-sW", obj]).splitlines())
            syms = sorted({(f[7], int(f[2], 0)) for f in fields if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND"})
        names = run(["c++filt"], input="\n".join(s[0] for s in syms)).splitlines()
        res = sorted(run([sys.executable, os.path.join(here, "kernel_resources.py"), src]).splitlines())
        print(f"== {os.path.basename(src)}: {len(syms)} kernels")
        if full:
            print("\n".join([f"{n} {size}" for n, size in syms] + res))
            continue
        lines, count, code = collections.defaultdict(list), collections.Counter(), collections.Counter()
        for (n, size), dem in zip(syms, names):
            lines[base(dem)].append(f"{n} {size}")
            count[base(dem)] += 1
            code[base(dem)] += size
        for r in res:
            lines[base(r.split(" VGPR ")[0])].append(" ".join(r.split()))
        for b in sorted(lines):
            digest = hashlib.sha256("\n".join(lines[b]).encode()).hexdigest()[:20]
            print(f"{b:34s} {count[b]:3d} kernels {code[b]:8d} code bytes  sha256 {digest}")


if __name__ == "__main__":
    main()
