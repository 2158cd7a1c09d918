#!/usr/bin/env python3
"""Resource usage of every gfx950 kernel of libdotsocp, from the compiler's own per-kernel summary: each .hip file is
compiled to device assembly with the flags csrc/Makefile gives that file (`hipcc -S --offload-device-only`; the
-ffp-contract override of the transform objects is read from the Makefile's own rule), and the `; Kernel info:` block
that the AMDGPU backend appends to every kernel is tabulated -- VGPRs, AGPRs, SGPRs, scratch (spill) bytes, static LDS
bytes, occupancy in waves per SIMD.  Runs without a GPU.

    python tools/isa_stats.py > profiles/r02_isa_stats.txt

--hash adds a digest of each kernel's instructions (label to .Lfunc_end, comments stripped, local label numbers
removed): two trees whose tables agree in that column and in the mangled names ship the same kernels, wherever the
source of a kernel lives.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot-socp_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]


def contract_overrides():
    """{file.hip: value} from the Makefile's `build/a.o build/b.o: CXXFLAGS := ... -ffp-contract=$(DCT_CONTRACT) ...` rule"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    value = re.search(r"^DCT_CONTRACT\s*\?=\s*(\S+)", mk, re.M).group(1)
    rule = re.search(r"^((?:build/\S+\.o\s*)+):\s*CXXFLAGS\s*:=.*-ffp-contract=\$\(DCT_CONTRACT\)", mk, re.M).group(1)
    return {os.path.basename(o)[:-2] + ".hip": value for o in rule.split()}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return out.stdout.splitlines()


def body_hash(name, text):
    body = text[:text.index(".Lfunc_end")]
    body = re.sub(r"\s*;.*", "", body)                       # comments
    body = re.sub(r"\.LBB\d+_", ".LBB_", body)               # basic-block labels carry the function's number in its file
    body = re.sub(r"\.Lfunc_\w+?\d+", ".Lfunc", body)
    lines = [ln.strip() for ln in body.splitlines() if ln.strip()]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    want_hash = "--hash" in sys.argv[1:]
    contract = contract_overrides()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")):
            asm = os.path.join(tmp, src[:-4] + ".s")
            flags = [f if not f.startswith("-ffp-contract=") else "-ffp-contract=" + contract.get(src, "off") for f in FLAGS]
            subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--offload-device-only", os.path.join(CSRC, src), "-o", asm],
                           check=True, stderr=subprocess.DEVNULL)
            text = open(asm).read()
            # "\t.globl\t<name>" ... "; Kernel info:" blocks follow each kernel's code
            for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^; Kernel info:\n(.*?)^; WaveLimiterHint", text, re.S | re.M):
                name, info = m.group(1), m.group(3)
                get = lambda k: int(re.search(r"; %s: (\d+)" % k, info).group(1))      # noqa: E731
                rows.append((src, name, get("NumVgprs"), get("NumAgprs"), get("TotalNumSgprs"), get("ScratchSize"),
                             get("LDSByteSize"), get("Occupancy"), body_hash(name, m.group(2)) if want_hash else ""))
    names = demangle([r[1] for r in rows])
    print("# gfx950 kernel resources of libdotsocp (compiler summary; flags: %s; -ffp-contract=%s for %s)"
          % (" ".join(FLAGS[:-1]), next(iter(contract.values())), " ".join(sorted(contract))))
    print("# occupancy = waves per SIMD the register / LDS budget allows; scratch = spill bytes per lane (0 is the bar)")
    print("%-16s %5s %5s %5s %8s %8s %4s  %s%s" % ("file", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "occ",
                                                 "hash              " if want_hash else "", "kernel"))
    spills = 0
    for (src, mangled, v, a, sg, sc, lds, occ, h), nm in zip(rows, names):
        nm = re.sub(r"^void ", "", nm)
        nm = re.sub(r"\(.*", "", nm).replace("dotsocp::", "")
        # with --hash the mangled name follows: it is the key two tables are compared by
        print("%-16s %5d %5d %5d %8d %8d %4d  %s%s%s" % (src, v, a, sg, sc, lds, occ, h + "  " if want_hash else "", nm,
                                                       "  " + mangled if want_hash else ""))
        spills += sc > 0
    print("# %d kernels, %d with scratch" % (len(rows), spills))
    return 0


if __name__ == "__main__":
    sys.exit(main())
