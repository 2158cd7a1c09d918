"""The buffer layouts of the particle march (dot-socp_amd/csrc/particle_block.h: ParticleBlock, MapFinalBlock) are plain
host arithmetic in a header without HIP: built with g++ under AddressSanitizer + UBSan into an ordinary executable and
driven by tests/san/particle_block_check.cpp -- n in {1, 2, 255, 256, 257}, every combination of push and map, with or
without mass, disp and action: regions disjoint, in the documented order, on 8-byte boundaries, n 32-bit flags, and the
totals 2n + nunit + npath + (n + 1) / 2 + 1 resp. m_part + MS_COUNT * map_blocks(n) of the formulas they replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "san", "_build")


def test_particle_block_layouts():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "particle_block_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "dot-socp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "san", "particle_block_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 failed" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
