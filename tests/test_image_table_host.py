"""The tap tables of imresize (dot-socp_amd/csrc/image_table.h) are plain host arithmetic in a header without HIP: built with
g++ under AddressSanitizer + UBSan into an ordinary executable and driven by tests/san/image_table_check.cpp over a list of
lengths (1 -> n, n -> 1, odd, shrinking by 65536, the multilevel grids): every index in [0, n_in), every row sums to 1
within 2 ulp, no row is empty, no write outside buffers of the documented size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "san", "_build")


def test_image_tables_under_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "image_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "dot-socp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "san", "image_table_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 failed" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
