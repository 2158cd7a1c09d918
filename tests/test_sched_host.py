"""The schedule of the inPALM loop (dot-socp_amd/csrc/schedule.h) is plain host arithmetic in a header without HIP: built with
g++ under AddressSanitizer + UBSan into an ordinary executable, tests/san/sched_check.cpp, which drives the planner that
Solver::step() executes -- plan_step() itself, not a model of it -- for iterations 1..400 over the grid of
tests/test_qcone_schedule.py and with a time limit that passes at each of the first 40 iterations: every reader of beta or q
finds them, no early cone pass is handed to an iteration that schedules another form, the stopping check comes at most two
iterations after the limit (seen at iteration 6: checks [1, 4, 7]; without the gamma form: stop at 6)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "san", "_build")


def test_planner_under_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sched_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "dot-socp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "san", "sched_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 failed" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
