"""bench.py --full: a plain run does only what its headline figure needs (set-up, warm-up, timed steps, the line); the CPU
baseline and the device copy rate come with --full alone.  CPU: the option and its default.  GPU: a plain and a --full line
of one small grid."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert bench.parse_args().full is True


def _line(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DOTSOCP_BENCH_NOPROF"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                          "--grid", "40", "36", "12"] + list(extra), env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_leaves_the_extras_to_full():
    plain = _line()
    assert "cpu_baseline" not in plain and plain["config"]["box_copy_gbs"] is None
    # the phase timers of one process come from its timed iterations themselves: they stay in the plain line
    assert plain["config"]["per_phase_hip_events_in_timed_region"] is True
    assert plain["roofline"]["launches"] > 0 and plain["kernel_ms"]["poisson"] > 0
    full = _line("--full", "--cpu-seconds", "0")
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["sample_grid"] == [40, 36, 12]
    assert full["config"]["box_copy_gbs"] is None or full["config"]["box_copy_gbs"] > 100
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["config"]["kkt_checks_in_timed_region"] == full["config"]["kkt_checks_in_timed_region"]
    assert full["config"]["per_phase_hip_events_in_timed_region"] is True
