"""Reads of never-written device memory (DOTSOCP_POISON=1, csrc/guard.hip).

Every test of the suite sees 0.0 in the slots of a device buffer that nothing has written yet: fresh hipMalloc memory has
come back as zeros, and the block cache zero-fills what it hands out again.  For nearly every kernel here 0.0 is the value
that makes a stray read harmless -- pad rows and columns, the boundary slots mexBFd leaves unwritten, halo layers before
the first exchange, tile-border side buffers, scratch that only some launches fill.  With DOTSOCP_POISON=1 every
floating-point buffer from guarded_malloc comes filled with the quiet NaN POISON instead (integer buffers -- indices,
counters, flags -- are left alone: a poisoned index would be a wild address).

(1) The mode is live: dotsocp_debug_alloc_peek shows POISON in every slot of a fresh block, after
    dotsocp_release_cache(), of a block reused from the cache, and between guard bands (DOTSOCP_CANARY=1).
(2) The battery (tests/poison_battery.py): every group of scenarios runs twice in fresh child processes, plain and
    poisoned.  Same launches, same inputs; only memory that nobody may read differs.  So the sha256 of every result array
    must be IDENTICAL -- no tolerance is involved -- and no result may hold a non-finite value (but for the one scenario
    that feeds NaNs in on purpose).  A child that ends by a signal or at its time limit is a fault or a hang: the
    remaining groups of the file are skipped and the cause is to be found by reading the code.
(3) DOTSOCP_DEVICE_CACHE_GB, the one switch no other test names, and the per-device accounting of the cache.

Findings and the table of non-zeroed allocation sites: DESIGN.md section 5, "Uninitialised device memory"."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dotsocp_amd import capi

import poison_battery as PB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x7ff8bad0bad0bad0                 # csrc/solver.h: POISON_WORD
GUARD_PATTERN = 0x7ff8dead5afe0bad          # csrc/guard.hip: PATTERN
# seconds a child may take.  Measured on the MI355X: every group spends 0.2 .. 1.1 s between its first
# and its last scenario, and a child lives for about 2 s with the imports and the oracle's CPU runs of the generic cases;
# the limits leave room for a cold start (first load of the code objects, a busy host), not for a slower battery -- a
# group that needs more than about 20 s on the device is to be split, not given a longer limit
LIMITS = {"loops-generic": 60, "loops-unpitched": 60, "loops-pitch0": 45, "slabs-tri": 60, "slabs-dct": 60, "post-solve": 45,
          "drivers": 45, "operators": 45, "operators-long": 45}
_STRIPPED = ("DOTSOCP_POISON", "DOTSOCP_CANARY", "DOTSOCP_PITCH", "DOTSOCP_DEVICE_CACHE", "DOTSOCP_DEVICE_CACHE_GB",
             "DOTSOCP_DCT_LONG_MIN", "DOTSOCP_CDFT_LONG_MIN", "DOTSOCP_STRESS_STREAMS")
_fault = []                                 # the group whose child ended by a signal or at its time limit


def _child(code, env, args, limit):
    """the finished fresh process; a fault (signal, abort, illegal access) or the time limit is recorded in _fault"""
    e = {k: v for k, v in os.environ.items() if k not in _STRIPPED}
    e["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    e.update(env)
    try:
        out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")] + list(args), env=e, cwd=ROOT,
                             capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as t:
        _fault.append((args, env, "time limit of %d s" % limit))
        pytest.fail("the child %s %s hung (time limit %d s): a hang, not a test failure -- find the cause by reading the code\n%s"
                    % (args, env, limit, (t.stdout or b"")[-2000:]))
    # (a signal seen by a shell comes back as 128 + n; a device fault that HIP reports as an error ends the child with an
    # exception instead, but the device has faulted all the same)
    fault = out.returncode < 0 or out.returncode in (134, 139) or "illegal memory access" in out.stderr + out.stdout
    if fault:
        _fault.append((args, env, "exit status %d" % out.returncode))
        pytest.fail("the child %s %s faulted (exit status %d): a fault, not a test failure -- find the cause by reading the code\n%s\n%s"
                    % (args, env, out.returncode, out.stdout[-2000:], out.stderr[-3000:]))
    return out


def _peek(n):
    a = np.full(n, 1.5)
    capi.check(capi.lib().dotsocp_debug_alloc_peek(n, a.ctypes.data))
    return a.view(np.uint64)


def _liveness_child():
    L = capi.lib()
    assert os.environ.get("DOTSOCP_POISON") == "1"
    guarded = os.environ.get("DOTSOCP_CANARY") == "1"
    n = 1000
    L.dotsocp_release_cache()
    fresh = _peek(n)                                           # a fresh block (into the cache when it is freed)
    reused = _peek(n)                                          # ... handed out again (no cache under guard bands: fresh again)
    held = L.dotsocp_release_cache()
    after = _peek(n)                                           # fresh again
    for name, a in (("fresh", fresh), ("reused", reused), ("after release_cache", after)):
        bad = np.flatnonzero(a != np.uint64(POISON))
        assert bad.size == 0, "%s: %d of %d slots are not the poison word, first %d: %#x" % (name, bad.size, n, bad[0], a[bad[0]])
    assert np.all(np.isnan(fresh.view(np.float64))) and POISON != GUARD_PATTERN
    if guarded:
        assert held == 0 and L.dotsocp_canary_check() == 0, L.dotsocp_last_error().decode()
    else:
        assert held >= 8 * n, held                             # the second peek did come from the cache
    # a lone allocation of another size, odd and tiny
    assert np.all(_peek(1) == np.uint64(POISON)) and np.all(_peek(33) == np.uint64(POISON))
    # the switch is read per call: off again, nothing is poisoned
    os.environ["DOTSOCP_POISON"] = "0"
    assert not np.any(_peek(n) == np.uint64(POISON)) or guarded
    print("child ok")


_LIVENESS = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_poison as T; T._liveness_child()"


def test_poison_fills_fresh_released_and_reused_blocks():
    out = _child(_LIVENESS, dict(DOTSOCP_POISON="1"), [], 45)
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), out.stdout[-1000:] + out.stderr[-3000:]


def test_poison_fills_the_payload_between_guard_bands():
    out = _child(_LIVENESS, dict(DOTSOCP_POISON="1", DOTSOCP_CANARY="1"), [], 45)
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), out.stdout[-1000:] + out.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------
# the battery
# ---------------------------------------------------------------------------------------------------------------------
_BATTERY = "import sys; sys.path.insert(0, sys.argv[1]); import poison_battery as B; B.run_group(sys.argv[2])"


def _run_group(group, poison):
    env = dict(PB.GROUP_ENV.get(group, {}))
    if poison:
        env["DOTSOCP_POISON"] = "1"
    out = _child(_BATTERY, env, [group], LIMITS[group])
    lines = [json.loads(s) for s in out.stdout.splitlines() if s.startswith("{")]
    print("\n%s, %s: exit %d" % (group, "poisoned" if poison else "plain", out.returncode))
    for ln in lines:
        if "scenario" in ln:
            print("  %-60s %6.2f s  launches %s  non-finite %d" % (ln["scenario"], ln["seconds"], ln["launches"],
                                                                   sum(ln["nonfinite"].values())))
        else:
            print("  group %s: %.2f s in the child" % (ln["group"], ln["seconds"]))
    assert out.returncode == 0, "%s (%s) failed:\n%s\n%s" % (group, env, out.stdout[-2000:], out.stderr[-3000:])
    scenarios = [ln for ln in lines if "scenario" in ln]
    assert lines and "group" in lines[-1] and scenarios, out.stdout[-2000:]
    return scenarios


@pytest.mark.parametrize("group", list(PB.GROUPS))
def test_poisoned_memory_changes_no_bit(group):
    if _fault:
        pytest.skip("an earlier child faulted or hung (%s): its cause comes first" % (_fault[0],))
    plain = _run_group(group, False)
    poisoned = _run_group(group, True)
    assert [s["scenario"] for s in plain] == [s["scenario"] for s in poisoned]
    problems = []
    for a, b in zip(plain, poisoned):
        name = a["scenario"]
        assert sorted(a["sha256"]) == sorted(b["sha256"]), name
        assert a["launches"] == b["launches"], name
        differ = [k for k in sorted(a["sha256"]) if a["sha256"][k] != b["sha256"][k]]
        if differ:
            problems.append("%s: poisoned memory changed %s (first non-finite entries: %s)" % (name, differ, b["first_nonfinite"]))
        for run, tag in ((a, "plain"), (b, "poisoned")):
            bad = {k: n for k, n in run["nonfinite"].items() if n}
            if bad and name != PB.NAN_ON_PURPOSE:
                problems.append("%s (%s): non-finite results %s, first at %s" % (name, tag, bad, run["first_nonfinite"]))
    assert not problems, "\n".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# the cap of the device block cache
# ---------------------------------------------------------------------------------------------------------------------
_CAP = "import sys; sys.path.insert(0, sys.argv[1]); import poison_battery as B; B.cache_cap_child('%s')"


def _cap_child(env, what="solve"):
    if _fault:
        pytest.skip("an earlier child faulted or hung (%s): its cause comes first" % (_fault[0],))
    out = _child(_CAP % what, env, [], 45)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    lines = [json.loads(s) for s in out.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, out.stdout[-1000:]
    return lines[0]


def test_device_cache_cap():
    """DOTSOCP_DEVICE_CACHE_GB (read once per process): after 40 x 40 x 12 was solved twice, as
    tests/test_gpu_errors.py::test_device_buffers_of_destroyed_contexts_are_reused solves it, the cache gives back at most
    1e6 bytes under a cap of 0.001 GB and nothing under a cap of 0; the fields are those of the default cap, bit for bit"""
    default, small, none = _cap_child({}), _cap_child(dict(DOTSOCP_DEVICE_CACHE_GB="0.001")), _cap_child(dict(DOTSOCP_DEVICE_CACHE_GB="0"))
    print("released: default cap %d, 0.001 GB %d, 0 GB %d" % (default["released"], small["released"], none["released"]))
    assert default["released"] > 8 * 40 * 40 * 12 * 27            # (the bar of the test named above: the cache was in use)
    assert 0 <= small["released"] <= 1e6
    assert none["released"] == 0
    for run in (default, small, none):
        assert sum(run["nonfinite"].values()) == 0
        assert any(k.startswith("solve1.") for k in run["sha256"])
        assert run["sha256"] == default["sha256"]


def test_device_cache_is_counted_per_device():
    """Two devices, a cap of 0.002 GB: what device 1 frees is counted against device 1's cap and evicts nothing of device 0
    (the cache once summed the blocks of all devices against one cap).  A destroyed 32 x 32 x 8 context leaves more than
    the cap behind and its largest buffer is under 0.8e6 bytes, so each device then holds between 1.2e6 and 2e6 bytes."""
    if capi.lib().dotsocp_device_count() < 2:
        pytest.skip("needs two devices")
    got = _cap_child(dict(DOTSOCP_DEVICE_CACHE_GB="0.002"), "two_devices")
    h0, h0_after, h1, total = got["held0"], got["held0_after"], got["held1"], got["held_all"]
    print("device 0 holds %d, after device 1's context %d; device 1 holds %d; all %d" % (h0, h0_after, h1, total))
    assert 1.2e6 < h0 <= 2e6 and 1.2e6 < h1 <= 2e6
    # (summed against one cap, device 1's 3 MB would have pushed every older block of device 0 out)
    assert 1.2e6 < h0_after <= 2e6 and total == h0_after + h1 > 2e6
