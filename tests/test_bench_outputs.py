"""bench.py --dump-outputs: what the timed run computed, written as .npy files so that two builds can be compared
output for output.  CPU: the writer against a stand-in context (sampling of large fields, size budget, same files on
every call).  GPU: two bench runs of one small grid write identical files, equal to solver_socp_inPALM's results on the
same problem."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phi", "q", "z", "alpha", "beta", "sigma", "scale", "kkt", "kkt_iter")


class _Ctx:
    """download(field, like): a field of like's shape whose values are its column-major positions plus 1e6 * field"""
    def download(self, field, like):
        n = int(np.prod(like.shape))
        return np.asfortranarray((np.arange(n, dtype=np.float64) + 1e6 * field).reshape(like.shape, order="F"))


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}


def test_dump_writes_float64_samples_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    import dotsocp_amd as D
    var = SimpleNamespace(phi=np.zeros(60), nq=500, zshape=(80, 10), cScale=2.5, dScale=0.5)
    hist = {"kkt": np.arange(70.0).reshape((10, 7), order="F"), "iter": np.arange(1.0, 11.0)}
    for d in ("a", "b"):
        bench.dump_outputs(D, _Ctx(), var, hist, 1.75, str(tmp_path / d))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in NAMES:
        assert a[k].dtype == np.float64
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["phi"], np.arange(60.0) + 1e6 * D.capi.F_PHI)      # short: written whole
    for k, f, n in (("q", D.capi.F_Q, 500), ("alpha", D.capi.F_ALPHA, 500), ("z", D.capi.F_Z, 800), ("beta", D.capi.F_BETA, 800)):
        pos = a[k] - 1e6 * f
        assert a[k].shape == (100,) and np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < n
    assert not np.array_equal(a["q"] - 1e6 * D.capi.F_Q, a["alpha"] - 1e6 * D.capi.F_ALPHA)   # one sample per field
    np.testing.assert_array_equal(a["sigma"], [1.75])
    np.testing.assert_array_equal(a["scale"], [2.5, 0.5])
    np.testing.assert_array_equal(a["kkt"], hist["kkt"])
    np.testing.assert_array_equal(a["kkt_iter"], hist["iter"])
    # every field of the default grid is sampled: the files stay under 64 MB whatever the grid
    assert 8 * (5 * bench.DUMP_SAMPLE + 3 + 8 * bench.DUMP_KKT_ROWS) + 9 * 128 < 64e6


@pytest.mark.gpu
def test_bench_dump_is_reproducible_and_equals_the_solver(tmp_path):
    import dotsocp_amd as D
    ny, nx, nt, warmup, steps = 40, 36, 12, 3, 7
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                              str(warmup), "--no-cpu-baseline", "--grid", str(ny), str(nx), str(nt), "--dump-outputs",
                              str(tmp_path / d)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        rec = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(rec) == 1 and '"ms_per_step"' in rec[0]
        dumps.append(_load(tmp_path / d))
    for k in NAMES:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k])
    rho0, rho1 = D.get_example_2d("example1", ny, nx)
    var, model = D.initialize(rho0, rho1, nt)
    D.InitialScaling(var, model, True, None, dim=2)
    hist, sigma = D.solver_socp_inPALM(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=warmup + steps, scaling=True,
                                                 ifCheckStepByStep=False, time_limit=1e9), model)
    got = dumps[0]
    for f in ("phi", "q", "z", "alpha", "beta"):
        want = getattr(var, f)
        assert got[f].shape == want.shape, f
        np.testing.assert_allclose(got[f], want, rtol=0, atol=1e-12 * np.abs(want).max())
    assert abs(got["sigma"][0] - sigma) <= 1e-12 * sigma
    np.testing.assert_array_equal(got["kkt_iter"], hist["iter"])
    np.testing.assert_allclose(got["kkt"], hist["kkt"], rtol=1e-9, atol=1e-14)
