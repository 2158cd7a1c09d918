"""Host side of the weight pyramid: level sizes (dotsocp_weights_len, no device), SpaceWeight against the Nq generators,
the weights / transfer argument rules of solver_wdotsocp2d."""
import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import capi
from dotsocp_amd.solvers import _weights_mode
from dotsocp_amd.weights import weights_len
from oracle.examples import gene_barrier_of_circle_pillar, get_weight_by_barrier


def nq(ny, nx, nt):
    return ny * nx * (nt - 1) + ny * (nx - 1) * nt + (ny - 1) * nx * nt


def test_weights_len_closed_form():
    for (ny, nx, nt), levels in [((33, 17, 9), 3), ((1025, 1025, 129), 4), ((9, 33, 17), 2), ((3, 3, 3), 2),
                                 ((24, 40, 12), 1), ((13, 7, 11), 2)]:
        for lv in range(levels):
            k = 2 ** (levels - 1 - lv)
            dims = [(n - 1) // k + 1 for n in (ny, nx, nt)]
            assert weights_len(ny, nx, nt, levels, lv) == nq(*dims), (ny, nx, nt, levels, lv)
        assert weights_len(ny, nx, nt, levels, -1) == -1 and weights_len(ny, nx, nt, levels, levels) == -1
    assert weights_len(33, 17, 9, 4, 3) == nq(33, 17, 9)       # three halvings: 9 -> 5 -> 3 -> 2
    assert weights_len(33, 17, 9, 5, 4) == -1                  # ... and 2 cannot be halved
    assert weights_len(32, 17, 9, 2, 1) == -1                  # an even length below the coarsest level
    assert weights_len(33, 17, 11, 3, 2) == -1                 # 11 -> 6 -> ?
    assert weights_len(33, 17, 9, 0, 0) == -1
    assert weights_len(33, 1, 9, 1, 0) == -1 and weights_len(33, 17, 1, 1, 0) == -1


@pytest.mark.parametrize("ny,nx,nt", [(9, 17, 5), (16, 12, 7), (33, 33, 17)])
def test_space_weight_expands_to_the_nq_generators(ny, nx, nt):
    barrier = gene_barrier_of_circle_pillar()
    sw = D.get_space_weight_by_barrier(nx, ny, barrier)
    assert sw.weightX.shape == (ny, nx - 1) and sw.weightY.shape == (ny - 1, nx)
    assert sw.weightX.flags.f_contiguous and sw.weightY.flags.f_contiguous
    w = sw.expand(nt)
    assert w.size == nq(ny, nx, nt)
    np.testing.assert_array_equal(w, get_weight_by_barrier(nx, ny, nt, barrier))        # the oracle's restatement
    np.testing.assert_array_equal(w, D.get_weight_by_barrier(nx, ny, nt, barrier))
    np.testing.assert_array_equal(D.get_space_weight_by_barrier(nx, ny, barrier, 50.0).expand(nt),
                                  get_weight_by_barrier(nx, ny, nt, barrier, 50.0))
    for space, full in ((D.gene_space_weight_circle, D.gene_weight_circle),
                        (D.gene_space_weight_circleInv, D.gene_weight_circleInv)):
        s = space(nx, ny)
        np.testing.assert_array_equal(s.expand(nt), full(nt, nx, ny))
        # gene_weight_circle.m: both edge families normalised with ny (nx - 1), ones on the time edges
        np.testing.assert_allclose(s.weightX.sum(), ny * (nx - 1), rtol=1e-13)
        np.testing.assert_allclose(s.weightY.sum(), ny * (nx - 1), rtol=1e-13)
        assert np.all(s.expand(nt)[:ny * nx * (nt - 1)] == 1.0)
    bx = w[ny * nx * (nt - 1):ny * nx * (nt - 1) + ny * (nx - 1) * nt].reshape((ny, nx - 1, nt), order="F")
    for t in range(nt):
        np.testing.assert_array_equal(bx[:, :, t], sw.weightX)


def test_space_weight_shapes_are_checked():
    with pytest.raises(ValueError):
        D.SpaceWeight(np.ones((5, 4)), np.ones((5, 5)))
    with pytest.raises(ValueError):
        D.SpaceWeight(np.ones(5), np.ones(5))


def test_weights_argument_rules():
    sw = D.SpaceWeight(np.ones((5, 4)), np.ones((4, 5)))
    arr = sw.expand(3)
    assert _weights_mode(arr, None, "device") == "host"            # no existing call changes
    assert _weights_mode(arr, None, "host") == "host"
    assert _weights_mode(sw, None, "device") == "device"
    assert _weights_mode(sw, None, "host") == "host"               # expanded on the host
    assert _weights_mode(arr, "device", "device") == "device"
    assert _weights_mode(sw, "host", "device") == "host"
    for bad in (dict(weights="device", transfer="host"), dict(weights="gpu", transfer="device")):
        with pytest.raises(ValueError):
            _weights_mode(sw, bad["weights"], bad["transfer"])
    # the driver refuses before it touches a device
    rho = np.ones((5, 5))
    with pytest.raises(ValueError, match="transfer='device'"):
        D.solver_wdotsocp2d(rho, rho, 3, 1, dict(tol=1e-3, weight=sw), weights="device", transfer="host")
    with pytest.raises(ValueError):
        D.solver_wdotsocp2d(rho, rho, 3, 1, dict(tol=1e-3, weight=arr), weights="pyramid")


def test_initial_scaling_takes_the_mean_from_the_pyramid():
    """A model without `weight` carries the level's mean(log10(weight + 1e-10)); the scalars are those of the Nq array"""
    rho0, rho1 = D.get_example_2d("example1", 9, 9)
    w = D.get_weight_by_barrier(9, 9, 5, gene_barrier_of_circle_pillar())
    var_a, model_a = D.initialize(rho0, rho1, 5)
    model_a.weight = w
    D.InitialScaling(var_a, model_a, True, None, dim=2, weighted=True)
    var_b, model_b = D.initialize(rho0, rho1, 5)
    model_b.weight_log10_mean = np.mean(np.log10(w + 1e-10))
    D.InitialScaling(var_b, model_b, True, None, dim=2, weighted=True)
    for k in ("D", "E", "cScale", "dScale"):
        assert getattr(var_a, k) == getattr(var_b, k), k
    assert model_a.normc == model_b.normc and model_a.normd == model_b.normd


@pytest.mark.skipif(capi.lib().dotsocp_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_pyramid_without_a_gpu():
    L = capi.lib()
    assert L.dotsocp_weights_create(0, 9, 9, 5, 2) is None
    assert b"no HIP device" in L.dotsocp_last_error()
    with pytest.raises(capi.DotsocpError) as e:
        D.WeightPyramid(9, 9, 5, 2)
    assert e.value.code == -2                                  # DOTSOCP_ENODEVICE
    with pytest.raises(capi.DotsocpError) as e:
        D.WeightPyramid(9, 8, 5, 2)                            # the grid is checked first
    assert e.value.code == -1
