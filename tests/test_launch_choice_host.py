"""(No device needed.)  The host-side answer to "which kernels will this solve launch" (dotsocp_dct_pass_kernel,
dotsocp_tsolve_kernel, dotsocp_row_pitch: capi.poisson_kernels, capi.dct_pass_kernel) on the shapes whose instance the
docstrings of tests/test_gpu_tri_slabs.py and tests/test_gpu_dct_probes.py name.  The launchers switch on the functions
that answer here, so what these tables say is what runs.  The CU count enters the thresholds of the persistent kernels:
the library asks device 0 and assumes 256 CUs where there is none -- the tables below are those of a 256-CU device (an
MI355X), the only other place this runs."""
import dct_probes as P
import test_gpu_tri_slabs as T
from dotsocp_amd import capi


def test_row_pitch():
    """Solver::row_pitch: rows of no multiple of 16 doubles padded to one, rows of a multiple of 256 doubles (from 512 on)
    16 doubles longer, short rows and the rest as they are"""
    L = capi.lib()
    assert [L.dotsocp_row_pitch(n) for n in (9, 16, 66, 130, 256, 257, 512, 768, 1024, 4096, 65536)] == \
        [9, 16, 80, 144, 256, 272, 528, 784, 1040, 4112, 65552]


def test_kernels_of_the_pipelined_mode_probes():
    """rows 32 .. 41 of tests/test_gpu_tri_slabs.py: the whole triple, also where the GPU test claims less"""
    want = {32: ("pow2-pipe", "pow2-pipe"), 33: ("pow2-pipe", "pow2-pipe"), 34: ("pow2-pipe", "other"),
            35: ("pow2-pipe", "pow2-pipe"), 36: ("pow2-pipe", "pow2-pipe"), 37: ("pow2-wg", "pow2-pipe"),
            38: ("pow2-wg", "pow2-wg"), 39: ("pow2-pipe", "pow2-wg"), 40: ("pow2-wg", "pow2-pipe"), 41: ("pow2-long", "none")}
    assert sorted(want) == sorted(T.PIPE_SHAPES) == sorted(T.PIPE_KERNELS)
    for no, (shape, dim) in T.PIPE_SHAPES.items():
        found = capi.poisson_kernels(*shape)
        assert found == want[no] + ("fused-pipe",), (no, shape, found)
        assert all(w is None or w == f for w, f in zip(T.PIPE_KERNELS[no], found))
        assert (dim == 1) == (shape[1] == 1)


def test_smallest_grids_of_the_pipelined_t_pass():
    """each shape of rows 32 .. 38 with half the columns has half the tiles: up to nt = 256 (two workgroups per CU, 1024
    tiles wanted) the pass falls back to k_dct_strided<2, .>; at 512 and 1024 one workgroup fits a CU and 512 tiles still do.
    The 1-D row of the plan keeps CY out of the LDS; nt = 128 on a plane of 16 x 256 tiles of 64 columns is k_tsolve_pipe's."""
    for no in (32, 33, 35, 36):
        ny, nx, nt = T.SHAPES[no][0]
        assert capi.poisson_kernels(ny, nx // 2, nt)[2] == "fused", no
    for no in (37, 38):
        ny, nx, nt = T.SHAPES[no][0]
        assert capi.poisson_kernels(ny, nx // 2, nt)[2] == "fused-pipe" and capi.poisson_kernels(ny, nx // 4, nt)[2] == "fused"
    assert capi.poisson_kernels(65536, 1, 64) == ("pow2-long", "none", "fused")
    assert capi.poisson_kernels(4096, 1, 256)[2] == "fused" and capi.poisson_kernels(8192, 1, 256)[2] == "fused-pipe"
    assert capi.poisson_kernels(1024, 1024, 128) == ("pow2-pipe", "pow2-pipe", "tri-pipe")
    assert capi.poisson_kernels(512, 512, 128)[2] == "tri-pipe"        # 528 x 512 / 64 = 4224 >= 4096 tiles
    assert capi.poisson_kernels(256, 512, 128) == ("pow2-pipe", "pow2-pipe", "fused-pipe")


def test_kernels_of_the_older_mode_probes(monkeypatch):
    """what the docstring of tests/test_gpu_tri_slabs.py says of its single-slab rows"""
    def t(no):
        return capi.poisson_kernels(*T.SHAPES[no][0])[2]
    assert t(1) == "tri" and all(t(no) == "tri" for no in range(10, 30) if T.SHAPES[no][0][2] != 512)
    assert t(9) == "passes"                       # 505 nodes, tsolve_tri_safe = 0: no fused pass for that length
    assert t(30) == "fused" and t(31) == "tri"    # (66, 5, 64): k_dct_strided<2, true>
    assert capi.poisson_kernels(34, 6, 512)[2] == "fused"
    assert capi.poisson_kernels(*T.SHAPES[25][0])[:2] == ("pow2-long", "none")
    monkeypatch.setenv("DOTSOCP_TSOLVE", "dct")   # read per call
    assert t(31) == "fused-pfa" and t(1) == "passes" and t(33) == "fused-pipe"


def test_kernels_of_the_entry_probes():
    """the instance table of tests/test_gpu_dct_probes.py for the powers of two"""
    want = {"pow2-wave": [((8, 9, 1), 0), ((64, 9, 1), 0), ((128, 9, 1), 0), ((1024, 1, 1), 0), ((9, 8, 1), 1), ((9, 64, 1), 1),
                          ((9, 1024, 1), 1), ((3, 3, 8), 2), ((3, 3, 1024), 2), ((10, 8, 1), 1), ((10, 64, 1), 1), ((2, 5, 64), 2)],
            "pow2-wg": [((64, 65, 1), 0), ((512, 9, 1), 0), ((1024, 9, 1), 0), ((2048, 9, 1), 0), ((32, 64, 1), 1),
                        ((10, 1024, 1), 1), ((16, 1024, 1), 1), ((10, 2048, 1), 1), ((2, 8, 1024), 2)],
            "pow2-pipe": P.CASES["fft1-pipe"],
            "pow2-long": [c[:2] for c in P.CASES["fft2"]],
            "other": P.CASES["pfa"] + P.CASES["rader"] + P.CASES["dense"]}
    assert sorted(want["pow2-wave"] + want["pow2-wg"]) == sorted(P.CASES["fft1"])
    for kernel, cases in want.items():
        for shape, axis in (c[:2] for c in cases):
            assert capi.dct_pass_kernel(shape, axis) == kernel, (shape, axis)
    # half the tiles of a pipelined entry probe: the workgroup-wide kernel
    for shape, axis in P.CASES["fft1-pipe"]:
        if axis == 0:
            half = (shape[0], shape[1] // 2, shape[2])
        else:
            half = (shape[0], shape[1], shape[2] // 2) if shape[2] > 1 else (shape[0] // 2, shape[1], shape[2])
        assert capi.dct_pass_kernel(half, axis) == "pow2-wg", (half, axis)
