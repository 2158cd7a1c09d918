"""ctypes binding of lib/libdotsocp.so (include/dotsocp.h).

There is no CPU fallback: if the shared library is missing this module raises at import of
the first symbol, and every compute entry point returns DOTSOCP_ENODEVICE without a GPU.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdotsocp.so")

i64 = ctypes.c_longlong
dbl = ctypes.c_double
vp = ctypes.c_void_p


class DotsocpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libdotsocp error {code}: {msg}")
        self.code = code


class Problem(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int), ("weighted", ctypes.c_int),
                ("ny", i64), ("nx", i64), ("nt", i64),
                ("D", dbl), ("E", dbl), ("cScale", dbl), ("dScale", dbl),
                ("normc", dbl), ("normd", dbl)]


class Opts(ctypes.Structure):
    _fields_ = [("tau", dbl), ("sigma", dbl), ("tol", dbl), ("maxit", i64),
                ("ifCheckStepByStep", ctypes.c_int), ("checkPrimDualFeas", ctypes.c_int),
                ("scaling", ctypes.c_int), ("time_limit", dbl)]


class Result(ctypes.Structure):
    _fields_ = [("sigma", dbl), ("sigma_internal", dbl), ("cScale", dbl), ("dScale", dbl),
                ("times", dbl * 7), ("iters", i64), ("hist_len", i64), ("stopped", ctypes.c_int),
                ("time_extra", dbl)]


class AccOpts(ctypes.Structure):
    _fields_ = [("restart", i64), ("rho", dbl), ("theta", dbl)]


REPORT_BINS = 49               # DOTSOCP_REPORT_BINS
REPORT_RHO_FLOOR = 1e-8        # DOTSOCP_REPORT_RHO_FLOOR


class Report(ctypes.Structure):
    """dotsocp_report"""
    _fields_ = [("n_nodes", i64), ("n_cells", i64), ("mass_err", dbl), ("neg_err", dbl),
                ("rho_min", dbl), ("rho_neg", i64), ("rho_hist", i64 * REPORT_BINS),
                ("fq_max", dbl), ("fq_pos", i64), ("fq_hist", i64 * REPORT_BINS),
                ("cost", dbl), ("nonfinite", i64)]


GEO_SUMS = 11                  # DOTSOCP_GEO_SUMS


class Geodesic(ctypes.Structure):
    """dotsocp_geodesic"""
    _fields_ = [("nt", i64), ("n_nodes", i64), ("cost", dbl), ("energy_min", dbl), ("energy_max", dbl), ("speed_spread", dbl),
                ("com_defect", dbl), ("momentum_defect", dbl), ("entropy_defect", dbl), ("peak_excess", dbl), ("nonfinite", i64)]


class AdvectOpts(ctypes.Structure):
    """dotsocp_advect_opts"""
    _fields_ = [("n", i64), ("nsub", ctypes.c_int), ("direction", ctypes.c_int), ("rho_floor", dbl)]


class PushOpts(ctypes.Structure):
    """dotsocp_push_opts"""
    _fields_ = [("n", i64), ("nsub", ctypes.c_int), ("direction", ctypes.c_int), ("rho_floor", dbl), ("nf", i64)]


class MapReport(ctypes.Structure):
    """dotsocp_map_report_t"""
    _fields_ = [("n", i64), ("n_clamped", i64), ("n_still", i64), ("mass", dbl),
                ("cost_map", dbl), ("cost_length", dbl), ("cost_action", dbl), ("disp_mean", dbl), ("len_mean", dbl),
                ("disp_max", dbl), ("len_max", dbl), ("detour_max", dbl),
                ("detour_hist", i64 * REPORT_BINS), ("detour_over", i64)]


class RenderOpts(ctypes.Structure):
    """dotsocp_render_opts"""
    _fields_ = [("mode", ctypes.c_int), ("channels", ctypes.c_int), ("nf", i64), ("nlevels", ctypes.c_int),
                ("barrier_index", ctypes.c_int), ("vmax", dbl), ("skip_y", i64), ("skip_x", i64), ("mask_frac", dbl)]


class RenderInfo(ctypes.Structure):
    """dotsocp_render_info"""
    _fields_ = [("vmax", dbl), ("rho_min", dbl), ("nonfinite", i64), ("masked", i64), ("my", i64), ("mx", i64)]


class Dual(ctypes.Structure):
    """dotsocp_dual"""
    _fields_ = [("n_nodes", i64), ("nonfinite", i64), ("mass0", dbl), ("mass1", dbl),
                ("dual_raw", dbl), ("bound_fwd", dbl), ("bound_bwd", dbl), ("bound", dbl),
                ("gap1_max", dbl), ("gap1_min", dbl), ("gap1_mean", dbl),
                ("gap0_max", dbl), ("gap0_min", dbl), ("gap0_mean", dbl), ("map_cost_bwd", dbl)]


class UpperOpts(ctypes.Structure):
    """dotsocp_upper_opts"""
    _fields_ = [("eps_h2", dbl), ("max_sweeps", i64), ("defect_tol", dbl), ("start", ctypes.c_int)]


class Upper(ctypes.Structure):
    """dotsocp_upper"""
    _fields_ = [("n_nodes", i64), ("sweeps", i64), ("zero0", i64), ("zero1", i64), ("nonfinite", i64),
                ("eps", dbl), ("mass0", dbl), ("mass1", dbl), ("upper", dbl), ("cost_kept", dbl), ("cost_fill", dbl),
                ("kept", dbl), ("fill", dbl), ("defect_first", dbl), ("defect_last", dbl)]


class PlanMap(ctypes.Structure):
    """dotsocp_plan_map_t"""
    _fields_ = [("rows", dbl), ("map_cost", dbl), ("spread", dbl), ("cost_rows", dbl), ("disp_mean", dbl), ("disp_max", dbl),
                ("n_clamped", i64), ("unit", dbl)]


class ImageOpts(ctypes.Structure):
    """dotsocp_image_opts"""
    _fields_ = [("ny", i64), ("nx", i64), ("layout", ctypes.c_int), ("reverse", ctypes.c_int), ("lower_bound", dbl)]


RENDER_LINEAR, RENDER_INVERTED, RENDER_LEVELS = 0, 1, 2        # DOTSOCP_RENDER_*
METHOD_INPALM, METHOD_PALM, METHOD_ACCADMM = 0, 1, 2


F_PHI, F_Q, F_ALPHA, F_Z, F_BETA, F_C, F_WEIGHT = range(7)

# every symbol include/dotsocp.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "dotsocp_last_error": (ctypes.c_char_p, []),
    "dotsocp_version": (ctypes.c_char_p, []),
    "dotsocp_device_count": (ctypes.c_int, []),
    "dotsocp_proj_soc": (ctypes.c_int, [vp, vp, i64, i64]),
    "dotsocp_bfd": (ctypes.c_int, [vp, vp, i64, i64, i64, dbl, dbl]),
    "dotsocp_bfd_conj": (ctypes.c_int, [vp, vp, i64, i64, i64, dbl]),
    "dotsocp_bfd1d": (ctypes.c_int, [vp, vp, i64, i64, dbl, dbl]),
    "dotsocp_bfd_conj1d": (ctypes.c_int, [vp, vp, i64, i64, dbl]),
    "dotsocp_oper_poisson": (ctypes.c_int, [vp, vp, i64, i64, i64, dbl]),
    "dotsocp_dctn": (ctypes.c_int, [vp, i64, i64, i64, ctypes.c_int]),
    "dotsocp_dct_axis": (ctypes.c_int, [vp, i64, i64, i64, ctypes.c_int, ctypes.c_int]),
    "dotsocp_proj_soc_dev": (ctypes.c_int, [vp, vp, i64, i64, vp]),
    "dotsocp_bfd_dev": (ctypes.c_int, [vp, vp, i64, i64, i64, dbl, dbl, vp]),
    "dotsocp_bfd_conj_dev": (ctypes.c_int, [vp, vp, i64, i64, i64, dbl, vp]),
    "dotsocp_create": (vp, [ctypes.POINTER(Problem), ctypes.c_int, ctypes.c_int]),
    "dotsocp_create_multi": (vp, [ctypes.POINTER(Problem), ctypes.c_int, ctypes.c_int]),
    "dotsocp_destroy": (None, [vp]),
    "dotsocp_rccl_unique_id": (ctypes.c_int, [vp]),
    "dotsocp_attach_rccl": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int]),
    "dotsocp_slab_range": (ctypes.c_int, [i64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(i64), ctypes.POINTER(i64)]),
    "dotsocp_field_len": (i64, [ctypes.POINTER(Problem), ctypes.c_int]),
    "dotsocp_dct_algorithm": (ctypes.c_int, [i64]),
    "dotsocp_dct_levels": (ctypes.c_int, [i64, ctypes.c_int]),
    "dotsocp_cdft_levels": (ctypes.c_int, [i64]),
    "dotsocp_tsolve_tri_safe": (ctypes.c_int, [i64, i64, i64]),
    "dotsocp_dct_pass_kernel": (ctypes.c_int, [ctypes.c_int, i64, i64, i64, i64, ctypes.c_int]),
    "dotsocp_tsolve_kernel": (ctypes.c_int, [ctypes.c_int, i64, i64, i64, i64]),
    "dotsocp_row_pitch": (i64, [i64]),
    "dotsocp_cone_writes_beta": (ctypes.c_int, [i64, dbl, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, dbl, dbl]),
    "dotsocp_rescale_due": (ctypes.c_int, [i64, ctypes.c_int, dbl, dbl]),
    "dotsocp_qcone_form": (ctypes.c_int, [i64, dbl, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dbl, dbl]),
    "dotsocp_release_cache": (i64, []),
    "dotsocp_upload": (ctypes.c_int, [vp, ctypes.c_int, vp]),
    "dotsocp_upload_layers": (ctypes.c_int, [vp, ctypes.c_int, vp, i64, i64]),
    "dotsocp_download": (ctypes.c_int, [vp, ctypes.c_int, vp]),
    "dotsocp_begin": (ctypes.c_int, [vp, ctypes.POINTER(Opts)]),
    "dotsocp_begin_method": (ctypes.c_int, [vp, ctypes.POINTER(Opts), ctypes.c_int, ctypes.POINTER(AccOpts)]),
    "dotsocp_run": (ctypes.c_int, [vp, i64, ctypes.POINTER(i64)]),
    "dotsocp_recover_outputs": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dotsocp_report_edges": (ctypes.c_int, [vp]),
    "dotsocp_solution_report": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(Report), vp, vp]),
    "dotsocp_geodesic_profile": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(Geodesic), vp, vp, vp]),
    "dotsocp_recover_velocity": (ctypes.c_int, [vp, vp, vp, dbl, vp, vp]),
    "dotsocp_advect_particles": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(AdvectOpts), vp, vp, vp, vp, ctypes.POINTER(i64)]),
    "dotsocp_push_mass": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(PushOpts), vp, vp, vp, vp, vp, ctypes.POINTER(i64),
                                         ctypes.POINTER(dbl), vp]),
    "dotsocp_map_report": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(AdvectOpts), vp, vp, vp, ctypes.POINTER(MapReport),
                                          vp, vp, vp]),
    "dotsocp_render_evolution": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(RenderOpts), vp, vp, vp, vp, vp, vp, vp,
                                                ctypes.POINTER(RenderInfo)]),
    "dotsocp_dual_bound": (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(Dual), vp, vp, vp, vp]),
    "dotsocp_plan_bound": (ctypes.c_int, [vp, vp, i64, i64, vp, ctypes.POINTER(UpperOpts), ctypes.POINTER(Upper), vp, vp, vp, vp,
                                          vp, vp, ctypes.c_int]),
    "dotsocp_plan_map": (ctypes.c_int, [vp, vp, i64, i64, vp, ctypes.POINTER(UpperOpts), ctypes.POINTER(Upper), vp, vp, vp, vp,
                                        vp, vp, ctypes.POINTER(PlanMap), vp, vp, vp, vp, vp, vp, i64, vp, ctypes.c_int]),
    "dotsocp_upper_map": (ctypes.c_int, [vp, vp, vp, vp, ctypes.POINTER(UpperOpts), ctypes.POINTER(Upper), vp, vp, vp, vp, vp, vp,
                                         ctypes.POINTER(PlanMap), vp, vp, vp, vp, vp, vp, i64, vp, vp]),
    "dotsocp_upper_bound": (ctypes.c_int, [vp, vp, vp, vp, ctypes.POINTER(UpperOpts), ctypes.POINTER(Upper), vp, vp, vp, vp,
                                           vp, vp]),
    "dotsocp_jump_next_level": (ctypes.c_int, [vp, vp]),
    "dotsocp_finish": (ctypes.c_int, [vp, ctypes.POINTER(Result)]),
    "dotsocp_get_history": (ctypes.c_int, [vp, vp, vp, vp, vp]),
    "dotsocp_set_profiling": (ctypes.c_int, [vp, ctypes.c_int]),
    "dotsocp_kernel_time": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.POINTER(dbl), ctypes.POINTER(i64)]),
    "dotsocp_canary_check": (ctypes.c_int, []),
    "dotsocp_debug_alloc_peek": (ctypes.c_int, [i64, vp]),
    "dotsocp_debug_cache_held": (i64, [ctypes.c_int]),
    "dotsocp_poisson_phi": (ctypes.c_int, [vp]),
    "dotsocp_synchronize": (ctypes.c_int, [vp]),
    "dotsocp_weights_create": (vp, [ctypes.c_int, i64, i64, i64, ctypes.c_int]),
    "dotsocp_weights_destroy": (None, [vp]),
    "dotsocp_weights_len": (i64, [i64, i64, i64, ctypes.c_int, ctypes.c_int]),
    "dotsocp_weights_set": (ctypes.c_int, [vp, vp]),
    "dotsocp_weights_set_space": (ctypes.c_int, [vp, vp, vp]),
    "dotsocp_weights_restrict": (ctypes.c_int, [vp, ctypes.c_int]),
    "dotsocp_weights_log10_mean": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(dbl)]),
    "dotsocp_weights_download": (ctypes.c_int, [vp, ctypes.c_int, vp]),
    "dotsocp_upload_weight_from": (ctypes.c_int, [vp, vp, ctypes.c_int]),
    "dotsocp_imresize_taps": (ctypes.c_int, [i64, i64]),
    "dotsocp_imresize_table": (ctypes.c_int, [i64, i64, vp, vp, ctypes.POINTER(ctypes.c_int)]),
    "dotsocp_imresize": (ctypes.c_int, [vp, vp, ctypes.c_int, i64, i64, i64, i64, i64, ctypes.c_int]),
    "dotsocp_image_density": (ctypes.c_int, [ctypes.POINTER(ImageOpts), vp, ctypes.c_int, vp, ctypes.c_int]),
}

_lib = None


def _share_torchs_hip_runtime():
    """The PyTorch-ROCm wheel ships its own copy of the HIP runtime (same SONAME as the system one), and whichever copy
    a process loads first serves everything loaded later.  If libdotsocp came first, with the system runtime, a later
    `import torch` would bring a second runtime and find "no ROCm-capable device".  So when torch is installed but not
    yet imported, its copy is loaded here first: libdotsocp then binds to it (same SONAME) and a later `import torch`
    finds its own runtime already in place -- the import order no longer matters.  DOTSOCP_SYSTEM_HIP=1 skips this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("DOTSOCP_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if not spec or not spec.submodule_search_locations:
        return
    for name in ("libamdhip64.so", "libamdhip64.so.7"):
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass
            return


def lib():
    """Load libdotsocp.so (built by `make -C dot-socp_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        _share_torchs_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != 0:
        raise DotsocpError(code, lib().dotsocp_last_error().decode())


def fptr(a):
    """Pointer to a Fortran/C-contiguous float64 numpy array (no copy)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not (a.flags.f_contiguous or a.flags.c_contiguous):
        raise ValueError("expected a contiguous float64 numpy array")
    return a.ctypes.data


def slab_range(nt, world, rank):
    t0, t1 = i64(), i64()
    check(lib().dotsocp_slab_range(nt, world, rank, ctypes.byref(t0), ctypes.byref(t1)))
    return t0.value, t1.value


def rccl_unique_id():
    """128-byte ncclUniqueId for dotsocp_attach_rccl(); call on rank 0 and broadcast to the others."""
    buf = (ctypes.c_ubyte * 128)()
    check(lib().dotsocp_rccl_unique_id(buf))
    return bytes(buf)


DCT_ALGORITHMS = ("none", "fft", "pfa", "rader", "bluestein", "dense")


def dct_algorithm(n):
    """The transform the DCT passes use for an axis of length n: "fft" (power of two), "pfa" (prime-factor lengths),
    "rader" (257), "bluestein" (other lengths up to 1024, and from 4101 up to 2^19 - 1: cdft_levels), "dense" (DCT-matrix product) or "none" (n <= 1).  No device needed."""
    return DCT_ALGORITHMS[lib().dotsocp_dct_algorithm(int(n))]


def dct_levels(n, axis):
    """Passes through memory that the transform of an axis of length n takes along `axis` (0: y, the contiguous one; 1: x;
    2: t): 0 no transform (n <= 1), 1 one pass with the whole line in LDS, 2 the two-level transform for power-of-two
    lines beyond the LDS (from 4096 along y and 16384 along x / t up to 2^20; DOTSOCP_DCT_LONG_MIN lowers the start),
    negative: unsupported.  No device needed."""
    return int(lib().dotsocp_dct_levels(int(n), int(axis)))


DCT_PASS_KERNELS = ("none", "pow2-wave", "pow2-wg", "pow2-pipe", "pow2-long", "other")
TSOLVE_KERNELS = (None, "tri", "tri-pipe", "fused", "fused-pipe", "fused-pfa", "passes")


def poisson_kernels(ny, nx, nt, pitch=None, device=0):
    """Test support: the kernels the Poisson solve of a single slab launches on an ny x nx x nt grid (1-D: (nx1d, 1, nt))
    on HIP device `device`, as (y pass, x pass, t step): two of DCT_PASS_KERNELS and one of TSOLVE_KERNELS.  pitch: doubles
    between rows (default: what a context gives rows of ny doubles; 0: unpitched, as dotsocp_oper_poisson and
    dotsocp_dct_axis run).  The library answers from the functions its launchers switch on (dotsocp_dct_pass_kernel,
    dotsocp_tsolve_kernel); arrays are taken to be 16-byte aligned; without a device 256 CUs are assumed."""
    L = lib()
    ny, nx, nt = int(ny), int(nx), int(nt)
    pitch = int(L.dotsocp_row_pitch(ny)) if pitch is None else int(pitch)
    ky, kx = (L.dotsocp_dct_pass_kernel(int(device), ny, nx, nt, pitch, a) for a in (0, 1))
    kt = L.dotsocp_tsolve_kernel(int(device), ny, nx, nt, pitch)
    for k in (ky, kx, kt):
        check(min(k, 0))
    return DCT_PASS_KERNELS[ky], DCT_PASS_KERNELS[kx], TSOLVE_KERNELS[kt]


def dct_pass_kernel(shape, axis, device=0):
    """Test support: the kernel (one of DCT_PASS_KERNELS) of the DCT pass along `axis` of an unpitched array of `shape`
    = (ny, nx, nt), as dotsocp_dct_axis runs it on HIP device `device`."""
    ny, nx, nt = (int(v) for v in shape)
    k = lib().dotsocp_dct_pass_kernel(int(device), ny, nx, nt, 0, int(axis))
    check(min(k, 0))
    return DCT_PASS_KERNELS[k]


def cdft_levels(n):
    """How the convolution-based transform of a length n runs: 0 no convolution transform (power of two, prime-factor
    length, dense product), 1 Rader / Bluestein with the convolution in LDS, 2 Bluestein with a two-level convolution
    through a scratch array (from 4101, or from DOTSOCP_CDFT_LONG_MIN >= 129, up to 2^19 - 1).  No device needed."""
    return int(lib().dotsocp_cdft_levels(int(n)))
