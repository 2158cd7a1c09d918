"""Recipe and ctypes loader for the reference's prebuilt MEX operators.

TEST INFRASTRUCTURE (see oracle/__init__.py).  chlhnu/DOT-SOCP ships the five operators of the inPALM hot path
only as x86-64 binaries (socp/{dot1d,dot2d,wdot2d}/utils/mex*.mexa64).  They import nothing from MATLAB but a
few functions of the C Matrix API (mxGetPr / mxGetM / mxGetN / mxGetScalar; the 1-D ones also mxIsDouble,
mxGetNumberOfElements and mexErrMsgIdAndTxt), all of which tests/fake_mx/fake_mx.c provides.

build_ref() copies the binaries out of a reference checkout into oracle/_ref/ (kept out of git) after checking
each against the md5 recorded below, and builds fake_mx.c there twice, once under each soname the binaries
ask for (libmx.so, libmex.so).  The functions below call each binary's mexFunction with the in-place calling
convention of oracle/mexops.py.  They are what tests/golden/make_golden.py records tests/golden/ref_operators.npz
from, and what tests/test_ref_operators.py compares the oracle with.

The binaries keep static state: call them from one thread.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
REF_DIR = os.path.join(_HERE, "_ref")
FAKE_MX = os.path.join(ROOT, "tests", "fake_mx", "fake_mx.c")
ENV = "DOTSOCP_REFERENCE"             # reference checkout; default: reference/ next to the repository

# name -> (path inside the reference checkout, md5).  mexProjSoc is the same file in dot1d, dot2d and wdot2d,
# mexBFd / mexBFdConj are the same in dot2d and wdot2d.
BINARIES = {
    "mexProjSoc": ("socp/dot2d/utils/mexProjSoc.mexa64", "dc08b09de6316b095063ed612598844d"),
    "mexBFd": ("socp/dot2d/utils/mexBFd.mexa64", "42d8dccd958ff986266fb3dabd457dfc"),
    "mexBFdConj": ("socp/dot2d/utils/mexBFdConj.mexa64", "8002b5a155540f621b56fe22dbbc081c"),
    "mexBFd1d": ("socp/dot1d/utils/mexBFd1d.mexa64", "fdb7d40f7013e7a1a6f1cd61d08f29ff"),
    "mexBFdConj1d": ("socp/dot1d/utils/mexBFdConj1d.mexa64", "4672f1008c8ee81e35932314bf0cafbc"),
}
SONAMES = ("libmx.so", "libmex.so")


def reference_dir():
    return os.environ.get(ENV) or os.path.join(os.path.dirname(ROOT), "reference")


def _md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def build_ref():
    """Fill oracle/_ref/ from the reference checkout.  Without a checkout: print one line, touch nothing, return
    False.  A binary whose md5 differs from the recorded one is an error."""
    src = reference_dir()
    paths = {name: os.path.join(src, rel) for name, (rel, _) in BINARIES.items()}
    if not all(os.path.isfile(p) for p in paths.values()):
        print("note: no reference checkout at %s (set %s); oracle/_ref/ left as it is" % (src, ENV))
        return False
    for name, p in paths.items():
        got = _md5(p)
        if got != BINARIES[name][1]:
            raise RuntimeError("%s: md5 %s, expected %s" % (p, got, BINARIES[name][1]))
    os.makedirs(REF_DIR, exist_ok=True)
    for name, p in paths.items():
        shutil.copyfile(p, os.path.join(REF_DIR, name + ".mexa64"))
    for soname in SONAMES:
        subprocess.check_call(["gcc", "-std=c99", "-O1", "-shared", "-fPIC", "-Wl,-soname," + soname,
                               "-o", os.path.join(REF_DIR, soname), FAKE_MX])
    return True


def available():
    """True when oracle/_ref/ holds every binary and both stand-in libraries."""
    files = [n + ".mexa64" for n in BINARIES] + list(SONAMES)
    return all(os.path.isfile(os.path.join(REF_DIR, f)) for f in files)


vp = ctypes.c_void_p
_st = None


class RefError(Exception):
    """A binary raised mexErrMsgIdAndTxt; .id is the error identifier."""

    def __init__(self, ident, msg):
        super().__init__("%s: %s" % (ident, msg))
        self.id = ident


def _load():
    global _st
    if _st is None:
        if not available():
            raise FileNotFoundError("oracle/_ref/ is incomplete: run oracle.ref_mex.build_ref() with a reference checkout")
        # The stand-ins are loaded by path first; the binaries' DT_NEEDED entries then match them by soname.
        # RTLD_DEEPBIND: a binary binds to these copies even if another fake_mx build sits in the global scope
        # (tests/test_gpu_mex_gateways.py loads one with RTLD_GLOBAL), so fmx_call and mexErrMsgIdAndTxt share state.
        mx = ctypes.CDLL(os.path.join(REF_DIR, "libmx.so"))
        mex = ctypes.CDLL(os.path.join(REF_DIR, "libmex.so"))
        for name, res, args in [("fmx_wrap_double", vp, [ctypes.c_size_t, ctypes.c_size_t, vp]), ("fmx_free", None, [vp]),
                                ("fmx_call", ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.c_int,
                                                            ctypes.POINTER(vp)]),
                                ("fmx_error_id", ctypes.c_char_p, []), ("fmx_error_msg", ctypes.c_char_p, [])]:
            f = getattr(mx, name)
            f.restype, f.argtypes = res, args
        mode = os.RTLD_NOW | getattr(os, "RTLD_DEEPBIND", 0)
        fns = {n: ctypes.cast(ctypes.CDLL(os.path.join(REF_DIR, n + ".mexa64"), mode=mode).mexFunction, vp)
               for n in BINARIES}
        _st = (mx, mex, fns)
    return _st


def call(name, args, nlhs=0):
    """Run binary `name` on `args` (Fortran-ordered float64 arrays, aliased so that in-place writes are visible,
    or numbers, passed as 1 x 1 doubles).  Returns None, or the error id the binary raised."""
    mx, _, fns = _load()
    hs, keep = [], []
    try:
        for v in args:
            if isinstance(v, np.ndarray):
                if v.dtype != np.float64 or not v.flags.f_contiguous:
                    raise ValueError("pass Fortran-contiguous float64 arrays (MATLAB layout)")
                m, n = (v.shape[0], v.shape[1]) if v.ndim == 2 else (v.size, 1)
                a = v
            else:
                a = np.array([float(v)])
                m, n = 1, 1
            keep.append(a)
            hs.append(mx.fmx_wrap_double(m, n, a.ctypes.data))
        prhs = (vp * max(len(hs), 1))(*hs)
        plhs = (vp * max(nlhs, 1))()
        rc = mx.fmx_call(fns[name], nlhs, plhs, len(hs), prhs)
        return mx.fmx_error_id().decode() if rc else None
    finally:
        for h in hs:
            mx.fmx_free(h)


def _run(name, args):
    err = call(name, args)
    if err is not None:
        raise RefError(err, _load()[0].fmx_error_msg().decode())


def mexProjSoc(out, inp):
    """mexProjSoc(out, in): rows of the M x K matrix `inp` projected onto the SOC, into `out`."""
    assert out.shape == inp.shape
    _run("mexProjSoc", [out, inp])


def mexBFd(z, q, nt, nx, ny, s, dF):
    """mexBFd(z, q, nt, nx, ny, s, dF).  The 2-D binary reads prhs[5] and prhs[6] whatever nrhs is (so do all the
    reference's call sites pass them): shorter calls would read past the argument list and are not offered."""
    _run("mexBFd", [z, q, nt, nx, ny, s, dF])


def mexBFdConj(q, z, nt, nx, ny, s):
    """mexBFdConj(q, w, nt, nx, ny, s).  Reads prhs[5] whatever nrhs is, like mexBFd."""
    _run("mexBFdConj", [q, z, nt, nx, ny, s])


def mexBFd1d(z, q, nt, nx, *sdF):
    """mexBFd1d(z, q, nt, nx[, s[, dF]])"""
    _run("mexBFd1d", [z, q, nt, nx, *sdF])


def mexBFdConj1d(q, z, nt, nx, *s):
    """mexBFdConj1d(q, w, nt, nx[, s])"""
    _run("mexBFdConj1d", [q, z, nt, nx, *s])
