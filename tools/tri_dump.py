#!/usr/bin/env python3
"""One sha256 per case over the bits of the t-axis tridiagonal kernels (csrc/tri.hip, tri_sweep.h): Poisson solves of
seeded normal right-hand sides through `oper_poisson3dim` (single slab: k_tsolve_single / k_tsolve_pipe, with
DOTSOCP_TS_PIPE=0 as well) and `poisson_on_slabs` (time slabs: k_tri_local / k_tri_reduced / k_tri_final*; one slab:
every k_tsolve_single<R, NSUB> instance).  Two builds that print the same listing compute the same bits.

    python tools/tri_dump.py > listing.txt          (imports the package of the tree the script lies in)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dotsocp_amd as D  # noqa: E402

DSC = 0.37
# (shape, dim, layouts) of tests/test_gpu_tri_slabs.py: shapes 1 .. 8 with their slab counts, then the one-slab shapes
SLABS = [((130, 9, 40), 2, [dict(nslabs=1), dict(nslabs=2), dict(nslabs=3), dict(nslabs=12), dict(nslabs=20), dict(ngpu=2)]),
         ((66, 10, 80), 2, [dict(nslabs=2)]), ((66, 10, 140), 2, [dict(nslabs=2)]),
         ((34, 6, 512), 2, [dict(nslabs=1), dict(nslabs=2), dict(nslabs=4)]), ((34, 6, 514), 2, [dict(nslabs=2)]),
         ((2048, 1, 512), 1, [dict(nslabs=2), dict(nslabs=4)]), ((2048, 4, 340), 2, [dict(nslabs=2)]),
         ((2048, 4, 262), 2, [dict(nslabs=2)])]
SLABS += [((66, 5, nt), 2, [dict(nslabs=1)]) for nt in (5, 12, 23, 49, 100, 133, 200, 270, 500)]
SLABS += [((514, 3, 200), 2, [dict(nslabs=1)]), ((2048, 1, 505), 1, [dict(nslabs=1)])]
# oper_poisson3dim: the grids of test_tridiagonal_t_solve_flavours_agree, each with and without the persistent kernel
OPER = [(512, 512, 72), (1024, 512, 128), (514, 520, 129), (512, 512, 133), (512, 512, 136)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def main():
    ndev = D.capi.lib().dotsocp_device_count()
    for k, (shape, dim, layouts) in enumerate(SLABS):
        rhs = np.asfortranarray(np.random.default_rng(100 + k).standard_normal(shape))
        for kw in layouts:
            tag = "poisson_on_slabs %dx%dx%d %s" % (shape + ("-".join("%s%d" % kv for kv in kw.items()),))
            if kw.get("ngpu", 1) > ndev:
                print("%-50s not run: %d device(s)" % (tag, ndev), flush=True)
                continue
            print("%-50s %s" % (tag, sha(D.poisson_on_slabs(rhs, DSC, dim=dim, **kw))), flush=True)
    for k, shape in enumerate(OPER):
        rhs = np.asfortranarray(np.random.default_rng(200 + k).standard_normal(shape))
        for pipe in ("1", "0"):
            os.environ["DOTSOCP_TS_PIPE"] = pipe           # read per call
            print("%-50s %s" % ("oper_poisson3dim %dx%dx%d TS_PIPE=%s" % (shape + (pipe,)),
                                sha(D.oper_poisson3dim(DSC ** 2, rhs))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
