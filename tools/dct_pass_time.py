#!/usr/bin/env python3
"""Driver for per-pass DCT timings: `rocprofv3 --kernel-trace --stats -- python tools/dct_pass_time.py N [LINES0 LINES1 REPS [AXES]]`
transforms an N x LINES0 x LINES1 array (length N along the contiguous axis) and a LINES0 x N x LINES1 array (length N
along a strided axis), each once to warm up and then REPS times forward and inverse.  AXES = 0 or 1 keeps one of the two
arrays (the two-level kernels of csrc/dct_long.hip carry the same names on both axis kinds: one trace per axis).  The kernel table of the trace then
holds the pass along N per axis kind (k_cdft<T, axis0, inverse, rader> / k_dct_mfma_split<axis0, ...>); run it once per
setting of DOTSOCP_CDFT / DOTSOCP_CDFT_MIN.  Prints the algorithm in use and the host time per call (copies included)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402


def main():
    n = int(sys.argv[1])
    l0, l1, reps = (int(v) for v in (sys.argv[2:5] + ["512", "64", "3"][len(sys.argv) - 2:]))
    rng = np.random.default_rng(n)
    axes = sys.argv[5] if len(sys.argv) > 5 else "01"
    for shape in [s for ax, s in enumerate(((n, l0, l1), (l0, n, l1))) if str(ax) in axes]:
        a = np.asfortranarray(rng.standard_normal(shape))
        D.mirt_idctn(D.mirt_dctn(a))
        t = time.perf_counter()
        for _ in range(reps):
            D.mirt_dctn(a)
            D.mirt_idctn(a)
        print(f"n={n} {D.dct_algorithm(n)} levels={[D.dct_levels(m, ax) for ax, m in enumerate(shape)]} shape={shape}: {(time.perf_counter() - t) / (2 * reps) * 1e3:.1f} ms per call on the host")


if __name__ == "__main__":
    main()
