#!/usr/bin/env python3
"""Set-up time of a stitched image problem: eight 512 x 512 pictures to the two n x n densities of the DOTmark stitch
(default n = 2049: stitched 2048 x 2048, then the double resize), by the device call (dotsocp_image_density: uploads, kernels,
one download) and by the numpy twin, alternating.  The pictures are decoded once, outside the timed window (both routes
need them).  Wall time of the call, which ends in a device synchronise and the download; a small call first loads the library
and the code objects.  Also example5's two densities (540 x 530 -> n x n, one picture each).
usage: image_setup_time.py --resources DIR [--type Shapes|ClassicImages] [--runs R] [n ...]   (> profiles/image_setup.txt)"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import images as I  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resources", required=True, help="the directory that holds DOTmark/, centaur.bmp and man.bmp")
ap.add_argument("--type", default="Shapes")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("sizes", nargs="*", type=int)
args = ap.parse_args()
if D.capi.lib().dotsocp_device_count() < 1:
    sys.exit("image_setup_time.py needs a HIP device: there is nothing to measure without one")

t = time.perf_counter()
stitches = I._stitch_images(args.type, None, None, args.resources)
pair = I._example5_images(args.resources)
print(f"decoding ten pictures (imread, host): {time.perf_counter() - t:.3f} s; stitch pictures {stitches[0][0].shape}, type {args.type}")
I.image_density(stitches[0], 33, 33, "stitch4", device=0)
I.image_density([pair[0]], 33, 33, "single", True, device=0)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


for n in args.sizes or [2049]:
    print(f"{n} x {n}:", flush=True)
    for what, sets, layout, rev in (("DOTmark_4stitch, 2 x 4 pictures", stitches, "stitch4", False),
                                    ("example5, 2 x 1 picture", [[p] for p in pair], "single", True)):
        dev_s, twin_s = [], []
        for run in range(args.runs):
            td, dev = timed(lambda: [I.image_density(s, n, n, layout, rev, 0.0, device=0) for s in sets])
            tt, twin = timed(lambda: [I.image_density(s, n, n, layout, rev, 0.0) for s in sets])
            same = all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(dev, twin))
            dev_s.append(td)
            twin_s.append(tt)
            print(f"  {what}, run {run}: device {td * 1e3:9.2f} ms, twin {tt * 1e3:9.2f} ms, same bits: {same}", flush=True)
        print(f"  {what}: device min {min(dev_s) * 1e3:.2f} ms, twin min {min(twin_s) * 1e3:.2f} ms, twin / device {min(twin_s) / min(dev_s):.1f}x",
              flush=True)
