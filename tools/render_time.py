#!/usr/bin/env python3
"""What six pictures of a solve cost, on the host and on the device.  One process, one context on an ny x nx x nt grid
(default 1024 x 1024 x 128) after a short inPALM run; then, as same-run pairs (one warm-up pair, then --reps timed pairs, the
two ways alternating):
  (a) ctx.outputs() (six grid-sized fields over the host link) + the numpy twin render.render / render.movement of them;
  (b) ctx.render(num_frame=6, arrows=True): one range pass over alpha0 on the device, two alpha layers per frame, the pictures
      and the arrow nodes back.
Every step ends in a device synchronise of its own (the C calls return after sync_all()), so host clocks around them measure
the work.  The pictures and arrows of the last pair are compared byte for byte.
usage: python tools/render_time.py [--grid NY NX NT] [--iters K] [--reps R] [--mode imshow|inverted|levels] [--rgb]
                                   [--out profiles/render_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import render as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", nargs=3, type=int, default=[1024, 1024, 128])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--mode", default="imshow", choices=sorted(R.MODES))
ap.add_argument("--rgb", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "render_time.txt"))
args = ap.parse_args()
ny, nx, nt = args.grid
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


rho0, rho1 = D.get_example_2d("example1", nx, ny)
var, model = D.initialize(rho0, rho1, nt, lazy_zeros=True)
D.InitialScaling(var, model, True, None, dim=2)
ctx = D.InPALMContext(var, dict(tau=1.9, sigma=1.0, tol=0.0, maxit=args.iters, scaling=True), model)
try:
    ctx.run(-1)
    ctx.finish(download=False)
    lut = R.gray_lut() if args.rgb else None
    sy, sx = R.movement_skips(ny, nx)
    kw = dict(num_frame=6, mode=args.mode, lut=lut)
    out_bytes = 8 * ny * nx * (3 * nt + 3 * (nt - 1))
    pic_bytes = 6 * ny * nx * (3 if args.rgb else 1) + 6 * 2 * 8 * (-(-ny // sy)) * (-(-nx // sx))
    say(f"{ny} x {nx} x {nt} after {args.iters} inPALM iterations; six frames, mode {args.mode}, {'RGB' if args.rgb else 'gray'}, "
        f"arrows every ({sy}, {sx}) nodes")
    say(f"over the host link: outputs {out_bytes / 1e9:.2f} GB, pictures and arrows {pic_bytes / 1e6:.2f} MB; read on the device by "
        f"render(): {8 * ny * nx * (nt - 1) / 1e9:.2f} GB (range pass) + {6 * 2 * 8 * ny * nx / 1e6:.0f} MB (frames)")
    ta, tb = [], []
    for rep in range(-1, args.reps):
        t0 = time.perf_counter()
        out = ctx.outputs()
        t1 = time.perf_counter()
        twin = R.render(out, **kw)
        mv = R.movement(out, twin["nodes"], twin["vmax"], sy, sx)
        t2 = time.perf_counter()
        dev = ctx.render(arrows=True, **kw)
        t3 = time.perf_counter()
        if rep >= 0:
            ta.append((t1 - t0, t2 - t1))
            tb.append(t3 - t2)
            say(f"  pair {rep}: outputs() {t1 - t0:7.3f} s + twin {t2 - t1:7.3f} s = {t2 - t0:7.3f} s   |   render() {t3 - t2:8.5f} s")
        if rep < args.reps - 1:
            del out, twin, mv
    same = (np.array_equal(dev["image"], twin["image"]) and dev["vmax"] == twin["vmax"]
            and all(dev[k].tobytes(order="F") == mv[k].tobytes(order="F") for k in mv))
    a = np.array([x + y for x, y in ta])
    b = np.array(tb)
    say(f"median of {args.reps}: outputs() + twin {np.median(a):.3f} s (outputs() alone {np.median([x for x, _ in ta]):.3f} s), "
        f"render() {np.median(b):.5f} s: ratio {np.median(a) / np.median(b):.0f}")
    say(f"pictures and arrows of the two ways: {'identical bytes' if same else 'DIFFERENT'}")
    if not same:
        sys.exit(1)
finally:
    ctx.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
