#!/usr/bin/env python3
"""Looking at a solve: Example 5.1 (Gaussian -> Gaussian, 129 x 129 x 33, 3 levels, inPALM, tol 1e-4) and six pictures of its
density at the frame nodes of utils/export_evolution_2d.m, made on the device (render= of the drivers;
dot-socp_amd/render.py) in the three ways the reference's demos look at it:
  imshow    gray, imshow(rho, [0, max])              (show_evolution_2d.m "imshow"), with the arrows of show_movement_2d.m
  inverted  gray, dark where the mass is             (export_evolution_2d.m)
  levels    128 log-spaced filled levels through a colour ramp (show_evolution_2d.m "contourf"; any 256 x 3 table will do)
Only the pictures (6 x 129 x 129 bytes per mode, three times that in colour) and the arrow nodes cross the host link.  The
eighteen PNG files go to --out (default: evolution_png/ beside this script); the arrow field is printed as a summary."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import render as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "evolution_png"))
args = ap.parse_args()

tol, nt, nx, levelN = 1e-4, 2 ** 5 + 1, 2 ** 7 + 1, 3
rho0, rho1 = D.get_example_2d("example1", nx, nx)
ramp = R.ramp_lut([(255, 255, 255), (40, 60, 160), (40, 170, 200), (250, 220, 60), (200, 30, 30)])
asked = [dict(num_frame=6, mode="imshow", arrows=True),
         dict(num_frame=6, mode="inverted"),
         dict(num_frame=6, mode="levels", nlevels=128, lut=ramp)]
output = D.solver_dotsocp2d(rho0, rho1, nt, levelN, dict(tol=tol, maxit=3000), "inPALM", render=asked)[0]
os.makedirs(args.out, exist_ok=True)
for req, r in zip(asked, output["render"]):
    for f, node in enumerate(r["nodes"]):
        R.write_png(os.path.join(args.out, "%s_t%02d.png" % (req["mode"], node)), r["image"][f])
    print(f"{req['mode']:8s}: {len(r['nodes'])} pictures {r['image'].shape[1:]} at nodes {r['nodes'].tolist()}, scale vmax = {r['vmax']:.6g}, "
          f"min rho = {r['rho_min']:.3e}, {r['nonfinite']} non-finite; distinct indices (colours) per frame "
          f"{[len(np.unique(r['image'][f].reshape(-1, 3), axis=0)) if r['image'].ndim == 4 else len(np.unique(r['image'][f])) for f in range(len(r['nodes']))]}")
mv = output["render"][0]
sy, sx = R.movement_skips(nx, nx)
print(f"arrows at every ({sy}, {sx}) nodes: {mv['Ex'].shape[0]} x {mv['Ex'].shape[1]} per frame, zero where rho < vmax / 100")
for f, node in enumerate(mv["nodes"]):
    ex, ey = mv["Ex"][:, :, f], mv["Ey"][:, :, f]
    live = (ex != 0) | (ey != 0)
    n = max(int(np.count_nonzero(live)), 1)
    print(f"  node {node:2d}: {np.count_nonzero(live):4d} arrows, mean flux (Ey, Ex) = ({ey[live].sum() / n:+.4f}, {ex[live].sum() / n:+.4f}), "
          f"longest {np.hypot(ex, ey).max():.4f}")
same = R.render({k: output[k] for k in ("rho", "Ex", "Ey")}, num_frame=6, mode="levels", nlevels=128, lut=ramp)
print("the colour pictures equal the numpy twin's on the downloaded outputs:", bool(np.array_equal(same["image"], output["render"][2]["image"])))
print("written:", args.out)
