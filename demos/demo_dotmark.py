#!/usr/bin/env python3
"""Problems given as pictures.  By default Example 5.5 of the paper: the centaur (centaur.bmp) becomes the man (man.bmp),
129 x 129 x 33, 3 levels, inPALM, tol 1e-4 -- the two densities are made from the image files on the device
(dotsocp_image_density through get_example_2d(..., resources=, device=0); dot-socp_amd/images.py) and six pictures of the
evolution are written as PNG files, as demo_evolution.py does.
  --resources DIR   the directory laid out as the reference's examples/dot2d/resources (centaur.bmp, man.bmp, DOTmark/);
                    default: the fixtures of the test suite, which hold the two BMPs and DOTmark/Shapes
  --type ClassicImages | Shapes
                    the reference's DOTmark stitch instead (demo_dot2d.m's default problem with ClassicImages, whose eight
                    files are not shipped here).  ClassicImages are stitched four to a density (DOTmark_4stitch); the binary
                    Shapes overshoot to negative densities in the stitch's double resize (the reference's behaviour,
                    restated), so for them single pictures are used: Shapes/1.png -> Shapes/5.png."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dotsocp_amd as D  # noqa: E402
from dotsocp_amd import render as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resources", default=os.path.join(ROOT, "tests", "golden", "images"))
ap.add_argument("--type", choices=["ClassicImages", "Shapes"])
ap.add_argument("--n", type=int, default=2 ** 7 + 1)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "dotmark_png"))
args = ap.parse_args()

tol, nt, nx, levelN = 1e-4, 2 ** 5 + 1, args.n, 3
if args.type is None:
    name = "example5"
    rho0, rho1 = D.get_example_2d("example5", nx, nx, resources=args.resources, device=0)
elif args.type == "ClassicImages":
    name = "DOTmark_4stitch"
    rho0, rho1 = D.get_example_2d("DOTmark_4stitch", nx, nx, resources=args.resources, DOTmark_type=args.type, device=0)
else:
    name = "shapes_1_to_5"
    shapes = os.path.join(args.resources, "DOTmark", "Shapes")
    rho0, rho1 = D.get_example_from_images(os.path.join(shapes, "1.png"), os.path.join(shapes, "5.png"), nx, nx, device=0)
print(f"{name}: densities {rho0.shape} made on the device, mean {rho0.mean():.15f} / {rho1.mean():.15f}, "
      f"min {min(rho0.min(), rho1.min()):.3g}, max {max(rho0.max(), rho1.max()):.3g}")
asked = [dict(num_frame=6, mode="inverted")]
output, timeML, _, hist = D.solver_dotsocp2d(rho0, rho1, nt, levelN, dict(tol=tol, maxit=3000), "inPALM", render=asked)
os.makedirs(args.out, exist_ok=True)
r = output["render"][0]
for f, node in enumerate(r["nodes"]):
    R.write_png(os.path.join(args.out, "%s_t%02d.png" % (name, node)), r["image"][f])
print(f"{len(r['nodes'])} pictures {r['image'].shape[1:]} at nodes {r['nodes'].tolist()}, scale vmax = {r['vmax']:.6g}, "
      f"iterations per level {[int(x['Iters']) for x in timeML[:-1]]}, KKT(1,3,6) {np.asarray(hist['kkt'])[-1][[0, 2, 5]].max():.2e}")
print("written:", args.out)
