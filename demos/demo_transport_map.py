#!/usr/bin/env python3
"""Where the mass goes: the transport map of Example 5.1 (Gaussian -> Gaussian, 129 x 129 x 33, 3 levels, inPALM,
tol 1e-4), by carrying particles along the solved flow on the device (advect= of the drivers; dot-socp_amd/advect.py).
Seeds: every 4th node where rho0 exceeds the floor max(rho0, rho1) / 100 (the mask of utils/show_movement_2d.m:31).
The two Gaussians are equal and their centres (0.25, 0.75) and (0.75, 0.25) -- along (first, second) array index -- lie
(+0.5, -0.5) apart in (y, x).  On the whole plane the map would be that translation; these Gaussians are wide (variance
0.05: a standard deviation of 0.22) and cut off by the unit square, so only the mass near the centre moves by nearly that
much, and a particle in the far corner has nowhere to go.  Printed: the deviation of the displacement from (+0.5, -0.5)
over all particles, weighted by the mass rho0 they stand for, and over the seeds within 0.1 of the start centre.
After the particles, the mass itself (push= of the drivers): rho0 carried by a particle on every node and deposited on the
grid -- the displacement interpolant next to the Eulerian rho layers -- with its mean distance l1 to rho at t = 1 (the
defect of the map) and half-way, and the check that every frame holds exactly the same number of mass units.
Last, the judgement of the map itself (map_report= and report= of the drivers): what the map realised by the flow costs
(the mass-weighted mean of |end - start|^2), beside the mean squared path length and the kinetic action of the same
particles -- equal for straight paths at constant speed, as an optimal map gives them -- and beside the Eulerian cost of
the solution report.
Beside the particles, the static map (plan_map= of the drivers): the barycentric map of the rounded Sinkhorn plan of the
upper bound, a second map that owes nothing to the march -- its cost and the spread around it (together the certified
upper bound), the mean squared distance map_gap between the particles' end points and T(x), and l1 between the static
displacement interpolant and the Eulerian rho at three time nodes.  The map is a barycentric projection: it is not measure
preserving."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dotsocp_amd as D  # noqa: E402

tol, nt, nx, levelN = 1e-4, 2 ** 5 + 1, 2 ** 7 + 1, 3
rho0, rho1 = D.get_example_2d("example1", nx, nx)
floor = D.default_rho_floor(rho0, rho1)
x0, y0 = D.seeds_on_nodes(nx, nx, stride=4, mask=rho0 > floor)
output, timeML, runHistML, runHist = D.solver_dotsocp2d(rho0, rho1, nt, levelN, dict(tol=tol, maxit=3000), "inPALM",
                                                        advect=dict(x=x0, y=y0, nsub=2, trajectories=True),
                                                        push=dict(stride=1, frames=[0, nt // 2, nt - 1], nsub=2),
                                                        map_report=dict(stride=1, nsub=2), report=True,
                                                        plan_map=dict(max_sweeps=50, frames=[0, nt // 2, nt - 1],
                                                                      compare=dict(stride=1, nsub=2)))
adv = output["advect"]
dev = np.hypot(adv["x"] - x0 - (-0.5), adv["y"] - y0 - 0.5)
print(f"{x0.size} particles (every 4th node with rho0 > {floor:.3g}), {adv['n_clamped']} clamped at the boundary")
print(f"displacement (dy, dx): mean ({np.mean(adv['y'] - y0):+.4f}, {np.mean(adv['x'] - x0):+.4f}), expected (+0.5, -0.5)")
print(f"deviation from the translation: mean {dev.mean():.4f}, worst {dev.max():.4f} ({dev.max() * (nx - 1):.2f} grid cells)")
w = rho0[np.rint(y0 * (nx - 1)).astype(int), np.rint(x0 * (nx - 1)).astype(int)]
print(f"  weighted by rho0: mean {np.sum(w * dev) / np.sum(w):.4f}")
near = np.hypot(y0 - 0.25, x0 - 0.75) <= 0.1
print(f"  {np.count_nonzero(near)} seeds within 0.1 of the start centre: mean {dev[near].mean():.4f}, worst {dev[near].max():.4f}")
mid = nt // 2
print(f"half-way (node {mid}): mean position (y, x) = ({adv['traj_y'][:, mid].mean():.4f}, {adv['traj_x'][:, mid].mean():.4f})")
# and back: the particles at t = 1 return to their seeds along the same flow
back = D.advect.advect({k: output[k] for k in ("rho", "Ex", "Ey")}, adv["x"], adv["y"], nsub=2, direction=-1)
print(f"there and back (host twin, direction -1): worst distance from the seeds {np.hypot(back['x'] - x0, back['y'] - y0).max():.2e}")
# the mass itself: rho0 pushed along the flow and deposited on the grid
push = output["push"]
print(f"pushed rho0 ({push['x'].size} particles, {push['n_clamped']} clamped): l1 against rho at t = 1: {push['l1'][-1]:.4e}, "
      f"at the middle frame (node {push['nodes'][1]}): {push['l1'][1]:.4e} (mean density 1)")
units = push["counts"].sum(axis=(0, 1))
print(f"units of 2^{int(np.log2(push['unit']))} per frame: {units.tolist()}; all equal to the particles' {push['total_units']}: "
      f"{bool(np.all(units == push['total_units']))}")
# how good the map is as a transport map, beside l1 (does it reach rho1?) and the Eulerian cost of the same solve
mr = output["map_report"]
print(f"map report ({mr['n']} particles, mass rho0): cost_map {mr['cost_map']:.6f} <= cost_length {mr['cost_length']:.6f} <= "
      f"cost_action {mr['cost_action']:.6f}; Eulerian cost (solution report) {output['report']['cost']:.6f}")
print(f"  paths: length / displacement - 1 = {mr['cost_length'] / mr['cost_map'] - 1:.2e} in the mean square, worst detour "
      f"{mr['detour_max']:.3e}, {mr['detour_over']} particles more than 10 % longer than straight, {mr['n_still']} never moved; "
      f"speed: action / length^2 - 1 = {mr['cost_action'] / mr['cost_length'] - 1:.2e}")
print(f"  mean displacement {mr['disp_mean']:.4f}, mean path length {mr['len_mean']:.4f}, longest {mr['len_max']:.4f}; "
      f"l1 at t = 1 beside it: {push['l1'][-1]:.4e}")
# the static map of the rounded plan beside the map of the flow
pm = output["plan_map"]
print(f"static map of the plan: map_cost {pm['map_cost']:.6f} + spread {pm['spread']:.6f} = {pm['cost_rows']:.6f} "
      f"(certified upper {pm['upper']['upper']:.6f}); flow's cost_map {mr['cost_map']:.6f}")
print(f"  particles against it ({pm['n']} seeds): map_gap {pm['map_gap']:.4e} (root {np.sqrt(pm['map_gap']) * (nx - 1):.3f} cells), "
      f"worst {np.sqrt(pm['map_gap_max']) * (nx - 1):.3f} cells; {pm['n_clamped']} nodes clamped")
print("  l1 of the static interpolant against rho at nodes " + ", ".join(f"{int(k)}: {v:.4e}" for k, v in zip(pm["nodes"], pm["l1"])))
