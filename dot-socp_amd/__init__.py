"""dot-socp_amd: MI355X-native (gfx950, HIP) implementation of the inPALM/ADMM SOCP iteration
loop of chlhnu/DOT-SOCP behind the reference's own entry points.

Import as `import dotsocp_amd` (alias module at the repository root; the directory name
`dot-socp_amd` is not a Python identifier).  The compute path is lib/libdotsocp.so -- there is
no CPU fallback; see include/dotsocp.h for the C ABI and INTEGRATION.md for the MATLAB binding.
"""
from . import advect, capi, dual, geodesic, render, upper  # noqa: F401
from .advect import default_rho_floor, map_report, masses_on_nodes, push_forward, seeds_on_nodes  # noqa: F401
from .capi import cdft_levels, dct_algorithm, dct_levels  # noqa: F401
from .dual import DualBound, dual_bound, hopf_lax  # noqa: F401
from .upper import (PlanMap, UpperBound, barycentric_map, plan_bound, plan_dense, plan_frames, plan_map, sinkhorn_round,  # noqa: F401
                    soft_transform, upper_bound)
from .geodesic import GeodesicProfile, geodesic_profile  # noqa: F401
from .examples import (SpaceWeight, ensure_barrier_validity, gene_barrier_of_circle_pillar,  # noqa: F401
                       gene_barrier_of_love_heart, gene_space_weight_circle, gene_space_weight_circleInv,
                       gene_weight_circle, gene_weight_circleInv, get_example_1d, get_example_2d,
                       get_space_weight_by_barrier, get_weight_by_barrier)
from . import images  # noqa: F401
from .images import (gene_barrier_of_example6, gene_barrier_of_maze14, gene_example5,  # noqa: F401
                     gene_example_DOTmark_4stitch, get_example_from_images, image_density, imread, imresize, rgb2gray)
from .mexops import (dct_axis, mexBFd, mexBFd1d, mexBFdConj, mexBFdConj1d, mexProjSoc, mirt_dctn, mirt_idctn,  # noqa: F401
                     oper_poisson, oper_poisson3dim)
from .model import (InitialScaling, ModelHandle, VarHandle, check_massConservation, initialize,  # noqa: F401
                    initialize_slab, recover_q, recover_RhoE, recoverOrgVar)
from .report import (SolutionReport, hist_negative_density, hist_positive_value, hist_violation_q_1d,  # noqa: F401
                     hist_violation_q_2d, report_edges, solution_report)
from .weights import WeightPyramid  # noqa: F401
from .solvers import (InPALMContext, poisson_on_slabs, solver_dotsocp1d, solver_dotsocp2d, solver_socp_accADMM,  # noqa: F401
                      solver_socp_inPALM, solver_socp_PALM, solver_wdotsocp2d, solver_wsocp_accADMM, solver_wsocp_inPALM)
