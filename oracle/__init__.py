"""oracle/ -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

CPU restatement (numpy + a small plain-C file) of the inPALM/ADMM SOCP iteration
loop of chlhnu/DOT-SOCP (socp/dot1d, socp/dot2d, socp/wdot2d), each function citing
the reference file:line it follows.

OPERATORS PINNED, LOOP UNPINNED: the five MEX operators of mex_kernels.c equal the
reference's prebuilt binaries bit for bit (run through ref_mex.py; tests/test_ref_operators.py,
tests/golden/ref_operators.npz).  The reference contains no tests, fixtures or golden vectors
for the loop and MATLAB/Octave are not available, so the rest of the restatement is pinned
only by (i) algebraic invariants that any faithful implementation must obey and (ii)
cross-checks against the known answers recorded in SURVEY.md section 8c(iii).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this
package -- as the checker / the reported CPU baseline, never as the product path.
"""
