"""Helper of test_gpu_dataflow_fragments.py (run as a subprocess: the switches are read once per process).
argv: output .npz, then designs as <name>:<k>,<c>,<root pivots>,<scatter 0 / 1> (c = 0: one dense front of k pivots).  Factors every
design of tests/front_trees.py's kind ("plain" values, the design's permutation, no amalgamation), solves one right-hand side and
writes D, L (CSC), the inertia and the solution."""
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP  # noqa: E402

out, res = sys.argv[1], {}
for spec in sys.argv[2:]:
    name, shape = spec.split(":")
    k, c, root, scatter = (int(v) for v in shape.split(","))
    d = ft.build([ft.N(k)] if c == 0 else [ft.N(root, 0, ft.N(k, c, scatter=bool(scatter)))])
    h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(h)
    h.set_perm(d.perm)
    h.ls_factor_b(d.A, d.npos, d.nneg)
    Lh = h.factor_csc()
    x = h.ls_solve(ft.rhs(d.n, 1)[0])
    res.update({f"{name}/d": h.diag().copy(), f"{name}/Lp": Lh.indptr, f"{name}/Li": Lh.indices, f"{name}/Lx": Lh.data, f"{name}/x": x,
                f"{name}/inertia": np.array(h.inertia), f"{name}/n": np.array(d.n)})
    finalize_b(h)
np.savez(out, **res)
print("CASE_OK")
