"""Helper of test_gpu_front_shapes.py (run as a subprocess: the route switches are read once per process).
argv: output .npz, handle options as JSON, design names of front_trees.DESIGNS.  Factors every design ("plain" values, the design's
permutation, no amalgamation), solves five right-hand sides in one batch and writes D, L (CSC), the inertia and the solutions;
the test compares them with the oracle.  A line "okkt-case: design <name>" on stderr in front of each design separates the
OKKT_DEBUG_FRONTS lines of the designs."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
from onephase_jl_amd import _lib as L  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP  # noqa: E402

out, opts, names = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3:]
res = {}
for name in names:
    d = ft.build(ft.DESIGNS[name][0])
    print(f"okkt-case: design {name}", file=sys.stderr, flush=True)
    h = linear_solver_HIP("symmetric", ordering=2, **dict(ft.NO_RELAX, **opts))
    initialize_b(h)
    h.set_perm(d.perm)
    h.ls_factor_b(d.A, d.npos, d.nneg)
    Lh = h.factor_csc()
    B = ft.rhs(d.n, 5)
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(B), L.p_f64(X), 5), "okkt_solve")
    res.update({f"{name}/D": h.diag(), f"{name}/Lp": Lh.indptr, f"{name}/Li": Lh.indices, f"{name}/Lx": Lh.data, f"{name}/X": X,
                f"{name}/inertia": np.array(h.inertia), f"{name}/perm": h.perm()})
    finalize_b(h)
np.savez(out, **res)
print("CASE_OK")
