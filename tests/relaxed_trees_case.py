"""Helper of test_gpu_relaxed_trees.py (run as a subprocess: the route switches are read once per process).
argv: output .npz, handle options as JSON, design names of relaxed_trees.DESIGNS.  Factors every design ("plain" values, the design's
permutation and relaxation options), and writes what the test compares with the oracle and with the model: D, L (CSC), the inertia,
the permutation, five single solves, batches of 1, 4 and 5 right-hand sides, three repeated solves; then other values (seed 1) on
the same handle and on a fresh one.  A line "okkt-case: design <name>" on stderr in front of each design separates the
OKKT_DEBUG_FRONTS lines of the designs."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
import relaxed_trees as rt  # noqa: E402
from onephase_jl_amd import _lib as L  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP  # noqa: E402


def solve_batch(h, B):
    B = np.ascontiguousarray(B)
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(B), L.p_f64(X), B.shape[0]), "okkt_solve")
    return X


def handle(d, o):
    h = linear_solver_HIP("symmetric", ordering=2, **o)
    initialize_b(h)
    h.set_perm(d.perm)
    return h


out, opts, names = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3:]
res = {}
for name in names:
    d, relax, _ = rt.design(name)
    o = dict(relax, **opts)
    print(f"okkt-case: design {name}", file=sys.stderr, flush=True)
    h = handle(d, o)
    h.ls_factor_b(d.A, d.npos, d.nneg)
    Lh = h.factor_csc()
    B = ft.rhs(d.n, 5)
    res.update({f"{name}/D": h.diag(), f"{name}/Lp": Lh.indptr, f"{name}/Li": Lh.indices, f"{name}/Lx": Lh.data,
                f"{name}/inertia": np.array(h.inertia), f"{name}/perm": h.perm(),
                f"{name}/rep": np.array([h.ls_solve(B[0]) for _ in range(3)]), f"{name}/singles": np.array([h.ls_solve(b) for b in B])})
    for nrhs in (1, 4, 5):
        res[f"{name}/X{nrhs}"] = solve_batch(h, B[:nrhs])
    d2 = ft.build(rt.DESIGNS[name][0], seed=1)
    for tag, hh in (("same", h), ("fresh", handle(d, o))):
        hh.ls_factor_b(d2.A, d2.npos, d2.nneg)
        res.update({f"{name}/{tag}/D": hh.diag(), f"{name}/{tag}/Lx": hh.factor_csc().data, f"{name}/{tag}/inertia": np.array(hh.inertia),
                    f"{name}/{tag}/X": solve_batch(hh, B)})
        finalize_b(hh)
np.savez(out, **res)
print("CASE_OK")
