"""Helper of test_gpu_schur_trees.py (run as a subprocess: the route switches are read once per process).
argv: input .npz, output .npz, handle options as JSON, design names of schur_trees.DESIGNS.  Every design ("plain" values, its last
root held back as the Schur set, the design's permutation, no amalgamation) is factored in Schur mode; S, the inertias, and r2, the
expanded and the fused solutions of batches of 2 and 5 right-hand sides are written out, and the test compares them with the host
reference.  The input holds "<name>/X2", the x2 the expansion starts from (zeros where it is missing).  A line
"okkt-case: design <name>" on stderr in front of each design separates the OKKT_DEBUG_FRONTS lines of the designs."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
import schur_trees as sct  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402

BATCHES = (2, 5)

if __name__ == "__main__":
    inp, out, opts, names = sys.argv[1], sys.argv[2], json.loads(sys.argv[3]), sys.argv[4:]
    res = {}
    with np.load(inp) as given:
        for name in names:
            d = sct.build(name)
            ns = sct.set_size(d)
            B = ft.rhs(d.n, sct.NRHS)
            X2 = given[f"{name}/X2"] if f"{name}/X2" in given.files else np.zeros((sct.NRHS, ns))
            n1pos = sct.interior_positive(d)
            print(f"okkt-case: design {name}", file=sys.stderr, flush=True)
            h = sct.schur_handle(d, **opts)
            one = sct.device_results(h, d, n1pos, d.n - ns - n1pos, B, X2, batches=BATCHES)
            res.update({f"{name}/{k}": v for k, v in one.items()})
            res[f"{name}/perm"] = h.perm()
            finalize_b(h)
    np.savez(out, **res)
    print("CASE_OK")
