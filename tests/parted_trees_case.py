"""Helper of test_gpu_parted_trees.py (run as a subprocess: the route switches are read once per process).
argv: output .npz, handle options as JSON, then an optional "wrong" and the cases of parted_trees.CASES as <design>/<nparts>.
Every case ("plain" values, the design's permutation, no amalgamation, nparts virtual ranks on one device) is factored and two
right-hand sides are solved one at a time; the composed D and L, the summed pivot counts, the solutions and every rank's buffer in
front of each exchange are written out (parted_trees.device_results), and the test compares them with the oracle.  With "wrong" a
factorisation asked for the wrong inertia and, right behind it, the right one follow (parted_trees.wrong_then_right).  A line
"okkt-case: design <design>/<nparts>" on stderr in front of each case separates the OKKT_DEBUG_FRONTS lines of the cases."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
import parted_trees as pt  # noqa: E402

if __name__ == "__main__":
    out, opts, cases = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3:]
    wrong = bool(cases) and cases[0] == "wrong"
    res = {}
    for case in cases[1:] if wrong else cases:
        name, nparts = case.rsplit("/", 1)
        d = pt.build(name)
        B = ft.rhs(d.n, pt.NRHS)
        print(f"okkt-case: design {case}", file=sys.stderr, flush=True)
        sh = pt.sharded(d, int(nparts), **opts)
        one = pt.device_results(sh, d, B)
        one.update({f"info/{k}": np.array(v) for k, v in sh.info.items()})
        one["perm"] = sh.solvers[0].perm()
        if wrong:
            one.update(pt.wrong_then_right(sh, d, B))
        sh.finalize()
        res.update({f"{case}/{k}": v for k, v in one.items()})
    np.savez(out, **res)
    print("CASE_OK")
