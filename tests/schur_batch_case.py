"""Helper of test_gpu_schur_batch.py (run as a subprocess: OKKT_DEBUG_POISON is read when the buffers are allocated).
argv: design names of schur_batch_designs.DESIGNS.  Every design runs case 1 of the device tests -- every item of batches of 1, 3 and
7, as bits, against a fresh single handle in Schur mode -- and the sums of the batch of 7 against the grouping rule."""
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import schur_batch_designs as sbd  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402

if __name__ == "__main__":
    for name in sys.argv[1:]:
        sbd.check_items(name, sizes=(1, 3, 7))
        sc = sbd.scenario(name)
        h = sc.handle()
        h.schur_batch_reserve(7, nrhs_max=3)
        h.ls_factor_schur_batch(sc.vals(7), sc.n1pos, sc.n1neg)
        S = h.schur_batch(-1)
        assert np.isfinite(S).all() and sbd.same(S, sbd.group_sum([h.schur_batch(b) for b in range(7)]))
        rhs = sc.rhs(7, 3)
        r2, r2i = h.schur_batch_condense(rhs, items=True)
        assert np.isfinite(r2).all() and sbd.same(r2, sbd.group_sum(list(r2i)))
        assert h.schur_batch_factor() == 1
        X = h.schur_batch_solve(rhs)
        assert np.isfinite(X).all() and sbd.same(h.schur_batch_expand(rhs, X[0][:, sc.idx]), X)
        finalize_b(h)
    print("CASE_OK")
