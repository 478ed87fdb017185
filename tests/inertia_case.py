"""Helper of test_gpu_inertia_designs.py (run as a subprocess: the route switches are read once per process, and a stop flag that
left a wait without an end must kill this process at the test's time limit and not the session).
argv: output .npz, handle options as JSON, mode ("steps" | "definite" | "schur"), design names of inertia_designs.NAMES.

"steps": per design one handle with early_exit = 1 and the attempts 1 .. 6 of the test's docstring in that order, no solve in between
but the refused one behind attempt 1.  The flags and counts of every attempt are written as they come; D, the values of L and a batch
of five solutions of attempt 4 are written, and compared bit for bit (here: one process) with a fresh early_exit = 0 handle and with
the attempts behind it.  Nothing is asserted here: the test holds the record against the oracle's reference."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
import inertia_designs as idn  # noqa: E402
from onephase_jl_amd import _lib as L  # noqa: E402
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP  # noqa: E402

out, opts, mode, names = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3], sys.argv[4:]


def handle(d, sym="symmetric", **o):
    h = linear_solver_HIP(sym, ordering=2, **dict(ft.NO_RELAX, **dict(opts, **o)))
    initialize_b(h)
    h.set_perm(d.perm)
    return h


def solve5(h, n):
    B = ft.rhs(n, 5)
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(B), L.p_f64(X), 5), "okkt_solve")
    return X


def bits(h, n):
    """D, the values of L and five solutions; None when the handle holds no factor (the attempt stopped: the record shows its flag)"""
    try:
        return h.diag(), h.factor_csc().data, solve5(h, n)
    except OkktError:
        return None


def same(a, b):
    return a is not None and b is not None and bool(all(np.array_equal(x, y) for x, y in zip(a, b)))


def attempt(h, A, n, m):
    flag = h.ls_factor_b(A, n, m)
    return [int(flag)] + [int(v) for v in h.inertia]


res, rec = {}, {}
for name in names:
    r = idn.reference(name)
    d = r.design
    print(f"okkt-case: design {name}", file=sys.stderr, flush=True)
    q = {}
    if mode == "steps":
        low, right, late = idn.decided_low(name), (d.npos, d.nneg), (d.npos - 1, d.nneg + 1)
        h0 = handle(d, early_exit=0)
        q["fresh"] = attempt(h0, d.A, *right)
        fresh = bits(h0, d.n)
        finalize_b(h0)
        # counting under this route: the 25 % tolerance and the four boundary matrices (complete counts: early_exit = 0)
        tol25 = idn.quantile_tols(name)[1][0]
        ht = handle(d, early_exit=0, inertia_tol=tol25)
        q["tol25"] = attempt(ht, d.A, *right)
        q["tol25_same_as_fresh"] = same(bits(ht, d.n), fresh)
        finalize_b(ht)
        hb = handle(d, early_exit=0, inertia_tol=idn.T_BOUNDARY)
        q["boundary"] = {kind: attempt(hb, A, *right) for kind, (A, _) in idn.boundary_matrices(name).items()}
        finalize_b(hb)
        h = handle(d, early_exit=1)
        q["s1"] = attempt(h, d.A, *low)                 # first attempt: the host's check only
        try:
            solve5(h, d.n)
            q["s1_solve"] = "solved"
        except OkktError as e:
            q["s1_solve"] = f"refused: {e}"
        q["s2"] = attempt(h, d.A, *low)                 # a retry: the device flag is on
        h2 = handle(d, early_exit=1, inertia_tol=tol25)
        q["s3_before"] = attempt(h2, d.A, *low)
        q["s3"] = attempt(h2, d.A, *right)              # right request, but a quarter of the pivots are zeros: a zero raises the stop
        finalize_b(h2)
        q["s4"] = attempt(h, d.A, *right)               # still a retry: the limits are met exactly
        b4 = bits(h, d.n)
        q["s4_same_as_fresh"] = same(b4, fresh)
        q["s5"] = attempt(h, d.A, *right)               # a first attempt
        q["s5_same_as_s4"] = same(bits(h, d.n), b4)
        q["s6_first"] = attempt(h, d.A, *late)          # decided by the very last pivots only
        q["s6"] = attempt(h, d.A, *late)                # ... as a retry
        q["s6_right"] = attempt(h, d.A, *right)
        q["s6_right_same_as_s4"] = same(bits(h, d.n), b4)
        finalize_b(h)
        if b4 is not None:
            res.update({f"{name}/D": b4[0], f"{name}/Lx": b4[1], f"{name}/X": b4[2]})
    elif mode == "definite":
        # an all-positive copy (|diagonal|: diagonally dominant, so positive definite), first with -t on the first pivot of one leaf
        Apos = idn.set_diagonal(d.A, np.arange(d.n), 0.0)
        Apos.data[Apos.indptr[:-1]] = np.abs(d.A.diagonal())
        leaf = idn.leaf_first_pivots(d)[:1]
        Aneg = idn.set_diagonal(Apos, d.perm[leaf], -idn.T_BOUNDARY)
        h = handle(d, sym="definite", early_exit=1, inertia_tol=idn.T_BOUNDARY)
        q["neg_pivot"] = attempt(h, Aneg, d.n, 0)
        q["clean"] = attempt(h, Apos, d.n, 0)           # a retry whose limits (n, 0) are met exactly
        q["clean_solve_finite"] = bool(np.all(np.isfinite(solve5(h, d.n))))
        finalize_b(h)
    elif mode == "schur":
        ns = d.nodes[-1]["k"]
        n1 = d.n - ns
        h = handle(d, early_exit=1)
        h.set_schur(d.perm[n1:])
        h.set_perm(d.perm)
        h.analyze(d.A)
        n1pos, n1neg = int(np.sum(r.D[:n1] > 0)), int(np.sum(r.D[:n1] < 0))
        m_req = idn.level_prefix_counts(name)[1][1] - int(np.sum(r.D[n1:] < 0)) - 1      # the level-0 pivots of A11, one fewer
        q["want"] = [n1pos, n1neg]
        for key, (n_, m_) in (("low_first", (n1 - m_req, m_req)), ("low_retry", (n1 - m_req, m_req)), ("right_retry", (n1pos, n1neg))):
            q[key] = [int(h.ls_factor_schur(d.A, n_, m_))] + [int(v) for v in h.inertia]
        finalize_b(h)
    else:
        raise SystemExit(f"unknown mode {mode}")
    rec[name] = q
res["record"] = np.array(json.dumps(rec))
np.savez(out, **res)
print("CASE_OK")
