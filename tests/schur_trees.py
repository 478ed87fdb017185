"""Schur mode on designed trees: the catalogue of sets and the host reference (shared by test_schur_trees.py, test_gpu_schur_trees.py
and schur_trees_case.py).

A Schur design is a design of front_trees.py whose LAST ROOT is held back: the Schur set is the pivot columns of that root in the
design's own order (`idx = d.perm[d.n - ns:]`), the handle gets `ordering = 2`, `NO_RELAX`, `set_schur(idx)` and `set_perm(d.perm)`.
The interior is then exactly the designed fronts below (and beside) that root and the Schur front is the root itself, k = f = ns: the
analysis reproduces the design unchanged (test_schur_trees.py), so which fronts hand their contribution blocks (CBs) to the Schur
front, and how large the set is, is chosen here and not found by an ordering.

The reference of one (design, values, seed), in the permuted numbering (interior 0 .. n1 - 1, set n1 .. n - 1):

  * S_ref = A22 - A21 X in long double, X the solution of A11 X = A12 column by column (the oracle's factor of A11, refined with
    long-double residuals by front_trees.true_solution); only the set's columns that touch the interior are solved for, the rest of
    S is A22;
  * r2_ref = b2 - A21 x1, x1 = A11^-1 b1 refined in the same way;
  * the true solutions of the whole system (the whole-matrix oracle on the design's permutation, refined);
  * S_oracle = A22 - (L21 D1) L21^T and r2_oracle = b2 - L21 (L11^-1 b1) in fp64 from the whole-matrix oracle factor: the elimination
    of the device in the same order, one summation order.  Their distance from S_ref / r2_ref is the yardstick of the device's.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import front_trees as ft
import oracle
from front_trees import N

NRHS = 5

# the six designs made for Schur mode (the set is the first argument of the last root)
NEW_DESIGNS = {
    "set-65-small-only": ([N(65, 0, N(16, 16), N(17, 16), N(48, 16), N(49, 16, scatter=True), N(100, 28), N(8, 64))],
                          "an interior of small fronts only, every small class at its edge, a CB of ns - 1 rows, the export's tile edge"),
    "set-256": ([N(256, 0, N(20, 255), N(10, 1))], "one block of the gather / put kernels, lcol = 256"),
    "set-257": ([N(257, 0, N(150, 256), N(20, 12))], "one row past the gather / put block and past lcol = 256"),
    "set-2048": ([N(2048, 0, N(129, 2047), N(20, 1))], "the last size of the unchunked assembly"),
    "set-2049-thin": ([N(2049, 0, N(3, 2048, scatter=True), N(2, 1025), N(1, 1024), N(40, 24), N(130, 1100, scatter=True),
                         N(8, 16, N(8, 16)))],
                      "chunked assembly: CBs that end at, one past and two chunks past a 1024-row boundary; small, big and task-chain children"),
    "lone-roots-then-set": ([N(140), N(30, 0, N(20, 10)), N(257, 0, N(150, 256), N(20, 12))],
                            "a big and a small interior tree that never touch the set"),
}


def _nnodes(roots):
    return sum(1 + _nnodes(r.children) for r in roots)


# every design of the front catalogue with more than one node (its last root becomes the set), then the new ones
DESIGNS = {name: v for name, v in ft.DESIGNS.items() if _nnodes(v[0]) > 1}
DESIGNS.update(NEW_DESIGNS)

# the set has no child: every other front belongs to a tree of its own
CHILDLESS = ("mixed-level", "mixed-level-scatter", "forest-3-roots")
IPM_DESIGNS = ["set-65-small-only", "set-257", "set-2049-thin", "fan-in-8", "task-chains-under-big", "edge-k1025-c1"]
VARIANT_DESIGNS = ["set-65-small-only", "task-chains-under-big", "fan-in-8", "set-2049-thin"]

# the set sizes that have to be in the catalogue (test_schur_trees.py holds the catalogue to them)
SET_SIZES = {2, 17, 64, 65, 128, 129, 130, 256, 257, 2048, 2049, 2101}


def build(name, values="plain", seed=0):
    return ft.build(DESIGNS[name][0], values=values, seed=seed)


def set_size(d):
    return d.nodes[-1]["k"]


def set_index(d):
    """the Schur set in the caller's labels: the pivot columns of the last root, in the design's order"""
    return d.perm[d.n - set_size(d):]


def interior_positive(d):
    """the designed number of positive pivots of A11: the signs of its diagonal (both value recipes give every column the sign of
    its diagonal entry; the reference checks this count against the oracle's D)"""
    return int((d.A.diagonal()[d.perm][:d.n - set_size(d)] > 0).sum())


def children_of_set(d):
    """the designed fronts whose CB goes into the Schur front"""
    return [nd for nd in d.nodes if nd["parent"] == len(d.nodes) - 1]


def lone_roots(d):
    """interior fronts without a parent (indices into d.nodes)"""
    return [i for i, nd in enumerate(d.nodes[:-1]) if nd["parent"] is None]


def reached(d):
    """ns x ns mask: entry (i, j) of S lies in the CB of some child of the set.  Every other entry of S is A22, bit for bit."""
    ns = set_size(d)
    n1 = d.n - ns
    m = np.zeros((ns, ns), dtype=bool)
    for nd in children_of_set(d):
        cb = nd["rows"][nd["k"]:] - n1
        m[np.ix_(cb, cb)] = True
    return m


class Ref:
    def __init__(self, **kw):
        self.__dict__.update(kw)


_REF = {}


def reference(name, values="plain", seed=0):
    """The reference of the module docstring; cached: the route variants and the batches reuse it, nobody changes it."""
    key = (name, values, seed)
    if key in _REF:
        return _REF[key]
    d = build(name, values, seed)
    ns = set_size(d)
    n1 = d.n - ns
    M = ft.full_csr(d.A)
    Mp = M[d.perm][:, d.perm].tocsr()          # permuted numbering: interior, then the set
    Mp.sort_indices()
    A11, A21, A22 = Mp[:n1, :n1].tocsr(), Mp[n1:, :n1].tocsr(), Mp[n1:, n1:].toarray()
    o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
    o.ls_factor_b(d.A, d.npos, d.nneg)
    D, Lo = o.diag(), o.L().tocsr()
    B = ft.rhs(d.n, NRHS)
    Bp = B[:, d.perm]
    XT = np.array([ft.true_solution(M, o.ls_solve, b) for b in B])
    # the oracle's own S and r2 (fp64)
    L11, L21 = Lo[:n1, :n1], Lo[n1:, :n1]
    S_or = A22 - ((L21 @ sp.diags(D[:n1])) @ L21.T).toarray()
    if n1 > 0 and L21.nnz:
        Y1 = spla.spsolve_triangular((L11 + sp.identity(n1)).tocsr(), Bp[:, :n1].T.copy(), lower=True, unit_diagonal=True)
        R2_or = Bp[:, n1:] - (L21 @ Y1).T
    else:
        R2_or = Bp[:, n1:].copy()
    # the long-double S and r2
    o1 = oracle.linear_solver_ORACLE("symmetric", perm=np.arange(n1, dtype=np.int64))
    n1pos = int((D[:n1] > 0).sum())
    assert n1pos == interior_positive(d) and not np.any(D == 0)
    o1.ls_factor_b(sp.tril(A11).tocsc(), n1pos, n1 - n1pos)
    A21l = A21.toarray().astype(np.longdouble)
    touch = np.flatnonzero(np.diff(A21.indptr) > 0)
    S_ref = A22.astype(np.longdouble)
    if len(touch):
        A12 = A21[touch].toarray()
        X = np.array([ft.true_solution(A11, o1.ls_solve, a) for a in A12]).astype(np.longdouble)      # one row per column of A12
        S_ref[:, touch] -= A21l @ X.T
    X1 = np.array([ft.true_solution(A11, o1.ls_solve, b) for b in Bp[:, :n1]]).astype(np.longdouble)
    R2_ref = Bp[:, n1:].astype(np.longdouble) - X1 @ A21l.T
    S64, R264 = S_ref.astype(np.float64), R2_ref.astype(np.float64)
    smax, rmax = float(np.max(np.abs(S_ref))), float(np.max(np.abs(R2_ref)))
    r = Ref(name=name, d=d, ns=ns, n1=n1, idx=set_index(d), n1pos=n1pos, n1neg=n1 - n1pos, M=M, B=B, XT=XT, A22=A22, S_ref=S_ref, R2_ref=R2_ref,
            S64=S64, R264=R264, smax=smax, rmax=rmax, S_oracle=S_or, R2_oracle=R2_or,
            e_oracle_S=float(np.max(np.abs(S_or - S_ref)) / smax), e_oracle_r2=float(np.max(np.abs(R2_or - R2_ref)) / rmax),
            X2=np.linalg.solve(S64, R264.T).T.copy(),
            e_oracle_solve=max(ft.fwd_err(o.ls_solve(b), xt) for b, xt in zip(B, XT)), reached=reached(d), eig=np.linalg.eigvalsh(S64))
    _REF[key] = r
    return r


def schur_handle(d, **opts):
    """an analysed Schur-mode handle of the design"""
    from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP
    h = linear_solver_HIP("symmetric", ordering=2, **dict(ft.NO_RELAX, **opts))
    initialize_b(h)
    h.set_schur(set_index(d))
    h.set_perm(d.perm)
    h.analyze(d.A)
    return h


def device_results(h, d, n1pos, n1neg, B, X2, batches=(NRHS,)):
    """What one factorisation in Schur mode gives: flag, inertias, S, and per batch size r2, the expanded x (from X2) and the fused x."""
    res = {"flag": np.array(h.ls_factor_schur(d.A, n1pos, n1neg)), "inertia": np.array(h.inertia), "S": h.schur()}
    res["sflag"] = np.array(h.schur_factor())
    res["schur_inertia"], res["total_inertia"] = np.array(h.schur_inertia), np.array(h.total_inertia)
    res["S_after"] = h.schur()
    for nr in batches:
        res[f"r2/{nr}"] = h.schur_condense(B[:nr]).reshape(nr, -1)
        res[f"xe/{nr}"] = h.schur_expand(B[:nr], X2[:nr]).reshape(nr, -1)
        res[f"xs/{nr}"] = h.schur_solve(B[:nr]).reshape(nr, -1)
    return res
