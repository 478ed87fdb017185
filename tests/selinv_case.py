"""Cases of selected inversion on the GPU, shared by test_gpu_selinv.py and run on its own as a subprocess for the
route switches that are read once per process (OKKT_DATAFLOW, OKKT_FLOW, OKKT_RELEASE_CB): prints SELINV_OK and a digest of every Z it
computed when every check held.

Z is compared with numpy.linalg.inv of the dense matrix.  Both sides are backward stable: each is the exact inverse of a matrix within
about eps * |F| of F (times a growth factor of the elimination), so their difference is about eps * cond(F) * |F^-1|.  The designed
fronts carry a diagonal of +-3 sqrt(f) and the synthetic systems are well scaled (cond(F) below 1e5 on every case here); Z_TOL = 1e-8
relative to max |F^-1| leaves two orders of magnitude above eps * cond(F) for the sums over a few thousand terms.  A nonconvex KKT
system is factored without pivoting, so the factor is backward stable only up to its growth g = max(|L| |D| |L'|) / max|F|: the
computed Z is the inverse of a matrix within eps g |F| of F.  The tolerance is then 100 eps g cond(F), the same first-order bound with the
same margin (measured: g near 1e3 on the nonconvex KKT case)."""
import hashlib
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
from onephase_jl_amd import synth  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP  # noqa: E402

Z_TOL = 1e-8


def dense(A):
    return synth.symmetrize_lower(sp.csc_matrix(A)).toarray()


def design_handle(name, **opts):
    d = ft.build(ft.DESIGNS[name][0])
    h = linear_solver_HIP("symmetric", ordering=2, **dict(ft.NO_RELAX, **opts))
    initialize_b(h)
    h.set_perm(d.perm)
    h.ls_factor_b(d.A, d.npos, d.nneg)
    return d, h


def growth(h, D):
    """max(|L| |D| |L'|) / max|F| of the handle's factor"""
    Lf = abs(h.factor_csc()) + sp.identity(D.shape[0], format="csc")
    G = Lf @ sp.diags(np.abs(h.diag())) @ Lf.T
    return max(1.0, float(abs(G).max()) / float(np.max(np.abs(D))))


def tolerance(D, h=None):
    """relative tolerance for the inverse of the dense symmetric D factored by h (see the module docstring)"""
    g = growth(h, D) if h is not None else 1.0
    return max(Z_TOL, 100.0 * np.finfo(float).eps * g * np.linalg.cond(D))


def check_against_dense(h, A, perm=None):
    """selinv on a factored handle; inverse_csc and inverse_diag against the dense inverse; returns (Zcsc, diag)"""
    info = h.selinv()
    assert info["status"] == 0 and info["nonfinite"] == 0, info
    D = dense(A)
    Ainv = np.linalg.inv(D)
    tol = tolerance(D, h)
    scale = np.max(np.abs(Ainv))
    p = h.perm() if perm is None else perm
    Z = h.inverse_csc()
    Zc = Z.tocoo()
    assert np.all(Zc.row >= Zc.col)
    ref = Ainv[p[Zc.row], p[Zc.col]]
    err = np.max(np.abs(Zc.data - ref))
    assert err <= tol * scale, (err, scale, tol)
    d = h.inverse_diag()
    assert np.max(np.abs(d - np.diag(Ainv))) <= tol * scale
    # the diagonal sits in the CSC as well, first in its column
    assert np.array_equal(Z.diagonal(), d[p])
    return Z, d


def check_on_pattern(h, A):
    """inverse_on_pattern against the dense inverse at every input entry (the analysed pattern, nzval layout)"""
    A = sp.csc_matrix(A)
    A.sort_indices()
    D = dense(A)
    Ainv = np.linalg.inv(D)
    zv = h.inverse_on_pattern()
    assert len(zv) == A.nnz
    rows = A.indices
    cols = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    ok = np.isfinite(zv)
    lower = rows >= cols
    assert ok[lower].all()
    err = np.max(np.abs(zv[ok] - Ainv[rows[ok], cols[ok]]))
    assert err <= tolerance(D, h) * np.max(np.abs(Ainv)), err
    return zv


def digest(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


ROUTE_DESIGNS = ["small-classes-f32-33-64-65-128-129", "task-chains-under-big", "mixed-level-scatter", "deep-chain-6", "forest-3-roots"]


def routes():
    out = []
    for name in ROUTE_DESIGNS:
        d, h = design_handle(name)
        Z, dg = check_against_dense(h, d.A, perm=d.perm)
        out.append(digest(Z.data, Z.indices, dg))
        finalize_b(h)
    return out


if __name__ == "__main__":
    dg = routes()
    print("SELINV_OK " + " ".join(dg))
