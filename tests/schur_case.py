"""Cases of Schur mode on the GPU, shared by test_gpu_schur_complement.py and run on its own as a subprocess
for the route switches that are read once per process (OKKT_DATAFLOW, OKKT_FLOW): prints SCHUR_OK when every check held.

S is compared with A22 - A21 A11^-1 A12 computed by NumPy from the dense A11 (LU with partial pivoting).  Both sides are backward stable,
so each is within about eps * cond(A11) * |A21| |A11^-1| |A12| of the exact S; on the well-scaled systems used here cond(A11) stays
below 1e4, and 1e-10 * max|S_ref| leaves two orders of magnitude above that for the accumulation over a few thousand terms."""
import sys

import numpy as np

sys.path.insert(0, ".")
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

S_TOL = 1e-10


def kkt(n=1500, m=1000, seed=5, delta=1e-8):
    prob = synth.make_problem(n, m, seed=seed, well_scaled=True)
    return synth.augmented_matrix(prob, delta=delta), n, m


def mixed_set(n, m, ns, seed=0):
    """ns indices, about half primal and half dual, in a shuffled order"""
    rng = np.random.default_rng(seed)
    k = ns // 2
    return np.concatenate([rng.choice(n, ns - k, replace=False), n + rng.choice(m, k, replace=False)])[rng.permutation(ns)]


def dense_parts(K, idx):
    A = synth.symmetrize_lower(K).toarray()
    inner = np.setdiff1d(np.arange(A.shape[0]), idx)
    return A[np.ix_(inner, inner)], A[np.ix_(idx, inner)], A[np.ix_(idx, idx)], inner


def schur_ref(K, idx):
    A11, A21, A22, _ = dense_parts(K, idx)
    return A22 - A21 @ np.linalg.solve(A11, A21.T)


def inertia_of(w):
    return int((w > 0).sum()), int((w < 0).sum())


def schur_handle(sym, K, idx, **opts):
    h = linear_solver_HIP(sym, **opts)
    initialize_b(h)
    h.set_schur(idx)
    h.analyze(K)
    return h


def check_schur(K, idx, n1, m1, sym="symmetric", Sref=None, **opts):
    """factor A11 + assemble S; S against the dense reference; returns (handle, S)"""
    h = schur_handle(sym, K, idx, **opts)
    assert h.ls_factor_schur(K, n1, m1) == 1, h.inertia
    S = h.schur()
    if Sref is None:
        Sref = schur_ref(K, idx)
    err = np.max(np.abs(S - Sref))
    assert err <= S_TOL * np.max(np.abs(Sref)), (len(idx), err, np.max(np.abs(Sref)))
    assert np.array_equal(S, S.T)
    return h, S


def whole_handle(K, n, m, sym="symmetric"):
    w = linear_solver_HIP(sym)
    initialize_b(w)
    assert w.ls_factor_b(K, n, m) in (0, 1)
    return w


def check_solves(h, S, K, whole, nrhs_list=(1, 3, 5), seed=0):
    """condense -> numpy.linalg.solve(S, r2) -> expand reproduces the whole-matrix solve; omega at the whole solve's level"""
    dim = K.shape[0]
    rng = np.random.default_rng(seed)
    for nrhs in nrhs_list:
        B = rng.normal(size=(nrhs, dim))
        R2 = h.schur_condense(B)
        X2 = np.linalg.solve(S, R2.T).T
        X = h.schur_expand(B, X2)
        Xw = np.array([whole.ls_solve(b) for b in B])
        _, om = whole.residual(K, B, X)
        _, omw = whole.residual(K, B, Xw)
        assert np.all(om <= np.maximum(100.0 * omw, 1e-13)), (nrhs, om, omw)
        assert np.max(np.abs(X - Xw)) <= 1e-8 * np.max(np.abs(Xw)), nrhs
        Xs = h.schur_expand(B, X2)
        assert np.array_equal(X, Xs)


def routes():
    """the route cases: an interior with big fronts through the dataflow launch (Schur front above and below small_front_max)
    and an interior of small fronts only (the banded hanging chain)"""
    K, n, m = kkt()
    for ns in (17, 300):
        idx = mixed_set(n, m, ns, seed=ns)
        h, S = check_schur(K, idx, n - (idx < n).sum(), m - (idx >= n).sum())
        w = whole_handle(K, n, m)
        check_solves(h, S, K, w, nrhs_list=(1, 5))
        finalize_b(h)
        finalize_b(w)
    prob = synth.hanging_chain(N_h=400)
    Kc = synth.augmented_matrix(prob, delta=1e-6)
    nc, mc = prob["n"], prob["m"]
    idx = mixed_set(nc, mc, 12, seed=4)
    h = schur_handle("symmetric", Kc, idx)
    st = h.stats()
    assert st["n_big_fronts"] == 0, st
    w = whole_handle(Kc, nc, mc)
    A11 = dense_parts(Kc, idx)[0]
    p1, n1 = inertia_of(np.linalg.eigvalsh(A11))
    assert h.ls_factor_schur(Kc, p1, n1) in (0, 1)
    assert h.inertia[:2] == (p1, n1)
    S = h.schur()
    Sref = schur_ref(Kc, idx)
    assert np.max(np.abs(S - Sref)) <= S_TOL * np.max(np.abs(Sref))
    check_solves(h, S, Kc, w, nrhs_list=(3,))
    finalize_b(h)
    finalize_b(w)


if __name__ == "__main__":
    routes()
    print("SCHUR_OK")
