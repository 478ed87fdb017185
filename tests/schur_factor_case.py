"""Cases of the dense factor of the Schur complement on the GPU, shared by test_gpu_schur_factor.py and run on
its own as a subprocess for the route switches that are read once per process (OKKT_DATAFLOW, OKKT_FLOW): prints SCHUR_FACTOR_OK when
every check held.

The accuracy rules measure against LAPACK, never against the code under test:
  reconstruction  max |P S P' - L D L'| of okkt_schur_get_factor <= 8 x the same of scipy.linalg.ldl (dsytrf) + ns 2^-52 max |S|;
  dense solve     componentwise backward error omega of x2 <= 8 x omega of scipy.linalg.solve(S, r2, assume_a="sym") + 2^-50;
  whole system    schur_case.check_solves' rule: omega <= max(100 x omega of the reference solve, 1e-13), 1e-8 relative difference in x.
The factor 8: pivot ties and the MFMA accumulation order differ from LAPACK's; both algorithms carry the same error bound."""
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import dense_ldlt_ref as ref
import schur_case as sc
from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b

MARGIN_MIN = 1e-8


def split(idx, n, m):
    return n - int((idx < n).sum()), m - int((idx >= n).sum())


def check_reconstruction(h, S):
    LD, ipiv = h.schur_get_factor()
    Lf, Df, perm = ref.unpack_lapack(LD, ipiv)
    err = ref.reconstruction_error(S, Lf, Df, perm)
    err_lapack = ref.scipy_reconstruction_error(S)
    ns = S.shape[0]
    print(f"reconstruction ns={ns} device={err:.3e} lapack={err_lapack:.3e}")
    assert err <= 8.0 * err_lapack + ns * 2.0**-52 * np.max(np.abs(S)), (ns, err, err_lapack)
    return LD, ipiv


def check_dense_solve(h, S, nrhs_list=(1, 3, 5), seed=0):
    ns = S.shape[0]
    Sf = np.tril(S) + np.tril(S, -1).T
    rng = np.random.default_rng(seed)
    for nrhs in nrhs_list:
        R2 = rng.normal(size=(nrhs, ns))
        X2 = h.schur_dense_solve(R2)
        for q in range(nrhs):
            om = ref.omega(Sf, X2[q], R2[q])
            om_lapack = ref.omega(Sf, scipy.linalg.solve(Sf, R2[q], assume_a="sym"), R2[q])
            print(f"dense solve ns={ns} nrhs={nrhs} omega={om:.3e} lapack={om_lapack:.3e}")
            assert om <= 8.0 * om_lapack + 2.0**-50, (ns, nrhs, q, om, om_lapack)
            assert np.array_equal(h.schur_dense_solve(R2[q]), X2[q])      # bitwise the same alone as in its batch
        buf = R2.copy()      # r2 may alias x2
        h._check(h._lib.okkt_schur_dense_solve(h._h, L.p_f64(buf), L.p_f64(buf), nrhs), "okkt_schur_dense_solve")
        assert np.array_equal(buf, X2)


def check_designed(h, S, zero=0):
    """a caller's S through okkt_schur_factor: ipiv against the restatement, inertia against eigvalsh, the same bits twice"""
    r = ref.bunch_kaufman(S)
    assert r["margin"] >= MARGIN_MIN, r["margin"]
    flag = h.schur_factor(S)
    LD, ipiv = check_reconstruction(h, S)
    assert np.array_equal(ipiv, r["ipiv"]), np.flatnonzero(ipiv != r["ipiv"])[:8]
    assert h.schur_inertia == r["inertia"] + (0,), (h.schur_inertia, r["inertia"])
    assert h.schur_inertia[:3] == ref.inertia_eig(S, drop=zero)
    assert flag == (1 if zero == 0 else 0)
    assert h.schur_factor(S) == flag
    LD2, ipiv2 = h.schur_get_factor()
    assert np.array_equal(LD, LD2) and np.array_equal(ipiv, ipiv2)
    if zero == 0:
        check_dense_solve(h, S, nrhs_list=(1, 3))
    return r


def check_fused(h, K, whole=None, Xref=None, nrhs_list=(1, 3, 5), seed=0):
    """schur_solve: bitwise condense -> dense solve -> expand; against the whole-matrix handle or a given dense solution"""
    dim = K.shape[0]
    rng = np.random.default_rng(seed)
    for nrhs in nrhs_list:
        B = rng.normal(size=(nrhs, dim))
        X = h.schur_solve(B)
        Xs = h.schur_expand(B, h.schur_dense_solve(h.schur_condense(B)))
        assert np.array_equal(X, Xs), nrhs
        if whole is not None:
            Xw = np.array([whole.ls_solve(b) for b in B])
            _, om = whole.residual(K, B, X)
            _, omw = whole.residual(K, B, Xw)
            print(f"fused solve nrhs={nrhs} omega={np.max(om):.3e} whole={np.max(omw):.3e}")
            assert np.all(om <= np.maximum(100.0 * omw, 1e-13)), (nrhs, om, omw)
            assert np.max(np.abs(X - Xw)) <= 1e-8 * np.max(np.abs(Xw)), nrhs
        buf = B.copy()      # rhs may alias sol
        h._check(h._lib.okkt_schur_solve(h._h, L.p_f64(buf), L.p_f64(buf), nrhs), "okkt_schur_solve")
        assert np.array_equal(buf, X)


def zeroed_diagonal(K, idx):
    """K with the set's own diagonal entries overwritten by 0.0, pattern unchanged: S becomes a general indefinite matrix"""
    K0 = K.copy()
    for c in idx:
        seg = slice(K0.indptr[c], K0.indptr[c + 1])
        hit = np.flatnonzero(K0.indices[seg] == c)
        assert hit.size == 1
        K0.data[K0.indptr[c] + hit[0]] = 0.0
    return K0


def check_needs_pivoting(K, n, m, ns, seed):
    idx = sc.mixed_set(n, m, ns, seed=seed)
    n1, m1 = split(idx, n, m)
    K0 = zeroed_diagonal(K, idx)
    h = sc.schur_handle("symmetric", K0, idx)
    assert h.ls_factor_schur(K0, n1, m1) == 1, h.inertia
    assert h.schur_factor() == 1
    A = synth.symmetrize_lower(K0).toarray()
    w = np.linalg.eigvalsh(A)
    assert h.total_inertia == (int((w > 0).sum()), int((w < 0).sum()), 0, 0), h.total_inertia
    rng = np.random.default_rng(seed)
    for nrhs in (1, 3):
        B = rng.normal(size=(nrhs, n + m))
        X = h.schur_solve(B)
        Xref = np.linalg.solve(A, B.T).T
        om = np.array([ref.omega(A, X[q], B[q]) for q in range(nrhs)])
        omr = np.array([ref.omega(A, Xref[q], B[q]) for q in range(nrhs)])
        print(f"zeroed diagonal ns={ns} nrhs={nrhs} omega={np.max(om):.3e} numpy={np.max(omr):.3e}")
        assert np.all(om <= np.maximum(100.0 * omr, 1e-13)), (ns, om, omr)
        assert np.max(np.abs(X - Xref)) <= 1e-8 * np.max(np.abs(Xref)), ns
    finalize_b(h)


def routes():
    """the fused solve and the inertia on an interior with big fronts and on one of small fronts only, whatever the interior route"""
    K, n, m = sc.kkt()
    w = sc.whole_handle(K, n, m)
    for ns in (17, 300):
        idx = sc.mixed_set(n, m, ns, seed=ns)
        n1, m1 = split(idx, n, m)
        h, S = sc.check_schur(K, idx, n1, m1)
        assert h.schur_factor() == 1
        assert h.total_inertia == w.inertia
        check_reconstruction(h, S)
        check_fused(h, K, whole=w, nrhs_list=(1, 5))
        finalize_b(h)
    finalize_b(w)
    check_needs_pivoting(K, n, m, 64, seed=64)
    prob = synth.hanging_chain(N_h=400)
    Kc = synth.augmented_matrix(prob, delta=1e-6)
    nc, mc = prob["n"], prob["m"]
    idx = sc.mixed_set(nc, mc, 12, seed=4)
    h = sc.schur_handle("symmetric", Kc, idx)
    wc = sc.whole_handle(Kc, nc, mc)
    assert h.ls_factor_schur(Kc, *split(idx, nc, mc)) in (0, 1)
    h.schur_factor()
    assert h.total_inertia == wc.inertia
    check_fused(h, Kc, whole=wc, nrhs_list=(3,))
    finalize_b(h)
    finalize_b(wc)


if __name__ == "__main__":
    routes()
    print("SCHUR_FACTOR_OK")
