"""GPU tests of GMRES-based iterative refinement (okkt_solve_gmres): the factor of a shifted matrix as the
preconditioner of A x = b, where plain refinement stalls; max_iters = 0; determinism and batches; designed fronts; full size; the
KKT layer's factor; non-finite input and the refusals.  The iteration counts are checked against the numpy restatement
(gmres_ref.py).  Measured values are printed as GMRES {json} lines."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import gmres_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EPS = 2.0 ** -52        # the default tolerance of okkt_solve_gmres
ULD = float(np.finfo(np.longdouble).eps) / 2


def record(**kw):
    print("GMRES " + json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))


def factored(A, npos, nneg, perm=None, **o):
    h = linear_solver_HIP("symmetric", **o)
    initialize_b(h)
    if perm is not None:
        h.set_perm(perm)
    h.ls_factor_b(A, npos, nneg)
    return h


def plain_solve(h, B):
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(np.ascontiguousarray(B)), L.p_f64(X), B.shape[0]), "okkt_solve")
    return X


def shifted(A, delta, count=None):
    """A (CSC) with delta added to the stored diagonal entries of its first count columns: the same pattern and entry order"""
    A = sp.csc_matrix(A, copy=True)
    count = A.shape[0] if count is None else count
    for j in range(count):
        p = A.indptr[j] + np.flatnonzero(A.indices[A.indptr[j]:A.indptr[j + 1]] == j)
        assert len(p) == 1, j
        A.data[p[0]] += delta
    return A


def longdouble_omega(M, b, x):
    """omega of x from the long-double residual of the full CSR M"""
    prod = M.data.astype(np.longdouble) * x.astype(np.longdouble)[M.indices]
    r = (b.astype(np.longdouble) - np.add.reduceat(prod, M.indptr[:-1])).astype(np.float64)
    den = np.add.reduceat(np.abs(M.data) * np.abs(x[M.indices]), M.indptr[:-1]) + np.abs(b)
    return float(np.max(np.where(np.abs(r) == 0, 0.0, np.abs(r) / np.where(den == 0, 1.0, den))))


# ---- 1. the factor of a shifted matrix ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("delta", [1e-12, 1.0, 10.0])
def test_shifted_factor(delta):
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-4)
    F = synth.augmented_matrix(prob, delta=1e-4 + delta)
    b = np.random.default_rng(4).normal(size=n + m)
    h = factored(F, n, m)
    x, info = h.ls_solve_gmres(A, b, restart=30, max_iters=200)
    _, om = h.residual(A, b, x)
    ref_x, ref = gr.gmres_ir(gr.LongResidual(ft.full_csr(sp.tril(A))), gr.dense_solver(ft.full_csr(sp.tril(F))), b)
    assert info["status"] == 0 and info["omega"] <= EPS, info
    assert om == info["omega"] and info["omega_per_rhs"][0] == om
    assert abs(info["iterations"] - ref["iterations"]) <= 2, (info, ref)
    assert info["work_bytes"] > 0
    # plain refinement given as many solves as GMRES used
    xr, rinfo = h.ls_solve_refine(A, b, max_steps=info["solves"] - 1)
    record(test="shifted", delta=delta, iterations=info["iterations"], cycles=info["cycles"], solves=info["solves"],
           omega0=info["omega0"], omega=info["omega"], ref_iterations=ref["iterations"], ref_cycles=ref["cycles"],
           ref_omegas=ref["omegas"], refine_steps=rinfo["steps"], refine_status=rinfo["status"], refine_omega=rinfo["omega"],
           work_bytes=info["work_bytes"])
    if delta == 10.0:
        assert rinfo["status"] in (1, 2) and rinfo["omega"] > 1e-10, rinfo
    finalize_b(h)


# ---- 2. max_iters = 0 ------------------------------------------------------------------------------------------------------------

def test_max_iters_zero_is_the_plain_solve():
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-4)
    h = factored(synth.augmented_matrix(prob, delta=1.0), n, m)
    B = np.random.default_rng(11).normal(size=(5, n + m))
    for nr in (1, 5):
        X, info = h.ls_solve_gmres(A, B[:nr], max_iters=0)
        assert np.array_equal(X, plain_solve(h, B[:nr]))
        _, om0 = h.residual(A, B[:nr], X)
        assert info["iterations"] == 0 and info["cycles"] == 0 and info["omega"] == info["omega0"] == np.max(om0)
        assert info["status"] == 1 and info["solves"] == (nr + 3) // 4
        assert np.array_equal(info["omega_per_rhs"], om0)
    finalize_b(h)


# ---- 3. determinism and batches ----------------------------------------------------------------------------------------------------

def test_determinism_and_batches():
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-4)
    h = factored(synth.augmented_matrix(prob, delta=1e-4 + 1.0), n, m)
    rng = np.random.default_rng(12)
    B = rng.normal(size=(5, n + m))
    B[1] = 0.0                                             # omega = 0 at the first residual: done before any cycle
    B[3] *= 1e8
    B[4] = A @ np.ones(n + m) + 1e-3 * rng.normal(size=n + m)
    X5, info5 = h.ls_solve_gmres(A, B, restart=20)
    X5b, info5b = h.ls_solve_gmres(A, B, restart=20)
    assert np.array_equal(X5, X5b) and np.array_equal(info5["omega_per_rhs"], info5b["omega_per_rhs"])
    singles = [h.ls_solve_gmres(A, B[q], restart=20) for q in range(5)]
    plain_bitwise = all(np.array_equal(plain_solve(h, B)[q], plain_solve(h, B[q:q + 1])[0]) for q in range(5))
    for q, (x1, i1) in enumerate(singles):
        assert i1["status"] == 0 and i1["omega"] <= EPS, (q, i1)
        assert np.max(np.abs(X5[q] - x1)) <= 1e-13 * max(np.max(np.abs(x1)), 1e-300), q
        if plain_bitwise:
            assert np.array_equal(X5[q], x1) and info5["omega_per_rhs"][q] == i1["omega_per_rhs"][0], q
    assert singles[1][1]["iterations"] == 0 and singles[1][1]["cycles"] == 0 and not X5[1].any()
    assert info5["iterations"] == max(i["iterations"] for _, i in singles)
    assert info5["status"] == 0 and np.all(info5["omega_per_rhs"] <= EPS)
    # one pass carries the group: fewer solve passes than the singles together
    assert info5["solves"] < sum(i["solves"] for _, i in singles)
    record(test="batch", plain_bitwise=plain_bitwise, iterations=[i["iterations"] for _, i in singles],
           solves_single=[i["solves"] for _, i in singles], solves_batch=info5["solves"])
    finalize_b(h)


# ---- 4. designed fronts -----------------------------------------------------------------------------------------------------------

REFINE_DESIGNS = ["edge-k129-c700", "edge-k2049-c129", "thin-tall-k1-2-127-128-c2100", "fan-in-8", "mixed-level"]


@pytest.mark.parametrize("name", REFINE_DESIGNS)
def test_designed_fronts_ipm(name):
    d = ft.build(ft.DESIGNS[name][0], values="ipm")
    o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
    o.ls_factor_b(d.A, d.npos, d.nneg)
    M = ft.full_csr(d.A)
    B = ft.rhs(d.n, 2)
    XT = np.array([ft.true_solution(M, o.ls_solve, b) for b in B])
    A = sp.csc_matrix(d.A)
    A.sort_indices()
    h = factored(shifted(A, 1e-2), d.npos, d.nneg, perm=d.perm, ordering=2, **ft.NO_RELAX)
    X, info = h.ls_solve_gmres(A, B)
    _, om = h.residual(A, B, X)
    fe = [ft.fwd_err(X[q], XT[q]) for q in range(2)]
    record(test="design", name=name, iterations=info["iterations"], cycles=info["cycles"], solves=info["solves"],
           omega0=info["omega0"], omega=om, fwd=fe)
    assert info["status"] == 0 and np.array_equal(om, info["omega_per_rhs"])
    for q in range(2):
        assert om[q] <= EPS and fe[q] <= 1e-13, (q, om[q], fe[q])
    finalize_b(h)


# ---- 5. full size --------------------------------------------------------------------------------------------------------------------

def test_full_size_sc3():
    prob = synth.make_config("S-C3", seed=0)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-8)
    h = factored(synth.augmented_matrix(prob, delta=1e-2), n, m)
    b = np.random.default_rng(9).normal(size=n + m)
    x, info = h.ls_solve_gmres(A, b)
    _, om = h.residual(A, b, x)
    oml = longdouble_omega(ft.full_csr(sp.tril(A)), b, x)
    record(test="full_size", name="S-C3", iterations=info["iterations"], cycles=info["cycles"], solves=info["solves"],
           omega0=info["omega0"], omega=info["omega"], omega_longdouble=oml, work_bytes=info["work_bytes"])
    assert info["status"] == 0 and info["omega"] <= EPS and om == info["omega"], info
    nnz_row = int(np.diff(ft.full_csr(sp.tril(A)).indptr).max())
    assert oml <= EPS * (1 + 4 * nnz_row * U) + 2 * (nnz_row + 1) * ULD, (oml, info["omega"])
    finalize_b(h)


# ---- 6. the KKT layer's factor -------------------------------------------------------------------------------------------------------

def test_kkt_route():
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    rng = np.random.default_rng(0)
    it = KS.Class_iterate(x=rng.normal(size=prob["n"]), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                          grad=rng.normal(size=prob["n"]), cons=prob["s"] + 0.1 * rng.normal(size=prob["m"]), a_norm_penalty_par=1e-4)
    d1, d2 = 1.0, 1e-8
    k = KS.HIP_KKT_solver("symmetric", KS.Class_parameters())
    k.initialize_b(it)
    k.form_system_b(it)
    k.factor_b(d1)
    K0 = k.matrix()                                       # values in the order of the analysed pattern
    nx = it.dim()
    ls = linear_solver_HIP.of_kkt(k)
    b = rng.normal(size=K0.shape[0])
    x0 = ls.ls_solve(b)
    # matrix() does not hold the shift: the plain solve is exact for K0 + d1 on the first n pivots, not for K0
    _, om_shift = ls.residual(shifted(K0, d1, nx).data, b, x0)
    _, om_plain = ls.residual(K0.data, b, x0)
    assert om_shift <= 1e-12 < om_plain, (om_shift, om_plain)
    A2 = shifted(K0, d2, nx)
    x, info = ls.ls_solve_gmres(A2.data, b)
    _, om = ls.residual(A2.data, b, x)
    record(test="kkt_route", iterations=info["iterations"], cycles=info["cycles"], omega0=info["omega0"], omega=info["omega"],
           omega_matrix_plus_d1=om_shift, omega_matrix=om_plain)
    assert info["status"] == 0 and info["omega"] <= EPS and om == info["omega"], info
    ls._finalize()      # a borrowed handle: the KKT solver still owns it
    k.finalize_b()


# ---- 7. non-finite input and the refusals -------------------------------------------------------------------------------------------

def test_non_finite_rhs_and_zero_pivot():
    prob = synth.make_config("S-small", seed=3, well_scaled=True)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-8)
    h = factored(synth.augmented_matrix(prob, delta=1e-2), n, m)
    B = np.random.default_rng(6).normal(size=(3, n + m))
    B[1, 7] = np.nan
    X, info = h.ls_solve_gmres(A, B)
    assert info["status"] == 3 and np.isnan(info["omega_per_rhs"][1])
    for q in (0, 2):
        x1, i1 = h.ls_solve_gmres(A, B[q])
        assert i1["status"] == 0 and np.isfinite(info["omega_per_rhs"][q]) and info["omega_per_rhs"][q] <= EPS
        assert np.max(np.abs(X[q] - x1)) <= 1e-13 * np.max(np.abs(x1))
    finalize_b(h)
    A = sp.csc_matrix(np.diag([2.0, 0.0, -3.0, 1.0]))
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    assert h.ls_factor_b(A, 3, 1) == 0
    x, info = h.ls_solve_gmres(A, np.ones(4), max_iters=5)
    assert info["status"] == 3 or np.all(np.isfinite(x))
    finalize_b(h)


def test_refusals():
    prob = synth.make_config("S-small", seed=2, convex=False, neg_shift=50.0, well_scaled=True)
    n, m = prob["n"], prob["m"]
    K0 = synth.augmented_matrix(prob, delta=0.0)
    good = synth.augmented_matrix(synth.make_config("S-small", seed=2, well_scaled=True), delta=1e-8)
    b = np.random.default_rng(1).normal(size=n + m)

    def works(h):
        x, info = h.ls_solve_gmres(good, b)
        assert info["status"] == 0, info

    # before a factorisation, then bad arguments, each followed by a call that works
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(good)
    with pytest.raises(OkktError, match="before a factorisation"):
        h.ls_solve_gmres(good, b)
    assert h.ls_factor_b(good, n, m) == 1
    works(h)
    lib, vals, x = h._lib, L.f64(sp.csc_matrix(good).data), np.zeros(n + m)
    for nrhs, restart, max_iters, what in ((-1, 30, 10, "nrhs"), (1, 30, -1, "max_iters"), (1, 65, 10, "restart")):
        assert lib.okkt_solve_gmres(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), nrhs, restart, max_iters, 0.0, None, None) == L.OKKT_ERR_INVALID
        assert what in lib.okkt_last_error(h._h).decode()
        works(h)
    assert lib.okkt_solve_gmres(h._h, None, L.p_f64(b), L.p_f64(x), 1, 30, 10, 0.0, None, None) == L.OKKT_ERR_INVALID
    works(h)
    finalize_b(h)
    # an early exit that stopped short, then a complete factorisation on the same handle
    early = linear_solver_HIP("symmetric", early_exit=1)
    initialize_b(early)
    assert early.ls_factor_b(K0, n, m) == 0 and sum(early.inertia) < n + m
    with pytest.raises(OkktError, match="before a factorisation"):
        early.ls_solve_gmres(K0, b)
    early._lib.okkt_set_early_exit(early._h, 0)
    assert early.ls_factor_b(good, n, m) == 1
    works(early)
    finalize_b(early)
    # Schur mode, then the set cleared
    s = linear_solver_HIP("symmetric")
    initialize_b(s)
    s.set_schur(np.array([0, n]))
    s.analyze(good)
    with pytest.raises(OkktError, match="Schur mode"):
        s.ls_solve_gmres(good, b)
    s.set_schur(np.array([], dtype=np.int64))
    assert s.ls_factor_b(good, n, m) == 1
    works(s)
    finalize_b(s)
    # a partitioned handle, then one part again
    p = linear_solver_HIP("symmetric")
    initialize_b(p)
    p.analyze(good)
    assert p._lib.okkt_dist_set_partition(p._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        p.ls_solve_gmres(good, b)
    assert p._lib.okkt_dist_set_partition(p._h, 1, 0) == L.OKKT_OK
    assert p.ls_factor_b(good, n, m) == 1
    works(p)
    finalize_b(p)
