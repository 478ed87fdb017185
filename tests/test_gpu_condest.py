"""GPU tests of the condition estimate and the forward error bound (okkt_condest, okkt_forward_error, okkt_kkt_condest,
okkt_kkt_direction_error_bound): against kappa_1 from a dense inverse, against the numpy restatement of
condest_ref.py (same estimate, same unit vectors), bitwise repeatability, the bound against the error of the long-double-refined
solution, the edge cases and the refusals."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import iterate_from_record
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import condest_ref as cr  # noqa: E402
import front_trees as ft  # noqa: E402
from test_condest_host import laplacian_2d  # noqa: E402

pytestmark = pytest.mark.gpu


def record(**kw):
    print("CONDEST " + json.dumps(kw))


def factored(A, npos, nneg, perm=None, **o):
    h = linear_solver_HIP("symmetric", **o)
    initialize_b(h)
    if perm is not None:
        h.set_perm(perm)
    h.ls_factor_b(A, npos, nneg)
    return h


def inertia(F):
    w = np.linalg.eigvalsh(F)
    return int((w > 0).sum()), int((w < 0).sum())


def cases():
    """(name, lower CSC, dense F, exact): the estimate must be exact on the diagonal and the Laplacian (nonnegative inverse)."""
    out = []
    d = np.random.default_rng(1).uniform(-1, 1, size=500) * 10.0 ** np.random.default_rng(2).uniform(-6, 6, size=500)
    out.append(("diagonal", sp.csc_matrix(np.diag(d)), np.diag(d), True))
    Fl = laplacian_2d(60, 1e-3)
    out.append(("laplacian-3600", sp.csc_matrix(np.tril(Fl)), Fl, True))
    prob = synth.make_config("S-small", seed=3, well_scaled=True)
    K = sp.csc_matrix(sp.tril(synth.augmented_matrix(prob, delta=1e-8)))
    out.append(("S-small", K, cr.dense_symmetric(K), False))
    for name in ["small-classes-f32-33-64-65-128-129", "edge-k385-c1", "thin-k128-f2049", "fan-in-8", "mixed-level"]:
        for values in ("plain", "ipm"):
            b = ft.build(ft.DESIGNS[name][0], values)
            out.append((f"{name}/{values}", b.A, cr.dense_symmetric(b.A), False))
    return out


CASES = None


def _cases():
    global CASES
    if CASES is None:
        CASES = cases()
    return CASES


@pytest.mark.parametrize("t", [1, 2, 4])
def test_condest_against_dense_inverse_and_restatement(t):
    for name, A, F, exact_case in _cases():
        p, q = inertia(F)
        h = factored(A, p, q)
        info = h.condest(A, t)
        idx = h.condest_indices()
        exact = np.linalg.cond(F, 1)
        n1, est, ref = cr.condest(F, t)
        record(test="condest", name=name, t=t, n=F.shape[0], cond1=info["cond1"], exact=float(exact), iterations=info["iterations"],
               solves=info["solves"], status=info["status"])
        assert info["status"] in (0, 1), (name, info)
        assert abs(info["norm1"] - n1) <= 1e-13 * n1, (name, info["norm1"], n1)
        if exact_case:
            assert abs(info["cond1"] - exact) <= 1e-10 * exact, (name, info, exact)
        else:
            assert info["cond1"] <= exact * (1 + 1e-10), (name, info, exact)
            assert info["cond1"] >= exact / 3.0, (name, info, exact)
        assert abs(info["inv_norm1"] - est) <= 1e-8 * est, (name, info, est)
        assert list(idx) == ref["indices"], (name, list(idx), ref["indices"])
        assert info["iterations"] == ref["iterations"] and info["solves"] == ref["solves"]
        finalize_b(h)


def test_repeatable_bitwise():
    b = ft.build(ft.DESIGNS["fan-in-8"][0], "ipm")
    runs = []
    for _ in range(2):
        h = factored(b.A, b.npos, b.nneg)
        runs.append(h.condest(b.A, 2))
        runs.append(h.condest(b.A, 2))
        finalize_b(h)
    for r in runs[1:]:
        assert all(np.float64(r[k]).tobytes() == np.float64(runs[0][k]).tobytes() for k in ("norm1", "inv_norm1", "cond1")), runs
        assert (r["iterations"], r["solves"], r["status"]) == (runs[0]["iterations"], runs[0]["solves"], runs[0]["status"])


FERR_DESIGNS = ["edge-k129-c700", "edge-k385-c1", "thin-k128-f2049", "fan-in-8", "mixed-level"]


def _ferr_case(name, A, npos, nneg, M, perm=None, **o):
    h = factored(A, npos, nneg, perm=perm, **o)
    B = ft.rhs(A.shape[0], 2)
    X0 = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(B), L.p_f64(X0), 2), "okkt_solve")
    XT = np.array([ft.true_solution(M, lambda r: h.ls_solve(r), B[q]) for q in range(2)])
    X1, _ = h.ls_solve_refine(A, B, max_steps=3)
    out = []
    for X in (X0, X1):
        ferr, berr = h.forward_error(A, B, X)
        _, om = h.residual(A, B, X)
        assert np.array_equal(berr, om)
        for q in range(2):
            true = float(np.max(np.abs(X[q] - XT[q])) / np.max(np.abs(X[q])))
            assert ferr[q] >= true, (name, q, ferr[q], true)
            out.append((float(ferr[q]), true, float(berr[q])))
    info = h.condest(A, 2)
    finalize_b(h)
    return out, info


@pytest.mark.parametrize("values", ["plain", "ipm"])
@pytest.mark.parametrize("name", FERR_DESIGNS)
def test_forward_error_designs(name, values):
    d = ft.build(ft.DESIGNS[name][0], values)
    out, info = _ferr_case(name, d.A, d.npos, d.nneg, ft.full_csr(d.A), perm=d.perm, ordering=2, **ft.NO_RELAX)
    record(test="ferr", name=name, values=values, cond1=info["cond1"], ferr_plain=[o[0] for o in out[:2]], true_plain=[o[1] for o in out[:2]],
           berr_plain=[o[2] for o in out[:2]], ferr_refined=[o[0] for o in out[2:]], true_refined=[o[1] for o in out[2:]],
           berr_refined=[o[2] for o in out[2:]])
    if values == "plain":          # well conditioned: the bound is tight enough to be useful
        assert max(o[0] for o in out) <= 1e-10, out


def test_forward_error_sc3():
    prob = synth.make_config("S-C3", seed=0)
    K = synth.augmented_matrix(prob, delta=1e-8)
    out, info = _ferr_case("S-C3", K, prob["n"], prob["m"], ft.full_csr(sp.tril(K)))
    record(test="ferr", name="S-C3", cond1=info["cond1"], ferr_plain=[o[0] for o in out[:2]], true_plain=[o[1] for o in out[:2]],
           berr_plain=[o[2] for o in out[:2]], ferr_refined=[o[0] for o in out[2:]], true_refined=[o[1] for o in out[2:]],
           berr_refined=[o[2] for o in out[2:]], iterations=info["iterations"], solves=info["solves"])


def test_edge_cases():
    # n = 1
    A = sp.csc_matrix(np.array([[-4.0]]))
    h = factored(A, 0, 1)
    info = h.condest(A, 4)
    assert info["cond1"] == 1.0 and info["norm1"] == 4.0 and info["inv_norm1"] == 0.25 and info["status"] == 0
    ferr, berr = h.forward_error(A, np.array([2.0]), np.array([-0.5]))
    assert berr == 0.0 and 0.0 <= ferr <= 1e-15
    finalize_b(h)
    # t > n is clamped
    F = np.array([[2.0, 1.0, 0.0], [1.0, -3.0, 0.5], [0.0, 0.5, 1.0]])
    A = sp.csc_matrix(np.tril(F))
    h = factored(A, *inertia(F))
    info = h.condest(A, 4)
    ref = cr.condest(F, 3)[2]
    c1 = np.linalg.cond(F, 1)
    assert c1 / 3.0 <= info["cond1"] <= c1 * (1 + 1e-12) and abs(info["inv_norm1"] - ref["est"]) <= 1e-12 * ref["est"]
    assert info["solves"] == ref["solves"] and list(h.condest_indices()) == ref["indices"]
    finalize_b(h)
    # nrhs > 4 for the forward error: each right-hand side as on its own
    d = ft.build(ft.DESIGNS["mixed-level"][0], "plain")
    h = factored(d.A, d.npos, d.nneg)
    B = ft.rhs(d.n, 6)
    X = np.array([h.ls_solve(b) for b in B])
    ferr, berr = h.forward_error(d.A, B, X)
    for q in range(6):
        f1, b1 = h.forward_error(d.A, B[q], X[q])
        assert f1 == ferr[q] and b1 == berr[q]
    finalize_b(h)
    # a factorisation whose flag is 0 (wrong inertia asked for) is accepted
    h = factored(A, 3, 0)
    assert h.inertia[:2] != (3, 0)
    info = h.condest(A, 2)
    assert info["status"] in (0, 1) and c1 / 3.0 <= info["cond1"] <= c1 * (1 + 1e-12)
    finalize_b(h)
    # an exact zero pivot: status 3, cond1 = Inf, no fault
    Z = sp.csc_matrix(np.diag([1.0, 0.0, 2.0]))
    h = factored(Z, 3, 0)
    info = h.condest(Z, 2)
    assert info["status"] == 3 and info["cond1"] == np.inf and info["inv_norm1"] == np.inf and info["norm1"] == 2.0
    ferr, _ = h.forward_error(Z, np.ones(3), np.ones(3))
    assert ferr == np.inf
    finalize_b(h)


def test_refusals():
    prob = synth.make_config("S-small", seed=2, convex=False, neg_shift=50.0, well_scaled=True)
    n, m = prob["n"], prob["m"]
    K0 = synth.augmented_matrix(prob, delta=0.0)
    b = np.ones(n + m)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K0)
    with pytest.raises(OkktError, match="before a complete factorisation"):
        h.condest(K0)
    with pytest.raises(OkktError, match="before a complete factorisation"):
        h.forward_error(K0, b, b)
    finalize_b(h)
    # an early exit that stopped short
    early = linear_solver_HIP("symmetric", early_exit=1)
    initialize_b(early)
    assert early.ls_factor_b(K0, n, m) == 0 and sum(early.inertia) < n + m
    with pytest.raises(OkktError, match="early exit"):
        early.condest(K0)
    with pytest.raises(OkktError, match="early exit"):
        early.forward_error(K0, b, b)
    finalize_b(early)
    # a partitioned handle
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K0)
    assert h._lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        h.condest(K0)
    finalize_b(h)


# ---- KKT level --------------------------------------------------------------------------------------------------------------------

def _kkt_F(k, delta):
    """The dense factored matrix of a KKT handle: its assembled lower triangle plus delta on the first n pivots."""
    dim, nnz = C.c_int64(), C.c_int64()
    k._check(k._lib.okkt_kkt_get_matrix(k._k, C.byref(dim), C.byref(nnz), None, None, None), "okkt_kkt_get_matrix")
    cp = np.zeros(dim.value + 1, dtype=np.int64)
    rv = np.zeros(max(nnz.value, 1), dtype=np.int64)
    nz = np.zeros(max(nnz.value, 1))
    k._check(k._lib.okkt_kkt_get_matrix(k._k, C.byref(dim), C.byref(nnz), L.p_i64(cp), L.p_i64(rv), L.p_f64(nz)), "okkt_kkt_get_matrix")
    A = sp.csc_matrix((nz[:nnz.value], rv[:nnz.value], cp), shape=(dim.value, dim.value))
    sh = np.zeros(dim.value)
    sh[:k._n_shift] = delta
    return cr.dense_symmetric(A, sh)


def _kkt_cases(golden):
    out = [(rec["name"], iterate_from_record(rec, KS.Class_iterate)) for rec in golden["toy_lps"]]
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    rng = np.random.default_rng(0)
    out.append(("S-small", KS.Class_iterate(x=rng.normal(size=prob["n"]), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"],
                                            H=prob["H"], grad=rng.normal(size=prob["n"]), cons=prob["s"] + 0.1 * rng.normal(size=prob["m"]),
                                            a_norm_penalty_par=1e-4)))
    return out


@pytest.mark.parametrize("kind,opts", [("symmetric", {}), ("clever_symmetric", {}), ("schur", {}), ("schur_direct", {}),
                                       ("schur", {"schur_dense_rows": 1})])
def test_kkt_condest(golden, kind, opts):
    delta = 1e-8
    for name, it in _kkt_cases(golden):
        pars = KS.Class_parameters()
        k = KS.HIP_KKT_solver(kind, pars, **opts)
        k.initialize_b(it)
        k.form_system_b(it)
        k.factor_b(delta)
        k._n_shift = it.dim()
        F = _kkt_F(k, delta)
        info = k.condest(2)
        exact = np.linalg.cond(F, 1)
        record(test="kkt_condest", kind=kind, opts=opts, name=name, cond1=info["cond1"], exact=float(exact))
        assert info["status"] in (0, 1)
        # the upper side allows the factor's own solve error: a pivot of delta = 1e-8 (toy_lp0: H = 0) grows L to 1 / delta, and the
        # device estimate, formed with the factor's solves, came out 3.5e-9 above the dense kappa there (MI355X)
        assert exact / 3.0 <= info["cond1"] <= exact * (1 + 1e-6), (kind, name, info, exact)
        if kind != "symmetric":
            with pytest.raises(OkktError, match="symmetric kind only"):
                k.direction_error_bound()
        k.finalize_b()


def test_kkt_direction_bound_and_default_path_unchanged(golden):
    for name, it in _kkt_cases(golden):
        runs = []
        for with_est in (False, True):
            k = KS.HIP_KKT_solver("symmetric")
            k.initialize_b(it)
            k.form_system_b(it)
            assert k.factor_b(1e-8) == 1
            if with_est:
                k.condest(2)
            k.kkt_associate_rhs_b(it, KS.Reduct_affine())
            with pytest.raises(OkktError):
                k.direction_error_bound()
            k.compute_direction_b()
            runs.append((k.dir.x.copy(), k.dir.y.copy(), k.dir.s.copy()))
            if with_est:
                ferr = k.direction_error_bound()
                assert 0.0 <= ferr < 1e-6, (name, ferr)
                record(test="kkt_direction_ferr", name=name, ferr=ferr)
            k.finalize_b()
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b), name
