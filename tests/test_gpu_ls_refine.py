"""GPU tests of refinement with extra-precise residuals (okkt_residual, okkt_solve_refine, okkt_kkt_set_ls_refine).

The residual r = b - A x is checked against the exact residual (fractions.Fraction) on small matrices and against the long-double
residual at S-C3 / S-metric size; the refinement against the designed fronts of front_trees.py ("ipm" values), full-size systems,
a factor of a nearby matrix, non-finite input and the symmetric KKT kind.  Measured values are printed as REFINE {json} lines."""
import ctypes as C
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP
from oracle import kkt_oracle as KO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53          # unit roundoff of double
EPS = 2.0 ** -52        # the default tolerance of okkt_solve_refine
ULD = float(np.finfo(np.longdouble).eps) / 2


def record(**kw):
    print("REFINE " + json.dumps(kw))


def raw_csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return (A.shape[0], L.i64(A.indptr), L.i64(A.indices), L.f64(A.data), 0)


def factored(A, npos, nneg, perm=None, **o):
    h = linear_solver_HIP("symmetric", **o)
    initialize_b(h)
    if perm is not None:
        h.set_perm(perm)
    h.ls_factor_b(A, npos, nneg)
    return h


def entries(raw):
    """(i, j, value) of the symmetric matrix the factor sees: the lower triangle, duplicates summed in input order from 0."""
    dim, cp, rv, nz, base = raw
    acc = {}
    for j in range(dim):
        for p in range(cp[j] - base, cp[j + 1] - base):
            i = int(rv[p]) - base
            if i < j:
                continue
            acc[(i, j)] = acc.get((i, j), 0.0) + float(nz[p])
    rows = [[] for _ in range(dim)]
    for (i, j), v in acc.items():
        rows[i].append((j, v))
        if i != j:
            rows[j].append((i, v))
    return rows


def exact_check(rows, b, x, r, om):
    """|r - r_exact| <= u |r_exact| + 4 nnz_i u^2 (|A||x|)_i against Fraction arithmetic; omega against a host omega"""
    worst = 0.0
    den = np.zeros(len(b))
    for i, row in enumerate(rows):
        ex = Fraction(float(b[i]))
        ax = 0.0
        for j, v in row:
            ex -= Fraction(v) * Fraction(float(x[j]))
            ax += abs(v) * abs(float(x[j]))
        den[i] = ax + abs(float(b[i]))
        err = abs(Fraction(float(r[i])) - ex)
        bound = U * abs(ex) + 4 * max(len(row), 1) * U * U * Fraction(ax)
        assert err <= bound, (i, float(err), float(bound))
        worst = max(worst, float(err / bound) if bound else 0.0)
    host = np.max(np.where(np.abs(r) == 0, 0.0, np.abs(r) / np.where(den == 0, 1.0, den)))
    assert abs(om - host) <= 8 * U * host, (om, host)
    return worst


def longdouble_check(M, b, x, r):
    """against the long-double residual of the full CSR M: the double-double bound widened by long double's own error"""
    prod = M.data.astype(np.longdouble) * x.astype(np.longdouble)[M.indices]
    rl = b.astype(np.longdouble) - np.add.reduceat(prod, M.indptr[:-1])
    ax = np.add.reduceat(np.abs(M.data) * np.abs(x[M.indices]), M.indptr[:-1])
    nnz = np.diff(M.indptr)
    bound = U * np.abs(rl.astype(np.float64)) + (4 * nnz * U * U + 2 * (nnz + 1) * ULD) * ax * 1.01
    err = np.abs(r.astype(np.longdouble) - rl).astype(np.float64)
    assert np.all(err <= bound), float(np.max(err / np.where(bound == 0, 1, bound)))
    return float(np.max(err / np.where(bound == 0, 1, bound)))


def host_omega(M, b, x, r):
    den = np.add.reduceat(np.abs(M.data) * np.abs(x[M.indices]), M.indptr[:-1]) + np.abs(b)
    return float(np.max(np.where(np.abs(r) == 0, 0.0, np.abs(r) / np.where(den == 0, 1.0, den))))


def plain_solve(h, B):
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(np.ascontiguousarray(B)), L.p_f64(X), B.shape[0]), "okkt_solve")
    return X


# ---- 1. residual exactness ----------------------------------------------------------------------------------------------------

def _check_residual_small(raw, npos, nneg, perm=None, seed=0, **o):
    dim = raw[0]
    h = factored(raw, npos, nneg, perm=perm, **o)
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(5, dim))
    X = plain_solve(h, B) + 1e-3 * rng.normal(size=(5, dim))     # not the solution: a residual of size
    R5, om5 = h.residual(raw[3], B, X)
    rows = entries(raw)
    worst = max(exact_check(rows, B[q], X[q], R5[q], om5[q]) for q in range(2))
    for nr in (1, 4):
        Rq, omq = h.residual(raw[3], B[:nr], X[:nr])
        assert np.array_equal(Rq, R5[:nr]) and np.array_equal(omq, om5[:nr])
    for q in range(5):
        r1, o1 = h.residual(raw[3], B[q], X[q])
        assert np.array_equal(r1, R5[q]) and o1 == om5[q]
    R5b, om5b = h.residual(raw[3], B, X)
    assert np.array_equal(R5b, R5) and np.array_equal(om5b, om5)
    finalize_b(h)
    return worst


@pytest.mark.parametrize("name,values", [("small-classes-f32-33-64-65-128-129", "plain"), ("small-classes-f32-33-64-65-128-129", "ipm"),
                                         ("edge-k385-c1", "ipm")])
def test_residual_exact_on_designs(name, values):
    d = ft.build(ft.DESIGNS[name][0], values=values)
    worst = _check_residual_small(raw_csc(d.A), d.npos, d.nneg, perm=d.perm, ordering=2, **ft.NO_RELAX)
    record(test="residual_exact", name=name, values=values, worst_over_bound=worst)


def test_residual_exact_on_reference_matrices(golden):
    for rec in golden["linear_solvers"]:
        A = sp.csc_matrix(np.array(rec["A_lower"]))
        _check_residual_small(raw_csc(A), rec["n"], rec["m"])


def test_residual_exact_with_upper_and_duplicate_entries():
    rng = np.random.default_rng(5)
    n = 60
    S = sp.random(n, n, density=0.15, random_state=5)
    M = sp.tril(S + S.T, -1) + sp.diags(rng.choice([-1.0, 1.0], n) * 4.0)
    T = sp.coo_matrix(M)
    cols, rows, vals = [], [], []
    for i, j, v in zip(T.row, T.col, T.data):
        if rng.random() < 0.3:                              # a duplicate pair summing to roughly v
            a = v * rng.uniform(0.2, 0.8)
            cols += [j, j]; rows += [i, i]; vals += [a, v - a]
        else:
            cols.append(j); rows.append(i); vals.append(v)
        if i != j and rng.random() < 0.3:                   # an upper entry with a value nobody may read
            cols.append(i); rows.append(j); vals.append(1e3 * rng.normal())
    order = rng.permutation(len(cols))                      # rows in no order inside a column
    cols, rows, vals = np.array(cols)[order], np.array(rows)[order], np.array(vals)[order]
    srt = np.argsort(cols, kind="stable")
    cols, rows, vals = cols[srt], rows[srt], vals[srt]
    colptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(colptr, cols + 1, 1)
    colptr = np.cumsum(colptr)
    Md = sp.csc_matrix(M).toarray()
    Md = np.tril(Md) + np.tril(Md, -1).T
    w = np.linalg.eigvalsh(Md)
    for base in (0, 1):
        raw = (n, L.i64(colptr + base), L.i64(rows + base), L.f64(vals), base)
        _check_residual_small(raw, int((w > 0).sum()), int((w < 0).sum()))


def test_residual_sc3_against_long_double():
    prob = synth.make_config("S-C3", seed=0)
    K = synth.augmented_matrix(prob, delta=1e-8)          # upper J' block present: ignored as by the factorisation
    h = factored(K, prob["n"], prob["m"])
    M = ft.full_csr(sp.tril(K))
    rng = np.random.default_rng(3)
    B = rng.normal(size=(5, K.shape[0]))
    X = plain_solve(h, B)
    R, om = h.residual(K, B, X)
    worst = max(longdouble_check(M, B[q], X[q], R[q]) for q in range(5))
    for q in range(5):
        assert abs(om[q] - host_omega(M, B[q], X[q], R[q])) <= 8 * U * om[q]
        r1, o1 = h.residual(K, B[q], X[q])
        assert np.array_equal(r1, R[q]) and o1 == om[q]
    record(test="residual_sc3", worst_over_bound=worst, omega0=[float(v) for v in om])
    finalize_b(h)


# ---- 2. refinement on designed fronts ------------------------------------------------------------------------------------------

REFINE_DESIGNS = ["edge-k129-c700", "edge-k2049-c129", "thin-tall-k1-2-127-128-c2100", "fan-in-8", "mixed-level"]


@pytest.mark.parametrize("name", REFINE_DESIGNS)
def test_refine_designed_fronts_ipm(name):
    """Measured on MI355X (two right-hand sides each): omega0 5.9e-15 .. 1.4e-12, one correction, omega <= 5.3e-17; forward error
    against the long-double-refined solution from 5.9e-14 .. 8.9e-12 down to 1.9e-18 .. 5.1e-17 (ratios refined / plain 1e-6 .. 1e-4)."""
    d = ft.build(ft.DESIGNS[name][0], values="ipm")
    o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
    o.ls_factor_b(d.A, d.npos, d.nneg)
    M = ft.full_csr(d.A)
    B = ft.rhs(d.n, 2)
    XT = np.array([ft.true_solution(M, o.ls_solve, b) for b in B])
    h = factored(d.A, d.npos, d.nneg, perm=d.perm, ordering=2, **ft.NO_RELAX)
    X0 = plain_solve(h, B)
    X, info = h.ls_solve_refine(d.A, B, max_steps=5)
    om = info["omega_per_rhs"]
    assert info["steps"] <= 5
    fe0 = [ft.fwd_err(X0[q], XT[q]) for q in range(2)]
    fe = [ft.fwd_err(X[q], XT[q]) for q in range(2)]
    _, om0 = h.residual(d.A, B, X0)
    _, omr = h.residual(d.A, B, X)
    assert np.array_equal(omr, om)                         # the omega reported is the omega of the returned x
    record(test="refine_design", name=name, steps=info["steps"], status=info["status"], omega0=[float(v) for v in om0],
           omega=[float(v) for v in om], fwd0=fe0, fwd=fe)
    for q in range(2):
        assert om[q] <= EPS or (info["status"] == 2 and om[q] <= 8 * EPS), (q, om[q], info)
        if om0[q] > 1e3 * U:
            assert om[q] <= EPS or om[q] <= om0[q] / 100
        assert fe[q] <= max(fe0[q], 8 * U), (fe[q], fe0[q])
    finalize_b(h)


# ---- 3, 4. max_steps = 0 and batch invariance -------------------------------------------------------------------------------------

def test_max_steps_zero_is_the_plain_solve_and_batches():
    prob = synth.make_config("S-small", seed=2, well_scaled=True)
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = factored(K, prob["n"], prob["m"])
    dim = K.shape[0]
    rng = np.random.default_rng(11)
    B = rng.normal(size=(5, dim))
    B[1] = 0.0                                             # converges at step 0 (omega = 0)
    B[3] *= 1e8
    for nr in (1, 5):
        X, info = h.ls_solve_refine(K, B[:nr], max_steps=0)
        assert np.array_equal(X, plain_solve(h, B[:nr]))
        assert info["steps"] == 0 and info["omega"] == info["omega0"]
        assert info["status"] == (0 if info["omega0"] <= EPS else 1)
    # five at once against one by one: the same decisions; the same bits whenever the plain solve's batches are bitwise the singles
    X5, info5 = h.ls_solve_refine(K, B, max_steps=4)
    singles = [h.ls_solve_refine(K, B[q], max_steps=4) for q in range(5)]
    plain_bitwise = all(np.array_equal(plain_solve(h, B)[q], plain_solve(h, B[q:q + 1])[0]) for q in range(5))
    for q, (x1, i1) in enumerate(singles):
        assert np.max(np.abs(X5[q] - x1)) <= 1e-13 * max(np.max(np.abs(x1)), 1e-300), q
        if plain_bitwise:
            assert np.array_equal(X5[q], x1) and info5["omega_per_rhs"][q] == i1["omega_per_rhs"][0], q
    assert singles[1][1]["steps"] == 0 and singles[1][1]["status"] == 0 and not X5[1].any()
    assert info5["steps"] == max(i["steps"] for _, i in singles)
    assert info5["status"] == max(i["status"] for _, i in singles)
    record(test="batch", plain_bitwise=plain_bitwise, steps=[i["steps"] for _, i in singles],
           omega=[float(i["omega"]) for _, i in singles])
    finalize_b(h)


# ---- 5. a factor of a nearby matrix ---------------------------------------------------------------------------------------------

def test_refine_with_the_factor_of_a_shifted_matrix():
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-4)
    b = np.random.default_rng(4).normal(size=n + m)
    for delta, ok in ((1e-12, True), (1.0, False)):
        As = synth.augmented_matrix(prob, delta=1e-4 + delta)
        h = factored(As, n, m)
        x, info = h.ls_solve_refine(A, b, max_steps=6)
        _, om = h.residual(A, b, x)
        assert om == info["omega"] and info["steps"] <= 6
        record(test="nearby", delta=delta, **{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in info.items()})
        if ok:
            assert info["status"] == 0 and info["omega"] <= EPS
        else:
            assert info["status"] in (1, 2) and info["omega"] <= info["omega0"] and np.all(np.isfinite(x))
        finalize_b(h)


# ---- 6. non-finite input ----------------------------------------------------------------------------------------------------------

def test_non_finite_rhs_and_zero_pivot():
    prob = synth.make_config("S-small", seed=3, well_scaled=True)
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = factored(K, prob["n"], prob["m"])
    B = np.random.default_rng(6).normal(size=(3, K.shape[0]))
    B[1, 7] = np.nan
    X, info = h.ls_solve_refine(K, B, max_steps=3)
    assert info["status"] == 3 and np.isnan(info["omega_per_rhs"][1])
    for q in (0, 2):
        x1, i1 = h.ls_solve_refine(K, B[q], max_steps=3)
        assert np.max(np.abs(X[q] - x1)) <= 1e-13 * np.max(np.abs(x1)) and i1["status"] != 3
        assert np.isfinite(info["omega_per_rhs"][q])
    finalize_b(h)
    # a zero pivot: flag 0, the factor exists; the refinement ends with status 3 or a finite result
    A = sp.csc_matrix(np.diag([2.0, 0.0, -3.0, 1.0]))
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    assert h.ls_factor_b(A, 3, 1) == 0
    x, info = h.ls_solve_refine(A, np.ones(4), max_steps=3)
    assert info["status"] == 3 or np.all(np.isfinite(x))
    finalize_b(h)


# ---- 7. long rows -------------------------------------------------------------------------------------------------------------------

def test_long_rows_border_and_40000_entry_row():
    rng = np.random.default_rng(8)
    n = 3000
    S = sp.random(n, n, density=0.002, random_state=8)
    M = sp.tril(S + S.T, -1).tolil()
    M[n - 1, : n - 1] = rng.normal(size=(1, n - 1))           # a border row over all n columns
    M = sp.csc_matrix(M) + sp.diags(np.full(n, 50.0))
    h = factored(M, n, 0)
    b = rng.normal(size=n)
    x = h.ls_solve(b) + 1e-6 * rng.normal(size=n)
    r, om = h.residual(M, b, x)
    w1 = longdouble_check(ft.full_csr(M), b, x, r)
    finalize_b(h)
    # S-metric with one row of J over all 40 000 columns: K's row has 40 001 entries (analysis only: the residual needs no factor)
    prob = synth.make_config("S-metric", seed=0)
    J = prob["J"].tolil()
    J[0, :] = rng.normal(size=(1, prob["n"]))
    prob["J"] = sp.csc_matrix(J)
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    Mf = ft.full_csr(sp.tril(K))
    assert np.diff(Mf.indptr).max() >= 40_000
    B = rng.normal(size=(2, K.shape[0]))
    X = rng.normal(size=(2, K.shape[0]))
    R, om2 = h.residual(K, B, X)
    w2 = max(longdouble_check(Mf, B[q], X[q], R[q]) for q in range(2))
    record(test="long_rows", worst_border=w1, worst_smetric_row=w2)
    finalize_b(h)


# ---- 8. full size -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S-C3", "S-metric"])
def test_full_size_refinement(name):
    prob = synth.make_config(name, seed=0)
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = factored(K, prob["n"], prob["m"])
    assert h.inertia[:3] == (prob["n"], prob["m"], 0)
    b = np.random.default_rng(9).normal(size=K.shape[0])
    for _ in range(2):
        h.ls_solve(b)                                         # warm: the super-block inverses
    t0 = time.perf_counter()
    for _ in range(3):
        h.ls_solve(b)
    t_solve = (time.perf_counter() - t0) / 3
    h.ls_solve_refine(K, b, max_steps=3)                      # builds the row map
    t0 = time.perf_counter()
    x, info = h.ls_solve_refine(K, b, max_steps=3)
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, om = h.residual(K, b, x)
    t_res = time.perf_counter() - t0
    record(test="full_size", name=name, steps=info["steps"], status=info["status"], omega0=info["omega0"], omega=info["omega"],
           resid_inf=info["resid_inf"], host_solve_s=t_solve, host_refine_s=t_ref, host_residual_s=t_res,
           solve_ms=h.stats()["last_solve_ms"])
    assert info["status"] == 0 and info["omega"] <= 4 * U, info
    assert om == info["omega"]
    finalize_b(h)


# ---- 9. the symmetric KKT kind -------------------------------------------------------------------------------------------------------

def _synth_iterate(prob, Iterate, seed=0):
    rng = np.random.default_rng(seed)
    n, m = prob["n"], prob["m"]
    return Iterate(x=rng.normal(size=n), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                   grad=rng.normal(size=n), cons=prob["s"] + 0.1 * rng.normal(size=m), a_norm_penalty_par=1e-4)


def _direction(kind, it, delta, **kw):
    k = KS.HIP_KKT_solver(kind, **kw)
    k.initialize_b(it); k.form_system_b(it)
    assert k.factor_b(delta) == 1
    k.kkt_associate_rhs_b(it, KS.Reduct_affine())
    k.compute_direction_b()
    return k


@pytest.mark.parametrize("name,seed,well", [("S-small", 0, True), ("S-small", 3, False), ("S-C3", 0, False)])
def test_kkt_symmetric_refined_direction(name, seed, well):
    prob = synth.make_config(name, seed=seed, **({"well_scaled": True} if well else {}))
    it = _synth_iterate(prob, KS.Class_iterate, seed)
    delta = 1e-6
    plain = _direction("symmetric", it, delta)
    zero = KS.HIP_KKT_solver("symmetric", hip_ls_refine_steps=0, hip_ls_refine_tol=1e-12)   # the setter called with 0 steps
    zero.initialize_b(it); zero.form_system_b(it)
    assert zero.factor_b(delta) == 1
    zero.kkt_associate_rhs_b(it, KS.Reduct_affine()); zero.compute_direction_b()
    for a in ("x", "y", "s"):
        assert np.array_equal(getattr(zero.dir, a), getattr(plain.dir, a))
    assert zero.kkt_err_norm.overall == plain.kkt_err_norm.overall
    ref = _direction("symmetric", it, delta, hip_ls_refine_steps=4)
    e0, e1 = plain.kkt_err_norm.overall, ref.kkt_err_norm.overall
    t0, t1 = plain.timers(), ref.timers()
    record(test="kkt_symmetric", name=name, seed=seed, nerr_plain=e0, nerr_refined=e1, ratio_plain=plain.kkt_err_norm.ratio,
           ratio_refined=ref.kkt_err_norm.ratio, direction_ms_plain=t0["direction_ms"], direction_ms_refined=t1["direction_ms"],
           n_solves=t1["n_solves"], solve_ms=t1["solve_ms"], refine_ms=t1["refine_ms"])
    assert e1 <= 2.0 * e0, (e0, e1)
    assert t1["n_solves"] >= 1 and t1["solve_ms"] > 0 and t1["refine_ms"] > 0
    if well:
        io = KO.pick_KKT_solver("symmetric", perm=plain.linear_solver_perm())
        oit = _synth_iterate(prob, KO.Iterate, seed)
        io.initialize_b(oit); io.form_system_b(oit)
        assert io.factor_b(delta) == 1
        io.kkt_associate_rhs_b(oit, KO.Reduct_affine()); io.compute_direction_b()
        for a in ("x", "y", "s"):
            da, db = getattr(ref.dir, a), getattr(io.dir, a)
            assert np.max(np.abs(da - db)) <= 1e-9 * max(1.0, np.max(np.abs(db))), a
    # batched directions with refinement against the one-by-one ones
    etas = [KS.Reduct_affine(), KS.Class_reduction_factors(0.3, 0.3, 0.3), KS.Reduct_stable(), KS.Class_reduction_factors(0.2, 0.0, 0.2),
            KS.Class_reduction_factors(0.05, 0.0, 0.05)]
    ref.kkt_associate_rhs_b(it, etas[0])
    batch = ref.compute_directions_b(etas)
    for eta, (d, kerr) in zip(etas, batch):
        ref.kkt_associate_rhs_b(it, eta); ref.compute_direction_b()
        for a in ("x", "y", "s"):
            one, got = getattr(ref.dir, a), getattr(d, a)
            assert np.max(np.abs(got - one)) <= 1e-9 * max(1.0, np.max(np.abs(one))), a
    for k in (plain, zero, ref):
        k.finalize_b()


def test_kkt_setter_refusals_and_option_strings():
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    it = _synth_iterate(prob, KS.Class_iterate, 0)
    for kind in ("schur", "schur_direct", "clever_symmetric"):
        k = KS.HIP_KKT_solver(kind)
        k.initialize_b(it)
        assert k._lib.okkt_kkt_set_ls_refine(k._k, 2, 0.0) == L.OKKT_ERR_INVALID
        assert "symmetric kind only" in k._lib.okkt_kkt_last_error(k._k).decode()
        k.finalize_b()
    k = KS.HIP_KKT_solver("symmetric")
    k.initialize_b(it)
    assert k._lib.okkt_kkt_set_ls_refine(k._k, -1, 0.0) == L.OKKT_ERR_INVALID
    k.finalize_b()
    # kkt!hip_ls_refine_steps / _tol through pick_KKT_solver: a tolerance nobody meets forces corrections
    pars = KS.Class_parameters()
    pars.kkt.kkt_solver_type = "symmetric"
    pars.kkt.hip_ls_refine_steps = 3
    pars.kkt.hip_ls_refine_tol = 1e-300
    k = KS.pick_KKT_solver(pars)
    k.initialize_b(it); k.form_system_b(it)
    assert k.factor_b(1e-6) == 1
    k.kkt_associate_rhs_b(it, KS.Reduct_affine()); k.compute_direction_b()
    assert k.timers()["n_solves"] >= 2
    k.finalize_b()
    pars.kkt.kkt_solver_type = "schur"
    k = KS.pick_KKT_solver(pars)
    with pytest.raises(OkktError):
        k.initialize_b(it)
    k.finalize_b()


# ---- 10. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors():
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    K = synth.augmented_matrix(prob, delta=1e-8)
    lib = L.load()
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    b = np.ones(K.shape[0])
    with pytest.raises(OkktError, match="before a factorisation"):
        h.ls_solve_refine(K, b)
    r, om = h.residual(K, b, np.zeros_like(b))           # the residual needs no factor
    assert np.array_equal(r, b) and om == 1.0
    assert h.ls_factor_b(K, prob["n"], prob["m"]) == 1
    vals = L.f64(sp.csc_matrix(K).data)
    x = np.zeros_like(b)
    assert lib.okkt_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, -2, 0.0, None, None) == L.OKKT_ERR_INVALID
    assert "max_steps" in lib.okkt_last_error(h._h).decode()
    finalize_b(h)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    assert lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        h.residual(K, b, x)
    finalize_b(h)
