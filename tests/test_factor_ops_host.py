"""Host tests of the factor-as-an-operator calls: the new entry points on a handle without a device, the
long-double reference (factor_ops_ref.py) against dense numpy on the smallest design of the GPU file, and the negative control of
okkt_factor_error confirmed with the oracle's factor before the GPU test relies on it."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import oracle
from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ops_ref as fr  # noqa: E402
import front_trees as ft  # noqa: E402

NEW = ["okkt_solve_forward", "okkt_solve_forward_dev", "okkt_solve_backward", "okkt_solve_backward_dev", "okkt_quadform",
       "okkt_quadform_dev", "okkt_factor_multiply", "okkt_factor_multiply_dev", "okkt_factor_error", "okkt_factor_error_dev"]
SMALLEST = "small-classes-f32-33-64-65-128-129"
CONTROL = fr.CONTROL
perturbed = fr.perturbed


def test_abi_symbols_and_no_device():
    """The new entry points exist with the declared signatures, refuse bad arguments with OKKT_ERR_INVALID and a host_symbolic_only
    handle with OKKT_ERR_NO_DEVICE, every one of them."""
    lib = L.load()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktFactorErrorInfo._fields_] == ["rho", "norm_abs_ldlt", "norm_f", "eta", "eta_row", "probes"]
    assert C.sizeof(L.OkktFactorErrorInfo) == 48
    assert (L.OKKT_OP_L, L.OKKT_OP_LT, L.OKKT_OP_LDLT, L.OKKT_OP_ABS_LDLT) == (1, 2, 3, 4)
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    A = sp.csc_matrix(np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0, 1.0, -2.0]]))
    h.analyze(A)
    b = np.ones(3)
    x = np.zeros(3)
    qp = np.zeros(1)
    qn = np.zeros(1)
    vals = L.f64(A.data)
    info = L.OkktFactorErrorInfo()
    dev = C.c_void_p(8)
    pb, px = L.p_f64(b), L.p_f64(x)
    calls = {
        "okkt_solve_forward": lambda hh, nrhs=1: lib.okkt_solve_forward(hh, pb, px, nrhs),
        "okkt_solve_forward_dev": lambda hh, nrhs=1: lib.okkt_solve_forward_dev(hh, dev, dev, nrhs),
        "okkt_solve_backward": lambda hh, nrhs=1: lib.okkt_solve_backward(hh, pb, px, nrhs),
        "okkt_solve_backward_dev": lambda hh, nrhs=1: lib.okkt_solve_backward_dev(hh, dev, dev, nrhs),
        "okkt_quadform": lambda hh, nrhs=1: lib.okkt_quadform(hh, pb, nrhs, L.p_f64(qp), L.p_f64(qn)),
        "okkt_quadform_dev": lambda hh, nrhs=1: lib.okkt_quadform_dev(hh, dev, nrhs, L.p_f64(qp), L.p_f64(qn)),
        "okkt_factor_multiply": lambda hh, nrhs=1: lib.okkt_factor_multiply(hh, L.OKKT_OP_LDLT, pb, px, nrhs),
        "okkt_factor_multiply_dev": lambda hh, nrhs=1: lib.okkt_factor_multiply_dev(hh, L.OKKT_OP_L, dev, dev, nrhs),
        "okkt_factor_error": lambda hh, nrhs=1: lib.okkt_factor_error(hh, L.p_f64(vals), 2, C.byref(info)),
        "okkt_factor_error_dev": lambda hh, nrhs=1: lib.okkt_factor_error_dev(hh, dev, 2, C.byref(info)),
    }
    assert sorted(calls) == sorted(NEW)
    for name, call in calls.items():
        assert call(None) == L.OKKT_ERR_INVALID, name
        assert call(h._h) == L.OKKT_ERR_NO_DEVICE, name
        assert "host_symbolic_only" in lib.okkt_last_error(h._h).decode(), name
        if "factor_error" not in name:
            assert call(h._h, -1) == L.OKKT_ERR_INVALID, name
    # NULL pointers, an unknown op, too many probes: refused before the device gate
    assert lib.okkt_solve_forward(h._h, None, px, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_solve_backward(h._h, pb, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_quadform(h._h, pb, 1, None, L.p_f64(qn)) == L.OKKT_ERR_INVALID
    assert lib.okkt_factor_multiply(h._h, L.OKKT_OP_L, None, px, 1) == L.OKKT_ERR_INVALID
    for op in (0, 5, -1):
        assert lib.okkt_factor_multiply(h._h, op, pb, px, 1) == L.OKKT_ERR_INVALID
        assert "unknown op" in lib.okkt_last_error(h._h).decode()
    assert lib.okkt_factor_error(h._h, L.p_f64(vals), 9, C.byref(info)) == L.OKKT_ERR_INVALID
    assert lib.okkt_factor_error(h._h, L.p_f64(vals), 2, None) == L.OKKT_ERR_INVALID
    # the handle still works
    assert h.stats()["n"] == 3
    finalize_b(h)


def _mix64_int(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_probe_hash_matches_plain_integers():
    for p in (0, 1, 7):
        v = fr.probe(p, 300)
        ref = [(-1.0 if _mix64_int((p << 32) ^ i) >> 63 else 1.0) for i in range(300)]
        assert v.tolist() == ref
        assert set(v.tolist()) == {-1.0, 1.0}
    assert not np.array_equal(fr.probe(0, 300), fr.probe(1, 300))


def test_reference_against_dense_numpy():
    """factor_ops_ref on the smallest design against dense float64 restatements: L v, L^T x, L D L^T x = A x up to the factorisation's
    error, the absolute variants, the counts, the quadratic form."""
    d = ft.build(ft.DESIGNS[SMALLEST][0])
    n = d.n
    Af = np.asarray(ft.full_csr(d.A).todense())
    Lm, dd = fr.dense_static_ldlt(Af, d.perm)
    F = fr.Factor(sp.csc_matrix(np.tril(Lm, -1)), dd, d.perm)
    assert np.array_equal(F.colcount, np.count_nonzero(Lm, axis=0)) and np.array_equal(F.rowcount, np.count_nonzero(Lm, axis=1))
    assert np.array_equal(F.colcount, d.colcounts())
    rng = np.random.default_rng(1)
    v = rng.normal(size=n)
    tol = 1e-13
    for got, ref in ((F.mul_L(v), Lm @ v), (F.mul_LT(v), Lm.T @ v), (F.mul_L(v, True), np.abs(Lm) @ v), (F.mul_LT(v, True), np.abs(Lm).T @ v)):
        assert np.max(np.abs(got.astype(np.float64) - ref)) <= tol * np.max(np.abs(ref))
    y = F.mul_LDLT(v).astype(np.float64)
    assert np.max(np.abs(y - Af @ v)) <= 1e-12 * np.max(np.abs(Af @ v))
    Pm = np.eye(n)[d.perm]            # (P x)_j = x[perm[j]]
    Ad = Pm.T @ (np.abs(Lm) @ np.diag(np.abs(dd)) @ np.abs(Lm).T) @ Pm
    ya = F.mul_LDLT(v, True).astype(np.float64)
    assert np.max(np.abs(ya - Ad @ np.abs(v))) <= tol * np.max(np.abs(ya))
    # with a scaling: S^-1 P^T L D L^T P S^-1 of the factor of S A S is A again
    s = 2.0 ** rng.integers(-3, 4, size=n)
    Ls, ds = fr.dense_static_ldlt(Af * np.outer(s, s), d.perm)
    Fs = fr.Factor(sp.csc_matrix(np.tril(Ls, -1)), ds, d.perm, s)
    ys = Fs.mul_LDLT(v).astype(np.float64)
    assert np.max(np.abs(ys - Af @ v)) <= 1e-12 * np.max(np.abs(Af @ v))
    assert np.array_equal(Fs.rhs_to_factor(v).astype(np.float64), (v * s)[d.perm])
    # the forward half solve of the reference's own factor, and the quadratic form from it
    z = np.linalg.solve(Lm, v[d.perm]) / dd
    qp, qn = fr.quadform_exact(dd, z)
    assert qp >= 0 >= qn
    q = float(qp + qn)
    assert abs(q - v @ np.linalg.solve(Af, v)) <= 1e-10 * abs(q)
    assert fr.quadform_exact([2.0, -3.0, 0.0], [0.5, 2.0, 7.0]) == (Fraction(1, 2), Fraction(-12))
    # the matrix products and the error of an exact-enough factor
    ref, quot, _ = fr.factor_error(F, d.A, 2)
    assert ref["norm_f"] == np.abs(Af).sum(axis=1).max()
    assert 1.0 <= ref["rho"] < 100.0
    assert ref["eta"] <= fr.eta_bound(F.cmax, F.rmax, 1 + max(nd["level"] for nd in d.nodes))


def test_negative_control_is_above_the_bound_with_the_oracles_factor():
    """The GPU file perturbs the largest diagonal entry of the control design by 1 + 2^-20 and asks eta for at least half of the
    quotient that row must produce.  With the oracle's factor of the same matrix: the clean eta is below the bound of section 8.12,
    and half of the perturbed row's quotient is above it."""
    d = ft.build(ft.DESIGNS[CONTROL][0])
    o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
    assert o.ls_factor_b(d.A, d.npos, d.nneg) == 1
    F = fr.Factor(o.L(), o.diag(), d.perm)
    h = 1 + max(nd["level"] for nd in d.nodes)
    bound = fr.eta_bound(F.cmax, F.rmax, h)
    clean, _, _ = fr.factor_error(F, d.A, 2)
    assert clean["eta"] <= bound
    Ap, row, quotient = perturbed(d.A, F)
    bad, quot, _ = fr.factor_error(F, Ap, 2)
    assert quotient / 2 > bound
    assert bad["eta"] >= quotient / 2 and quot[0][row] >= quotient / 2
