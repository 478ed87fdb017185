"""Host tests of the threshold pivot report: the NumPy restatement (pivots_ref.py) on hand-worked cases whose
multipliers are powers of two, the designed KKT system of the robust route against the four conditions its GPU test relies on, and the
new entry points of the ABI on a handle without a device."""
import ctypes as C
import os
import sys

import numpy as np
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pivots_ref as pr  # noqa: E402

NEW = ["okkt_pivot_report", "okkt_get_multipliers", "okkt_get_multipliers_dev", "okkt_get_rejected_pivots", "okkt_schur_solve_refine",
       "okkt_schur_solve_refine_dev"]


def multipliers_of(A, order=None):
    Lm, d, _ = pr.static_ldlt(A, order)
    n = Lm.shape[0]
    g, p = pr.column_maxima(pr.dense_strict_lower_csc(Lm), np.arange(n) if order is None else order)
    return Lm, d, g, p


def test_hand_worked_3x3():
    # col 0: l = (2, 4); the reduced matrix is [[-7, -14], [-14, -28]]; col 1: l = 2, and the last pivot is exactly 0
    A = np.array([[2.0, 0, 0], [4, 1, 0], [8, 2, 4]])
    Lm, d, g, p = multipliers_of(A)
    assert np.array_equal(Lm, [[1, 0, 0], [2, 1, 0], [4, 2, 1]])
    assert np.array_equal(d, [2.0, -7.0, 0.0])
    assert np.array_equal(g, [4.0, 2.0, 0.0]) and np.array_equal(p, [2, 2, -1])


def test_hand_worked_4x4():
    # col 0: l = (2, 0, 4) leaves [[4, 4, -8], [4, 2, 8], [-8, 8, -15]]; col 1: l = (1, -2) leaves [[-2, 16], [16, -31]]; col 2: l = -8
    A = np.array([[1.0, 0, 0, 0], [2, 8, 0, 0], [0, 4, 2, 0], [4, 0, 8, 1]])
    Lm, d, g, p = multipliers_of(A)
    assert np.array_equal(Lm, [[1, 0, 0, 0], [2, 1, 0, 0], [0, 1, 1, 0], [4, -2, -8, 1]])
    assert np.array_equal(d, [1.0, 4.0, -2.0, 97.0])
    assert np.array_equal(g, [4.0, 2.0, 8.0, 0.0]) and np.array_equal(p, [3, 3, 3, -1])
    rep, rej = pr.report(g, 0.25)          # 1 / u = 4: only g > 4 is rejected
    assert rep["rejected"] == 1 and list(rej) == [2] and rep["max_multiplier"] == 8.0 and rep["max_col"] == 2
    rep, rej = pr.report(g, 1.0)
    assert list(rej) == [2, 0, 1]           # descending g, ties by ascending index
    # under another order the columns move with their variables: eliminate 3 first, then 0, 1, 2
    order = np.array([3, 0, 1, 2])
    _, _, g2, p2 = multipliers_of(A, order)
    assert g2[3] == 8.0 and p2[3] == 2      # column of variable 3: l = (4, 0, 8) / 1


def test_tie_takes_the_lowest_row():
    A = np.array([[1.0, 0, 0, 0], [-2, 8, 0, 0], [2, 0, 8, 0], [1, 0, 0, 8]])
    _, _, g, p = multipliers_of(A)
    assert g[0] == 2.0 and p[0] == 1
    assert pr.column_max([1.0, -4.0, 4.0], [5, 7, 9]) == (4.0, 7)
    rep, _ = pr.report(np.array([3.0, 5.0, 5.0, 1.0]), 1.0)
    assert rep["max_col"] == 1


def test_empty_last_column_and_zero_column():
    assert pr.column_max([], []) == (0.0, -1)
    assert pr.column_max([0.0, 0.0], [4, 6]) == (0.0, 4)      # stored zeros: a row below the diagonal exists
    A = np.diag([1.0, 2.0])
    _, _, g, p = multipliers_of(A)
    assert g[1] == 0.0 and p[1] == -1


def test_non_finite_entries():
    assert pr.column_max([1.0, np.nan, np.inf], [3, 4, 5]) == (np.inf, 4)
    assert pr.column_max([1e300, -np.inf, np.nan], [3, 4, 5]) == (np.inf, 4)
    A = np.array([[1.0, 0, 0], [2, 4, 0], [np.nan, 0, 1]])
    _, _, g, p = multipliers_of(A)
    assert g[0] == np.inf and p[0] == 2
    rep, rej = pr.report(g, 1.0)
    assert rep["nonfinite_cols"] >= 1 and rep["max_multiplier"] == np.inf and rej[0] == 0 and rep["max_col"] == 0


def test_schur_set_columns_report_nothing():
    A = np.array([[1.0, 0, 0, 0], [2, 8, 0, 0], [0, 4, 2, 0], [4, 0, 8, 1]])
    F = pr.Factor(A, [1])                 # order 0, 2, 3, then the set {1}
    g, p = F.multipliers()
    assert g[1] == 0.0 and p[1] == -1
    assert g[0] == 4.0 and p[0] == 3      # the interior column keeps its row towards the set among its rows: l = (0, 4, 2)


def test_designed_kkt_meets_its_conditions():
    """The four conditions of the robust route's design, in the restatement, before any device run."""
    K, n, m, tiny, partners = pr.designed_kkt()
    F0 = pr.Factor(K, [])
    g, p = F0.multipliers()
    rep, rej = pr.report(g, 1e-8)
    # 1. exactly the designed columns are rejected, their multipliers exact powers of two, their partners the designed constraints
    assert sorted(rej) == list(tiny) and np.all(g[tiny] == 2.0 ** 40) and np.array_equal(p[tiny], partners)
    assert np.all(g[np.setdiff1d(np.arange(n + m), tiny)] < 1e4)
    b = np.random.default_rng(7).normal(size=n + m)
    # 2. the plain static solve is visibly inaccurate
    assert pr.omega(F0.Af, F0.solve(b), b) >= 1e-8
    # 3. the rounds end within three, below max_set
    flag, info, F = pr.robust_rounds(K, n, m, max_rounds=3)
    assert flag == 1 and info["rounds"] == 2 and info["rejected"] == [5, 0] and info["mode"] == "schur"
    assert np.array_equal(info["set"], np.sort(np.concatenate([tiny, partners]))) and len(info["set"]) < 64
    assert F.inertia() == (n, m, 0)
    # 4. the refined Schur-route solution reaches omega <= 2^-52
    x, ri = pr.solve_refine(F, b, 5)
    assert ri["status"] == 0 and ri["omega"] <= 2.0 ** -52
    # the second design (nothing rejected) and the third (the set would pass max_set)
    K2, n2, m2, _, _ = pr.designed_kkt(tiny=(), tiny_sigma=())
    flag2, info2, _ = pr.robust_rounds(K2, n2, m2)
    assert flag2 == 1 and info2["mode"] == "plain" and info2["rejected"] == [0] and len(info2["set"]) == 0
    K3, n3, m3, tiny3, _ = pr.designed_kkt(n=48, m=80, tiny=tuple(range(0, 36)), tiny_sigma=())
    try:
        pr.robust_rounds(K3, n3, m3)
        raised = False
    except RuntimeError as e:
        raised = "max_set" in str(e)
    assert raised and 2 * len(tiny3) > 64


def test_abi_symbols_and_no_device():
    """The new entry points exist with the declared signatures and refuse a host_symbolic_only handle with OKKT_ERR_NO_DEVICE."""
    lib = L.load()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktPivotInfo._fields_] == ["u", "rejected", "nonfinite_cols", "max_multiplier", "max_col", "seconds_device"]
    assert C.sizeof(L.OkktPivotInfo) == 48
    assert lib.okkt_pivot_report(None, 1e-8, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_multipliers(None, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_rejected_pivots(None, None, None, 0) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_solve_refine(None, None, None, None, 1, 3, 0.0, None, None) == L.OKKT_ERR_INVALID
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    A = sp.csc_matrix(np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0, 1.0, -2.0]]))
    h.analyze(A)
    info = L.OkktPivotInfo()
    g = np.zeros(3)
    p = np.zeros(3, dtype=np.int64)
    assert lib.okkt_pivot_report(h._h, 1e-8, C.byref(info)) == L.OKKT_ERR_NO_DEVICE
    assert "host_symbolic_only" in lib.okkt_last_error(h._h).decode()
    assert lib.okkt_get_multipliers(h._h, L.p_f64(g), L.p_i64(p)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_get_multipliers_dev(h._h, C.c_void_p(8), None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_get_rejected_pivots(h._h, L.p_i64(p), L.p_i64(p), 3) == L.OKKT_ERR_NO_DEVICE
    # the refinement through the Schur route: invalid outside Schur mode, no device in it
    b = np.ones(3)
    x = np.zeros(3)
    vals = L.f64(A.data)
    assert lib.okkt_schur_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, 3, 0.0, None, None) == L.OKKT_ERR_INVALID
    h.set_schur([2])
    h.analyze(A)
    assert lib.okkt_schur_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, 3, 0.0, None, None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_solve_refine_dev(h._h, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 1, 3, 0.0, None, None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), -1, 3, 0.0, None, None) == L.OKKT_ERR_INVALID
    finalize_b(h)
