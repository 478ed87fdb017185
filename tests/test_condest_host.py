"""The condition estimator's numpy restatement (condest_ref.py), driven by exact dense solves, against numpy.linalg.cond(A, 1); the
C ABI of the estimate and its refusal on a host-symbolic-only handle (no GPU needed)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import condest_ref as cr  # noqa: E402
import front_trees as ft  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kkt_known_answers.json")
NEW = ("okkt_condest", "okkt_condest_dev", "okkt_condest_indices", "okkt_forward_error", "okkt_forward_error_dev", "okkt_kkt_condest",
       "okkt_kkt_direction_error_bound")


def laplacian_2d(k, shift):
    """The 5-point Laplacian on a k x k grid plus a diagonal shift graded from shift to 1.5 shift along the numbering: an M-matrix, so its
    inverse is entrywise nonnegative.  The grading breaks the grid's mirror symmetry, whose mirrored columns of F^-1 would tie in
    1-norm and row inf-norm (a near-tie the device and the host could break differently)."""
    T = sp.diags([-np.ones(k - 1), 4.0 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
    E = sp.diags([np.ones(k - 1), np.ones(k - 1)], [-1, 1])
    A = sp.kron(sp.eye(k), T) + sp.kron(E, -sp.eye(k)) + sp.diags(shift * (1.0 + 0.5 * np.arange(k * k) / (k * k)))
    return A.toarray()


def kkt_dense(H, J, s, y, delta):
    n, m = H.shape[0], J.shape[0]
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H + delta * np.eye(n)
    K[n:, :n] = J
    K[:n, n:] = J.T
    K[n:, n:] = -np.diag(s / y)
    return K


def kkt_cases():
    """The indefinite / quasi-definite list: S-small, the golden toy_lp0-8 and the "ipm" front designs of n <= 4000."""
    out = []
    prob = synth.make_config("S-small", seed=3, well_scaled=True)
    out.append(("S-small", cr.dense_symmetric(synth.augmented_matrix(prob, delta=1e-8))))
    for rec in json.load(open(GOLDEN))["toy_lps"]:
        n, m = rec["n"], rec["m"]
        H = np.array(rec["H_lower"], float).reshape(n, n)
        H = np.tril(H) + np.tril(H, -1).T
        J = np.array(rec["J"], float).reshape(m, n)
        out.append((rec["name"], kkt_dense(H, J, np.array(rec["s"]), np.array(rec["y"]), rec["delta"])))
    for name in IPM_DESIGNS:
        b = ft.build(ft.DESIGNS[name][0], "ipm")
        out.append((name + "/ipm", cr.dense_symmetric(b.A)))
    return out


IPM_DESIGNS = ["small-classes-f32-33-64-65-128-129", "edge-k385-c1", "fan-in-8", "mixed-level"]


def test_symbols_and_struct():
    lib = L.load()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktCondestInfo._fields_] == ["norm1", "inv_norm1", "cond1", "iterations", "solves", "status"]
    assert C.sizeof(L.OkktCondestInfo) == 40
    assert C.sizeof(L.OkktRefineInfo) == 32 and C.sizeof(L.OkktOpts) == 72


def test_host_symbolic_only_refuses():
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    A = sp.csc_matrix(np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0, 1.0, -2.0]]))
    h.analyze(A)
    vals = L.f64(A.data)
    info = L.OkktCondestInfo()
    fe = np.zeros(1)
    assert h._lib.okkt_condest(h._h, L.p_f64(vals), 2, C.byref(info)) == L.OKKT_ERR_NO_DEVICE
    assert h._lib.okkt_forward_error(h._h, L.p_f64(vals), L.p_f64(np.ones(3)), L.p_f64(np.ones(3)), 1, L.p_f64(fe), None) == L.OKKT_ERR_NO_DEVICE
    assert h._lib.okkt_forward_error(h._h, L.p_f64(vals), None, None, -1, None, None) == L.OKKT_ERR_INVALID
    with pytest.raises(OkktError):
        h.condest(A)
    finalize_b(h)


def test_generator_heads_and_determinism():
    # the head rows give the class, so columns of different classes are never parallel; the rest is fixed by (draw, row)
    for n in (1, 2, 3, 4, 50):
        H = min(n, 4)
        cols = [cr.gen_column(d, c, n) for d, c in enumerate(range(1 << (H - 1)))]
        for a in range(len(cols)):
            for b in range(a):
                assert abs(cols[a] @ cols[b]) < n
    a = cr.gen_column(7, 3, 1000)
    assert np.array_equal(a, cr.gen_column(7, 3, 1000)) and not np.array_equal(a, cr.gen_column(8, 3, 1000))
    assert 400 < (a > 0).sum() < 600


@pytest.mark.parametrize("t", [1, 2, 4])
def test_diagonal_exact(t):
    d = np.random.default_rng(1).uniform(-1.0, 1.0, size=300) * 10.0 ** np.random.default_rng(2).uniform(-6, 6, size=300)
    F = np.diag(d)
    n1, est, r = cr.condest(F, t)
    exact = np.linalg.cond(F, 1)
    assert abs(n1 * est - exact) <= 1e-12 * exact, (n1 * est, exact, r)


@pytest.mark.parametrize("t", [1, 2, 4])
def test_laplacian_exact(t):
    # F^-1 >= 0: the second iteration finds the maximal column
    F = laplacian_2d(60, 1e-3)
    n1, est, r = cr.condest(F, t)
    exact = np.linalg.cond(F, 1)
    assert F.shape[0] == 3600
    assert abs(n1 * est - exact) <= 1e-12 * exact, (n1 * est, exact, r)
    assert r["status"] == 0 and r["iterations"] <= 3


@pytest.mark.parametrize("t", [1, 2, 4])
def test_kkt_lower_bound_within_three(t):
    for name, F in kkt_cases():
        n1, est, r = cr.condest(F, t)
        exact = np.linalg.cond(F, 1)
        assert n1 * est <= exact * (1 + 1e-10), (name, n1 * est, exact)
        assert n1 * est >= exact / 3.0, (name, n1 * est, exact, r)
        assert r["iterations"] <= cr.ITMAX and r["status"] in (0, 1)


def test_two_runs_identical():
    for name, F in kkt_cases()[:4] + [("lap", laplacian_2d(20, 0.1))]:
        a = cr.condest(F, 2)
        b = cr.condest(F, 2)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], name


def test_singular_is_non_finite():
    # a solve that produces a non-finite value (an exact zero pivot) ends the estimate at once
    D = np.array([1.0, 2.0, 0.0, 3.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = cr.estimate(lambda B: B / D[:, None], 4, 2)
    assert r["status"] == 3 and r["est"] == np.inf and r["solves"] == 1
