"""GMRES-based iterative refinement on the host (no GPU needed): the numpy restatement of okkt_solve_gmres (gmres_ref.py) against
dense solves on the system of the refinement's shifted-factor test, where plain refinement stalls; the C ABI symbols, signatures and
refusals through ctypes on the built library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import gmres_ref as gr  # noqa: E402

EPS = 2.0 ** -52
NEW = ("okkt_solve_gmres", "okkt_solve_gmres_dev")


def shifted_case(delta):
    """S-small, seed 1, well scaled: A = K(1e-4), F = K(1e-4 + delta) (the shift on the H block), b from default_rng(4)"""
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    A = synth.augmented_matrix(prob, delta=1e-4)
    F = synth.augmented_matrix(prob, delta=1e-4 + delta)
    b = np.random.default_rng(4).normal(size=prob["n"] + prob["m"])
    return gr.LongResidual(ft.full_csr(sp.tril(A))), gr.dense_solver(ft.full_csr(sp.tril(F))), b


@pytest.mark.parametrize("delta", [1.0, 10.0])
def test_restatement_converges_where_refinement_stalls(delta):
    resid, solve, b = shifted_case(delta)
    x, info = gr.gmres_ir(resid, solve, b, restart=30, max_iters=200)
    assert info["status"] == 0 and info["omega"] <= 4 * EPS, info
    _, om = resid(b, x)
    assert om == info["omega"]
    assert info["cycles"] <= 4 and info["iterations"] <= 80, info
    xp, wp, _ = gr.plain_ir(resid, solve, b, max_solves=info["solves"])
    if delta == 10.0:
        assert wp > 4 * EPS, (wp, info["solves"])    # rho(I - F^-1 A) = 0.78: plain refinement is far from 4 eps
        assert wp > 1e-10
    # the dense solution of A x = b agrees
    xd = np.linalg.solve(resid.M.toarray(), b)
    assert np.max(np.abs(x - xd)) <= 1e-8 * np.max(np.abs(xd))


def test_restatement_max_iters_zero_and_exact_factor():
    resid, solve, b = shifted_case(1.0)
    x, info = gr.gmres_ir(resid, solve, b, max_iters=0)
    assert np.array_equal(x, solve(b)) and info["iterations"] == 0 and info["status"] == 1
    assert info["omega"] == info["omega0"]
    resid, solve, b = shifted_case(0.0)              # F = A: converges with at most one short cycle
    x, info = gr.gmres_ir(resid, solve, b)
    assert info["status"] == 0 and info["cycles"] <= 1 and info["iterations"] <= 3, info


def test_symbols_and_signatures():
    lib = L.load()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktGmresInfo._fields_] == ["iterations", "cycles", "status", "solves", "omega0", "omega", "resid_inf",
                                                        "work_bytes"]
    assert C.sizeof(L.OkktGmresInfo) == 48


def test_null_handle_and_bad_arguments():
    lib = L.load()
    assert lib.okkt_solve_gmres(None, None, None, None, 1, 30, 10, 0.0, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_solve_gmres_dev(None, None, None, None, 1, 30, 10, 0.0, None, None) == L.OKKT_ERR_INVALID
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    A = sp.csc_matrix(np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0, 1.0, -2.0]]))
    h.analyze(A)
    lib = h._lib
    vals = L.f64(A.data)
    b = np.ones(3)
    x = np.zeros(3)
    om = np.zeros(1)
    info = L.OkktGmresInfo()
    # invalid arguments come first
    for nrhs, restart, max_iters, what in ((-1, 30, 10, "nrhs"), (1, 30, -1, "max_iters"), (1, 65, 10, "restart")):
        assert lib.okkt_solve_gmres(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), nrhs, restart, max_iters, 0.0, None, None) == L.OKKT_ERR_INVALID
        assert what in lib.okkt_last_error(h._h).decode()
        assert lib.okkt_solve_gmres_dev(h._h, None, None, None, nrhs, restart, max_iters, 0.0, None, None) == L.OKKT_ERR_INVALID
    # a host_symbolic_only handle has no device
    assert lib.okkt_solve_gmres(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, 30, 10, 0.0, C.byref(info), L.p_f64(om)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_solve_gmres_dev(h._h, None, None, None, 0, 0, 10, 0.0, None, None) == L.OKKT_ERR_NO_DEVICE
    with pytest.raises(OkktError):
        h.ls_solve_gmres(A, b)
    finalize_b(h)
