"""Refinement with extra-precise residuals on the host: the C ABI symbols and signatures, the refusal on a host-symbolic-only
handle, and the path of the KKT options, which are a setter of the handle and never okkt_opts fields (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

NEW = ("okkt_residual", "okkt_residual_dev", "okkt_solve_refine", "okkt_solve_refine_dev", "okkt_kkt_set_ls_refine")


def test_symbols_and_signatures():
    lib = L.load()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktRefineInfo._fields_] == ["steps", "status", "omega0", "omega", "resid_inf"]
    assert C.sizeof(L.OkktRefineInfo) == 32
    # okkt_opts keeps its layout: no field was added
    assert C.sizeof(L.OkktOpts) == 72 and L.OkktOpts._fields_[-1][0] == "schur_dense_rows"


def _host_only_handle():
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    A = sp.csc_matrix(np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0, 1.0, -2.0]]))
    h.analyze(A)
    return h, A


def test_host_symbolic_only_refuses_refinement():
    h, A = _host_only_handle()
    lib = h._lib
    n = 3
    vals = L.f64(A.data)
    b = np.ones(n)
    x = np.zeros(n)
    r = np.zeros(n)
    om = np.zeros(1)
    info = L.OkktRefineInfo()
    assert lib.okkt_residual(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), L.p_f64(r), 1, L.p_f64(om)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_residual_dev(h._h, None, None, None, None, 1, None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, 2, 0.0, C.byref(info), L.p_f64(om)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_solve_refine_dev(h._h, None, None, None, 0, 2, 0.0, None, None) == L.OKKT_ERR_NO_DEVICE
    # invalid arguments come first
    assert lib.okkt_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, -1, 0.0, None, None) == L.OKKT_ERR_INVALID
    assert "max_steps" in lib.okkt_last_error(h._h).decode()
    assert lib.okkt_solve_refine(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), -1, 1, 0.0, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_residual(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), L.p_f64(r), -1, None) == L.OKKT_ERR_INVALID
    with pytest.raises(OkktError):
        h.ls_solve_refine(A, b)
    with pytest.raises(OkktError):
        h.residual(A, b, x)
    finalize_b(h)


def test_null_handles():
    lib = L.load()
    assert lib.okkt_residual(None, None, None, None, None, 1, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_solve_refine(None, None, None, None, 1, 1, 0.0, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_kkt_set_ls_refine(None, 1, 0.0) == L.OKKT_ERR_INVALID


def test_pars_defaults_pass_nothing_to_okkt_opts():
    pars = KS.Class_parameters()
    assert pars.kkt.hip_ls_refine_steps == 0 and pars.kkt.hip_ls_refine_tol == 0.0
    assert KS.okkt_opts_from_pars(pars.kkt) == {}
    pars.kkt.hip_ls_refine_steps = 3
    pars.kkt.hip_ls_refine_tol = 1e-15
    assert KS.okkt_opts_from_pars(pars.kkt) == {}          # not okkt_opts fields, whatever their values
    pars.kkt.hip_ordering = 3
    assert KS.okkt_opts_from_pars(pars.kkt) == {"ordering": 3}


def test_kkt_solver_keywords_stay_out_of_okkt_opts():
    pars = KS.Class_parameters()
    pars.kkt.kkt_solver_type = "symmetric"
    pars.kkt.hip_ls_refine_steps = 2
    k = KS.pick_KKT_solver(pars)
    assert (k.ls_refine_steps, k.ls_refine_tol) == (2, 0.0)
    assert "hip_ls_refine_steps" not in k._opts and "hip_ls_refine_tol" not in k._opts
    k2 = KS.HIP_KKT_solver("symmetric", pars, hip_ls_refine_steps=4, hip_ls_refine_tol=1e-14, ordering=3)
    assert (k2.ls_refine_steps, k2.ls_refine_tol) == (4, 1e-14)
    assert k2._opts == {"ordering": 3}
    for key in k2._opts:                                   # what is left is an okkt_opts field
        assert hasattr(L.OkktOpts(), key)
