"""Host side of the Schur route made whole: the new symbols and their signatures, the argument checks that come
before any device work, the answer of a host_symbolic_only handle, the NumPy restatement of the dense inverse's block recurrence
against numpy.linalg.inv, and the pivot margins of every designed input the GPU cases factor."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import dense_ldlt_ref as ref
import schur_factor_case as fc
import schur_route_case as rc
from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["okkt_schur_get_inverse", "okkt_schur_get_inverse_dev", "okkt_schur_inverse_nonfinite", "okkt_schur_selinv", "okkt_schur_logdet",
       "okkt_schur_condest", "okkt_schur_condest_dev", "okkt_schur_forward_error", "okkt_schur_forward_error_dev", "okkt_schur_solve_gmres",
       "okkt_schur_solve_gmres_dev"]


def test_symbols_and_signatures():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "okkt.h")).read()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
        assert re.search(r"\b" + name + r"\(", header), name
    for twin, plain in (("okkt_schur_condest", "okkt_condest"), ("okkt_schur_condest_dev", "okkt_condest_dev"),
                        ("okkt_schur_forward_error", "okkt_forward_error"), ("okkt_schur_forward_error_dev", "okkt_forward_error_dev"),
                        ("okkt_schur_solve_gmres", "okkt_solve_gmres"), ("okkt_schur_solve_gmres_dev", "okkt_solve_gmres_dev"),
                        ("okkt_schur_selinv", "okkt_selinv"), ("okkt_schur_logdet", "okkt_logdet")):
        assert L.SIGNATURES[twin] == L.SIGNATURES[plain]
    for m in ("schur_inverse", "schur_inverse_dev", "schur_selinv", "schur_logdet", "schur_condest", "schur_forward_error", "schur_solve_gmres",
              "schur_solve_gmres_dev", "condest_robust", "forward_error_robust", "selinv_robust", "logdet_robust", "ls_solve_gmres_robust"):
        assert callable(getattr(linear_solver_HIP, m))


def test_block_width_of_the_restatement_is_the_kernels():
    text = open(os.path.join(ROOT, "onephase.jl_amd", "csrc", "dense_ldlt.h")).read()
    assert int(re.search(r"constexpr int kDlIB = (\d+);", text).group(1)) == rc.B


def test_null_arguments():
    lib = L.load()
    z = np.zeros(4)
    sg = C.c_int32()
    v = C.c_double()
    info = L.OkktCondestInfo()
    inv = L.OKKT_ERR_INVALID
    # no handle
    assert lib.okkt_schur_get_inverse(None, L.p_f64(z), 2) == inv
    assert lib.okkt_schur_get_inverse_dev(None, None, 2) == inv
    assert lib.okkt_schur_inverse_nonfinite(None) == inv
    assert lib.okkt_schur_selinv(None, None) == inv
    assert lib.okkt_schur_logdet(None, C.byref(v), C.byref(sg)) == inv
    assert lib.okkt_schur_condest(None, L.p_f64(z), 2, C.byref(info)) == inv
    assert lib.okkt_schur_condest_dev(None, None, 2, C.byref(info)) == inv
    assert lib.okkt_schur_forward_error(None, L.p_f64(z), L.p_f64(z), L.p_f64(z), 1, L.p_f64(z), None) == inv
    assert lib.okkt_schur_forward_error_dev(None, None, None, None, 1, L.p_f64(z), None) == inv
    assert lib.okkt_schur_solve_gmres(None, None, None, None, 1, 30, 10, 0.0, None, None) == inv
    assert lib.okkt_schur_solve_gmres_dev(None, None, None, None, 1, 30, 10, 0.0, None, None) == inv


def host_handle(schur):
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    A = sp.csc_matrix(np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0, 1.0, -2.0]]))
    if schur:
        h.set_schur([2])
    h.analyze(A)
    return h, A


@pytest.mark.parametrize("schur", [False, True], ids=["plain", "schur-mode"])
def test_host_symbolic_only_and_null_pointers(schur):
    h, A = host_handle(schur)
    lib = h._lib
    vals, b, x, out = L.f64(A.data), np.ones(3), np.zeros(3), np.zeros(3)
    z = np.zeros(9)
    sg, v = C.c_int32(), C.c_double()
    inv, nodev = L.OKKT_ERR_INVALID, L.OKKT_ERR_NO_DEVICE
    # NULL arguments come first
    assert lib.okkt_schur_get_inverse(h._h, None, 1) == inv
    assert lib.okkt_schur_get_inverse_dev(h._h, None, 1) == inv
    assert lib.okkt_schur_logdet(h._h, None, C.byref(sg)) == inv
    assert lib.okkt_schur_logdet(h._h, C.byref(v), None) == inv
    assert lib.okkt_schur_condest(h._h, None, 2, None) == inv
    assert lib.okkt_schur_condest_dev(h._h, None, 2, None) == inv
    assert lib.okkt_schur_forward_error(h._h, L.p_f64(vals), None, L.p_f64(x), 1, L.p_f64(out), None) == inv
    assert lib.okkt_schur_forward_error(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, None, None) == inv
    assert lib.okkt_schur_forward_error_dev(h._h, None, None, None, 1, L.p_f64(out), None) == inv
    assert lib.okkt_schur_solve_gmres(h._h, L.p_f64(vals), None, L.p_f64(x), 1, 30, 10, 0.0, None, None) == inv
    assert lib.okkt_schur_solve_gmres_dev(h._h, None, None, None, 1, 30, 10, 0.0, None, None) == inv
    for nrhs, restart, max_iters, what in ((-1, 30, 10, "nrhs"), (1, 30, -1, "max_iters"), (1, 65, 10, "restart")):
        assert lib.okkt_schur_solve_gmres(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), nrhs, restart, max_iters, 0.0, None, None) == inv
        assert what in lib.okkt_last_error(h._h).decode()
    # then the handle has no device, in Schur mode or not
    assert lib.okkt_schur_get_inverse(h._h, L.p_f64(z), 3) == nodev
    assert lib.okkt_schur_get_inverse_dev(h._h, C.c_void_p(8), 3) == nodev
    assert lib.okkt_schur_selinv(h._h, None) == nodev
    assert lib.okkt_schur_logdet(h._h, C.byref(v), C.byref(sg)) == nodev
    assert lib.okkt_schur_condest(h._h, L.p_f64(vals), 2, None) == nodev
    assert lib.okkt_schur_condest_dev(h._h, C.c_void_p(8), 2, None) == nodev
    assert lib.okkt_schur_forward_error(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, L.p_f64(out), None) == nodev
    assert lib.okkt_schur_forward_error_dev(h._h, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 1, L.p_f64(out), None) == nodev
    assert lib.okkt_schur_solve_gmres(h._h, L.p_f64(vals), L.p_f64(b), L.p_f64(x), 1, 30, 10, 0.0, None, None) == nodev
    assert lib.okkt_schur_solve_gmres_dev(h._h, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 1, 30, 10, 0.0, None, None) == nodev
    assert lib.okkt_schur_inverse_nonfinite(h._h) == 0
    with pytest.raises(OkktError):
        h.schur_selinv()
    with pytest.raises(OkktError, match="ls_factor_robust has not succeeded"):
        h.condest_robust(A)
    finalize_b(h)


RESTATED = [("definite", ref.definite), ("antidiagonal", ref.antidiagonal), ("heavy_tail", ref.heavy_tail), ("spectrum", ref.spectrum)]


@pytest.mark.parametrize("n", [1, 2, 3, rc.B - 1, rc.B, rc.B + 1, 2 * rc.B + 1, 100])
@pytest.mark.parametrize("design", [d for d, _ in RESTATED])
def test_restated_recurrence_against_numpy(design, n):
    S = dict(RESTATED)[design](n)
    Z, r = rc.block_inverse(S)
    ref_inv = np.linalg.inv(rc.full(S))
    tol = max(1e-10, 100.0 * rc.EPS * np.linalg.cond(rc.full(S)))
    assert np.array_equal(Z, Z.T)
    assert np.max(np.abs(Z - ref_inv)) <= tol * np.max(np.abs(ref_inv)), (design, n)
    if design == "antidiagonal":      # every pivot 2 x 2: no block of the walk may split one
        bl = rc.blocks(r["D"])
        assert all(r["D"][c, c - 1] == 0.0 for c in bl[1:-1])


@pytest.mark.parametrize("p", rc.PAIRS)
def test_restated_recurrence_with_a_pair_on_a_block_edge(p):
    S = ref.pair_at(rc.PAIR_N, p)
    Z, r = rc.block_inverse(S)
    assert list(np.flatnonzero(r["ipiv"] < 0)) == [p, p + 1]
    bl = rc.blocks(r["D"])
    assert p + 1 not in bl      # the pair stays in one block
    if p == rc.B - 1:
        assert bl[1] == rc.B - 1      # the first block ended one column early
    ref_inv = np.linalg.inv(S)
    assert np.max(np.abs(Z - ref_inv)) <= 1e-10 * np.max(np.abs(ref_inv))


def test_every_designed_gpu_input_meets_the_pivot_margin():
    """what test_gpu_schur_route.py factors (the 2049 case apart: test_the_large_case_meets_the_pivot_margin)"""
    for name, ns, make in rc.dense_cases():
        if ns > 300:
            continue
        assert ref.bunch_kaufman(make())["margin"] >= fc.MARGIN_MIN, name


def test_the_large_case_meets_the_pivot_margin():
    (name, ns, make), = [c for c in rc.dense_cases() if c[1] > 300]
    assert ref.bunch_kaufman(make())["margin"] >= fc.MARGIN_MIN, name
