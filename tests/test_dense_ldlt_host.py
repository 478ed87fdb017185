"""CPU tests around the dense factor of the Schur complement: the NumPy restatement of the Bunch-Kaufman
factorisation (tests/dense_ldlt_ref.py) reconstructs P S P', agrees in inertia with eigvalsh and in its pivots with LAPACK's dsytrf on
the designed inputs of the GPU tests, every seed of those inputs keeps its smallest comparison margin above the bound below which the
GPU tests could not ask for the same ipiv; the new entry points exist with their ctypes signatures and refuse what needs no device."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg.lapack

import dense_ldlt_ref as ref
from onephase_jl_amd import _lib as L

ORDERS = [1, 2, 3, 63, 64, 65, 129, 300]
DESIGNS = {"antidiagonal": ref.antidiagonal, "definite": ref.definite, "heavy_tail": ref.heavy_tail, "spectrum": ref.spectrum,
           "singular": ref.singular}


def cases():
    for name in sorted(DESIGNS):
        for ns in ORDERS:
            if name == "singular" and ns < 3:
                continue
            yield pytest.param(name, ns, id=f"{name}-{ns}")
    for p in (29, 30, 31, 62, 63, 64):
        yield pytest.param(f"pair_at-{p}", 129, id=f"pair_at-{p}")


def build(name, ns):
    return ref.pair_at(ns, int(name.split("-")[1])) if name.startswith("pair_at") else DESIGNS[name](ns)


@pytest.mark.parametrize("name,ns", list(cases()))
def test_restatement(name, ns):
    S = build(name, ns)
    r = ref.bunch_kaufman(S)
    # the seeds are fixed so that no decision is within rounding of a tie (the GPU tests compare ipiv exactly)
    assert r["margin"] >= 1e-8, r["margin"]
    # reconstruction: at LAPACK's level (same rule as for the device factor: 8 x dsytrf's own error + ns eps max|S|)
    err = ref.reconstruction_error(S, r["L"], r["D"], r["perm"])
    assert err <= 8.0 * ref.scipy_reconstruction_error(S) + ns * 2.0**-52 * np.max(np.abs(S)), err
    assert np.array_equal(np.tril(r["L"]), r["L"]) and np.all(np.diag(r["L"]) == 1.0)
    # inertia
    zero = 1 if name == "singular" else 0
    assert r["inertia"] == ref.inertia_eig(S, drop=zero)
    # the same pivots as dsytrf, and its layout unpacks to the same factor form
    ld, piv, info = scipy.linalg.lapack.dsytrf(S, lower=1)
    assert np.array_equal(piv, r["ipiv"])
    Lf, Df, perm = ref.unpack_lapack(ld, piv)
    assert np.array_equal(perm, r["perm"])
    assert ref.reconstruction_error(S, Lf, Df, perm) <= 8.0 * ref.scipy_reconstruction_error(S) + ns * 2.0**-52 * np.max(np.abs(S))


def test_one_large_order_keeps_its_margins():
    for name in ("antidiagonal", "definite", "heavy_tail", "spectrum"):
        assert ref.bunch_kaufman(DESIGNS[name](1100))["margin"] >= 1e-8, name


def test_designs_do_what_they_are_for():
    assert np.all(ref.bunch_kaufman(ref.antidiagonal(64))["ipiv"] < 0)
    assert np.array_equal(ref.bunch_kaufman(ref.definite(129))["ipiv"], np.arange(1, 130))
    piv = ref.bunch_kaufman(ref.heavy_tail(300))["ipiv"]
    far = [k for k, p in enumerate(piv) if abs(abs(int(p)) - 1 - k) >= 32]
    assert len(far) >= 30      # interchanges far beyond the 32 columns of a panel, all along the factorisation
    for p in (30, 31, 63, 64):
        assert list(np.flatnonzero(ref.bunch_kaufman(ref.pair_at(129, p))["ipiv"] < 0)) == [p, p + 1]
    assert ref.bunch_kaufman(ref.singular(65))["inertia"][2] == 1


def test_symbols_and_signatures():
    lib = L.load()
    ip, f64p, vp = C.POINTER(L.OkktInertia), C.POINTER(C.c_double), C.c_void_p
    want = {
        "okkt_schur_factor": [vp, f64p, C.c_int64, ip, ip],
        "okkt_schur_factor_dev": [vp, vp, C.c_int64, ip, ip],
        "okkt_schur_dense_solve": [vp, f64p, f64p, C.c_int64],
        "okkt_schur_dense_solve_dev": [vp, vp, vp, C.c_int64],
        "okkt_schur_solve": [vp, f64p, f64p, C.c_int64],
        "okkt_schur_solve_dev": [vp, vp, vp, C.c_int64],
        "okkt_schur_get_factor": [vp, f64p, C.c_int64, C.POINTER(C.c_int32)],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name


def test_refusals_without_a_device():
    lib = L.load()
    x = np.zeros(4)
    ipiv = np.zeros(2, dtype=np.int32)
    # a handle cannot be created without a device: what is left is the null handle, refused by every new entry point
    assert lib.okkt_schur_factor(None, None, 2, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_factor_dev(None, None, 2, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_dense_solve(None, L.p_f64(x), L.p_f64(x), 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_dense_solve_dev(None, None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_solve(None, L.p_f64(x), L.p_f64(x), 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_solve_dev(None, None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_get_factor(None, L.p_f64(x), 2, ipiv.ctypes.data_as(C.POINTER(C.c_int32))) == L.OKKT_ERR_INVALID
