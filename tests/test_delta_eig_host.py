"""The host side of the Lanczos bound of the delta loop (no GPU needed): the tridiagonal solver of
okkt_kkt_min_eig through okkt_debug_tridiag_eig against numpy.linalg.eigvalsh, the C ABI symbols, the refusals that stand in front of
the device, the path of the options, and the restatement of the delta sequence in lanczos_ref.py against the recorded loops."""
import ctypes as C

import numpy as np
import pytest

import lanczos_ref as R
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS

NEW = ("okkt_kkt_min_eig", "okkt_kkt_ipopt_strategy_eig", "okkt_debug_tridiag_eig")
EPS = 2.0 ** -52


def tridiag(alpha, beta):
    """(rc, theta_min, theta_max, s, bound) of the hook; beta has len(alpha) entries, the last one the residual coefficient."""
    k = len(alpha)
    a, b = L.f64(np.asarray(alpha, float)), L.f64(np.asarray(beta, float))
    tmin, tmax, bound = C.c_double(), C.c_double(), C.c_double()
    s = np.zeros(k)
    rc = L.load().okkt_debug_tridiag_eig(k, L.p_f64(a), L.p_f64(b), C.byref(tmin), C.byref(tmax), L.p_f64(s), C.byref(bound))
    return rc, tmin.value, tmax.value, s, bound.value


def dense(alpha, beta):
    k = len(alpha)
    return np.diag(alpha) + np.diag(beta[: k - 1], 1) + np.diag(beta[: k - 1], -1)


def check(alpha, beta, vec_tol=None):
    """theta_min and theta_max to a few ulps of ||T||; s a unit vector with (T - theta_min) s at that level; the bound's definition."""
    alpha, beta = np.asarray(alpha, float), np.asarray(beta, float)
    rc, tmin, tmax, s, bound = tridiag(alpha, beta)
    assert rc == 0
    T = dense(alpha, beta)
    scale = max(np.max(np.abs(alpha)), np.max(np.abs(beta[: len(alpha) - 1])) if len(alpha) > 1 else 0.0)
    w = np.linalg.eigvalsh(T / scale) * scale if scale > 0 else np.zeros(len(alpha))
    k = len(alpha)
    tol = 16 * k * EPS * 3 * scale                      # eigvalsh's own backward error, k eps ||T||, and the bisection's last bit
    assert abs(tmin - w[0]) <= tol and abs(tmax - w[-1]) <= tol
    assert abs(np.linalg.norm(s) - 1.0) <= 8 * EPS and s[np.argmax(np.abs(s))] > 0.0
    r = (T / scale) @ s - (tmin / scale) * s if scale > 0 else np.zeros(k)
    assert np.linalg.norm(r) <= (vec_tol if vec_tol is not None else 64 * k * EPS)
    assert bound == abs(beta[k - 1] * s[k - 1])
    return tmin, tmax, s


def test_symbols_and_signatures():
    lib = L.load()
    for name in NEW:
        assert name in L.SIGNATURES and name not in L.MISSING
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktKktEigInfo._fields_] == ["theta_min", "theta_max", "bound", "rho", "rho_abs", "rho_margin", "resid", "steps",
                                                         "status", "seconds_device"]
    assert C.sizeof(L.OkktKktEigInfo) == 72
    assert C.sizeof(L.OkktOpts) == 72 and L.OkktOpts._fields_[-1][0] == "schur_dense_rows"      # okkt_opts keeps its layout


@pytest.mark.parametrize("k", [1, 2, 3, 17, 64])
def test_tridiagonal_against_eigvalsh(k):
    rng = np.random.default_rng(k)
    for trial in range(4):
        alpha = rng.normal(size=k) * 10.0 ** rng.integers(-2, 3)
        beta = np.abs(rng.normal(size=k)) * (1.0 if trial % 2 else 0.01)
        if trial == 3:
            beta = -beta                                  # the sign of the off-diagonal does not change the spectrum, only the vector's signs
        check(alpha, beta)


def test_tridiagonal_k1_is_the_entry():
    rc, tmin, tmax, s, bound = tridiag([-2.5], [0.75])
    assert (rc, tmin, tmax, bound) == (0, -2.5, -2.5, 0.75) and s[0] == 1.0


def test_tridiagonal_zero_beta_in_the_middle():
    # two blocks: the smallest eigenvalue sits in the second one, the vector is zero on the first
    alpha = np.array([3.0, 4.0, 5.0, -1.0, 2.0, 0.5])
    beta = np.array([0.5, 0.25, 0.0, 1.5, 0.75, 0.125])
    tmin, tmax, s = check(alpha, beta)
    assert np.all(s[:3] == 0.0) and np.linalg.norm(s[3:]) > 0.99
    # ... and in the first one
    tmin, tmax, s = check(alpha[::-1].copy(), np.array([0.75, 1.5, 0.0, 0.25, 0.5, 0.125]))
    assert np.all(s[3:] == 0.0)
    # every off-diagonal entry zero: the diagonal itself
    tmin, tmax, s = check(alpha, np.zeros(6))
    assert (tmin, tmax) == (-1.0, 5.0) and s[3] == 1.0
    # the zero matrix
    rc, tmin, tmax, s, bound = tridiag(np.zeros(5), np.zeros(5))
    assert (rc, tmin, tmax, bound) == (0, 0.0, 0.0, 0.0) and abs(np.linalg.norm(s) - 1.0) < 1e-15


def test_tridiagonal_clustered_alpha():
    # 64 diagonal entries within 1e-13 of 1 and a tiny coupling: every eigenvalue to a few ulps; any unit vector of the cluster is
    # an eigenvector to the cluster's width, which is what the residual is held to
    k = 64
    rng = np.random.default_rng(5)
    alpha = 1.0 + 1e-13 * rng.normal(size=k)
    beta = 1e-14 * np.abs(rng.normal(size=k))
    check(alpha, beta, vec_tol=1e-12)
    # two well-separated clusters
    alpha = np.concatenate([-2.0 + 1e-12 * rng.normal(size=8), 5.0 + 1e-12 * rng.normal(size=8)])
    check(alpha, 1e-3 * np.ones(16), vec_tol=1e-9)


def test_tridiagonal_entries_spanning_300_decades():
    alpha = np.array([1e150, -1e-150, 3e-150, 2.0, -1e150, 1e-150, 5e149, 1.0])
    beta = np.array([1e-150, 1e-150, 1.0, 1e100, 1e-150, 1e149, 1e-150, 1e-150])
    tmin, tmax, s = check(alpha, beta)
    assert np.isfinite(tmin) and np.isfinite(tmax) and np.all(np.isfinite(s))
    # all tiny: the scaling is exact, nothing underflows into the answer
    tmin, tmax, s = check(1e-150 * np.array([2.0, -1.0, 3.0]), 1e-150 * np.array([1.0, 0.5, 0.25]))
    assert tmin < 0.0 < tmax


def test_tridiagonal_refusals():
    lib = L.load()
    a = np.ones(65)
    out = [C.c_double() for _ in range(3)]
    s = np.zeros(65)
    args = (C.byref(out[0]), C.byref(out[1]), L.p_f64(s), C.byref(out[2]))
    assert lib.okkt_debug_tridiag_eig(65, L.p_f64(a), L.p_f64(a), *args) == L.OKKT_ERR_INVALID
    assert lib.okkt_debug_tridiag_eig(0, L.p_f64(a), L.p_f64(a), *args) == L.OKKT_ERR_INVALID
    assert lib.okkt_debug_tridiag_eig(3, None, L.p_f64(a), *args) == L.OKKT_ERR_INVALID
    bad = np.array([1.0, np.nan, 2.0])
    assert lib.okkt_debug_tridiag_eig(3, L.p_f64(bad), L.p_f64(a), *args) == L.OKKT_ERR_INVALID
    bad = np.array([1.0, np.inf, 2.0])
    assert lib.okkt_debug_tridiag_eig(3, L.p_f64(a), L.p_f64(bad), *args) == L.OKKT_ERR_INVALID


def test_null_handles_and_host_only_handle():
    lib = L.load()
    info = L.OkktKktEigInfo()
    nf, sk, d = C.c_int32(), C.c_int32(), C.c_double()
    assert lib.okkt_kkt_min_eig(None, 8, 0.0, 0, C.byref(info), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_kkt_ipopt_strategy_eig(None, 0.0, None, 8, 0, C.byref(nf), C.byref(d), C.byref(sk), None) == L.OKKT_ERR_INVALID
    o = L.OkktOpts()
    lib.okkt_default_opts(C.byref(o))
    o.host_symbolic_only = 1
    k = C.c_void_p()
    assert lib.okkt_kkt_create(C.byref(k), C.byref(o), L.OKKT_KKT_SYMMETRIC) == 0
    assert lib.okkt_kkt_min_eig(k, 8, 0.0, 0, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_kkt_min_eig(k, 8, 0.0, 0, C.byref(info), None) == L.OKKT_ERR_NO_DEVICE
    assert b"host_symbolic_only" in lib.okkt_kkt_last_error(k)
    assert lib.okkt_kkt_ipopt_strategy_eig(k, 0.0, None, 8, 0, None, C.byref(d), C.byref(sk), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_kkt_ipopt_strategy_eig(k, 0.0, None, 8, 0, C.byref(nf), C.byref(d), C.byref(sk), None) == L.OKKT_ERR_NO_DEVICE
    assert b"host_symbolic_only" in lib.okkt_kkt_last_error(k)
    assert sk.value == 0
    assert lib.okkt_kkt_destroy(k) == 0


def test_pars_defaults_pass_nothing_to_okkt_opts():
    pars = KS.Class_parameters()
    assert pars.kkt.hip_delta_eig_steps == 0 and pars.kkt.hip_delta_eig_scaled == 0
    assert KS.okkt_opts_from_pars(pars.kkt) == {}
    pars.kkt.hip_delta_eig_steps = 32
    pars.kkt.hip_delta_eig_scaled = 1
    assert KS.okkt_opts_from_pars(pars.kkt) == {}          # arguments of the strategy's entry point, not okkt_opts fields


def test_kkt_solver_keywords_stay_out_of_okkt_opts():
    pars = KS.Class_parameters()
    pars.kkt.kkt_solver_type = "symmetric"
    k0 = KS.pick_KKT_solver(pars)
    assert (k0.delta_eig_steps, k0.delta_eig_scaled, k0.skipped, k0.delta_eig_info) == (0, 0, 0, None)
    pars.kkt.hip_delta_eig_steps = 24
    k = KS.pick_KKT_solver(pars)
    assert (k.delta_eig_steps, k.delta_eig_scaled) == (24, 0)
    assert "hip_delta_eig_steps" not in k._opts and "hip_delta_eig_scaled" not in k._opts
    k2 = KS.HIP_KKT_solver("schur", pars, hip_delta_eig_steps=40, hip_delta_eig_scaled=1, ordering=3)
    assert (k2.delta_eig_steps, k2.delta_eig_scaled) == (40, 1)
    assert k2._opts == {"ordering": 3}


@pytest.mark.parametrize("prob", ["indef5", "posdiag_indef5"])
def test_delta_sequence_restates_the_recorded_loops(golden, prob):
    """lanczos_ref.delta_sequence against the attempts recorded from the reference (tests/golden): the same doubles, and the number of
    attempts an exact lambda_min would skip never reaches the last, successful one."""
    from conftest import iterate_from_record
    rec = golden[prob]
    it = iterate_from_record(rec, KS.Class_iterate)
    Q = R.dense_q(it)
    lam = float(np.linalg.eigvalsh(Q)[0])
    d = KS.Class_delta_parameters()
    for key, exp in rec["delta_loops"].items():
        prev = float(key.split("_prev")[1])
        seq = R.delta_sequence(float(np.min(np.diag(Q))), prev, d)
        tried = exp["tried"]
        assert [v for v, _ in seq[: len(tried)]] == tried
        nfac, last = R.attempts_until_success(seq, lam)
        assert (nfac, last) == (exp["num_fac"], exp["delta"])
        assert 0 <= R.exact_skips(seq, lam, d.max) <= nfac - 2 or nfac == 1
        if prev == 0.0:      # (what the parity tests on the GPU require of their inputs)
            assert R.margin_from_grid(seq, lam) >= 0.1
