"""The delta loop with its attempts factored `width` at a time as one uniform batch (okkt_kkt_ipopt_strategy_batch, DESIGN.md section
8.15) against okkt_kkt_ipopt_strategy on a twin handle: the same status, delta, serial attempt count, diagonal-dominance warnings and
direction, as bytes; the number of batched factorisations is ceil(attempts needed / width), computed from the sequence of
lanczos_ref.py; the refusals leave the handle to the serial loop."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import lanczos_ref as R
from conftest import iterate_from_record
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd.linear_system_solvers import OkktError

pytestmark = pytest.mark.gpu

KINDS = ["schur", "schur_direct", "symmetric"]
WIDTHS = [1, 2, 4, 16]


def _direction(k, it):
    k.kkt_associate_rhs_b(it, KS.Reduct_affine())
    k.compute_direction_b()
    return k.dir.x.tobytes(), k.dir.y.tobytes(), k.dir.s.tobytes()


def solver(it, kind, delta_prev=0.0, delta_max=None, **opts):
    pars = KS.Class_parameters()
    if delta_max is not None:
        pars.delta.max = delta_max
    k = KS.HIP_KKT_solver(kind, pars, **opts)
    it.delta = delta_prev
    k.initialize_b(it)
    k.form_system_b(it)
    return k


def serial(it, kind, **kw):
    """The serial loop on a handle of its own: (status, num_fac, delta, warnings, direction)."""
    k = solver(it, kind, **kw)
    status, nfac, delta = k.ipopt_strategy_b(it)
    assert k.delta_loop == "serial"
    out = (status, nfac, delta, k.diag_dom_warnings, _direction(k, it))      # a complete factor exists whatever the status
    k.finalize_b()
    return out


def run_pair(it, kind, widths=WIDTHS, **kw):
    """Every width on a twin handle against the serial loop; returns (status, num_fac, delta, {width: launches})."""
    s0, f0, d0, w0, dir0 = serial(it, kind, **kw)
    launches = {}
    for width in widths:
        k = solver(it, kind, **kw)
        status, nfac, delta, launches[width] = k.ipopt_strategy_batch(it, width)
        print(f"{kind} width={width}: status {s0}/{status} delta {d0!r}/{delta!r} #fac {f0}/{nfac} launches {launches[width]}")
        assert (status, nfac, k.diag_dom_warnings) == (s0, f0, w0)
        assert np.float64(delta).tobytes() == np.float64(d0).tobytes()
        assert _direction(k, it) == dir0
        assert launches[width] == math.ceil(f0 / width)
        k.finalize_b()
    it.delta = 0.0
    return s0, f0, d0, launches


@functools.lru_cache(maxsize=None)
def indef_case(n, lam):
    it = R.indefinite_design(KS.Class_iterate, n, lam)
    Q = R.dense_q(it)
    w = np.linalg.eigvalsh(Q)
    seq = R.delta_sequence(float(np.min(np.diag(Q))), 0.0, KS.Class_delta_parameters())
    return it, w, seq


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [-3.7, -4e-4, -900.0])
def test_parity_isolated(lam, kind):
    it, w, seq = indef_case(37, lam)
    assert R.margin_from_grid(seq, w[0]) >= 0.1          # the input: no attempt within 10 % of -lambda_min
    nfac_ref, delta_ref = R.attempts_until_success(seq, w[0])
    status, nfac, delta, launches = run_pair(it, kind)
    assert (status, nfac, delta) == ("success", nfac_ref, delta_ref)
    assert launches == {width: math.ceil(nfac_ref / width) for width in WIDTHS}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prob", ["indef5", "posdiag_indef5"])
def test_parity_golden(golden, prob, kind):
    rec = golden[prob]
    it = iterate_from_record(rec, KS.Class_iterate)
    status, nfac, delta, launches = run_pair(it, kind)
    exp = rec["delta_loops"][("symmetric" if kind == "symmetric" else "schur") + "_prev0.0"]
    assert (status, nfac, delta) == (exp["status"], exp["num_fac"], exp["delta"])


@pytest.mark.parametrize("kind", KINDS)
def test_convex_iterate_is_one_attempt_and_one_launch(kind):
    it = R.convex_design(KS.Class_iterate, 37)
    status, nfac, delta, launches = run_pair(it, kind)
    assert (status, nfac, delta) == ("success", 1, 0.0)
    assert set(launches.values()) == {1}


@pytest.mark.parametrize("kind", KINDS)
def test_delta_max_below_the_needed_delta(kind):
    """The attempt above delta_max ends the loop as a failure and leaves a complete factor to solve with (run_pair solves with it)."""
    it, w, seq = indef_case(37, -3.7)
    status, nfac, delta, launches = run_pair(it, kind, delta_max=1e-3)
    assert (status, nfac, delta) == ("failure", 6, 0.004096)
    assert launches == {1: 6, 2: 3, 4: 2, 16: 1}


def test_delta_prev_nonzero():
    it, w, seq = indef_case(37, -3.7)
    status, nfac, delta, launches = run_pair(it, "symmetric", delta_prev=2.0)
    assert status == "success" and delta == (2.0 * KS.Class_delta_parameters().dec) * 8.0 and nfac == 3
    assert launches == {1: 3, 2: 2, 4: 1, 16: 1}


def test_option_takes_the_batched_loop_where_it_applies():
    it, w, seq = indef_case(37, -3.7)
    s0, f0, d0, w0, dir0 = serial(it, "symmetric")
    k = solver(it, "symmetric", hip_delta_batch=4)
    assert k.ipopt_strategy_b(it) == (s0, f0, d0)
    assert (k.delta_loop, k.delta_launches) == ("batch", math.ceil(f0 / 4))
    assert _direction(k, it) == dir0
    k.finalize_b()
    # a plan with big fronts: the option falls back to the serial loop and says so
    big, _, _ = indef_case(1031, -3.7)
    s1, f1, d1, _, dir1 = serial(big, "schur")
    k = solver(big, "schur", hip_delta_batch=4)
    assert k.ipopt_strategy_b(big) == (s1, f1, d1)
    assert (k.delta_loop, k.delta_launches) == ("serial", None)
    assert _direction(k, big) == dir1
    k.finalize_b()
    it.delta = big.delta = 0.0


def _raw(k, width, delta_prev=0.0):
    nf, la, d = C.c_int32(), C.c_int32(), C.c_double()
    rc = k._lib.okkt_kkt_ipopt_strategy_batch(k._k, delta_prev, None, width, C.byref(nf), C.byref(d), C.byref(la))
    return rc, k._lib.okkt_kkt_last_error(k._k).decode()


def test_refusals_leave_the_serial_loop(golden):
    it, w, seq = indef_case(37, -3.7)
    s0, f0, d0, w0, dir0 = serial(it, "symmetric")
    # width out of range
    k = solver(it, "symmetric")
    for width in (0, 65, -3):
        rc, msg = _raw(k, width)
        assert rc == L.OKKT_ERR_INVALID and "width outside" in msg
    assert k.ipopt_strategy_b(it) == (s0, f0, d0) and _direction(k, it) == dir0
    k.finalize_b()
    # the linear solver's scaling on
    k = solver(it, "symmetric", hip_ls_scaling=1)
    rc, msg = _raw(k, 4)
    assert rc == L.OKKT_ERR_INVALID and "scaling" in msg
    with pytest.raises(OkktError, match="scaling"):
        k.ipopt_strategy_batch(it, 4)
    assert k.ipopt_strategy_b(it)[0] == s0 and k.delta_loop == "serial"
    k.finalize_b()
    # big fronts
    big, _, _ = indef_case(1031, -3.7)
    s1, f1, d1, _, dir1 = serial(big, "schur")
    k = solver(big, "schur")
    rc, msg = _raw(k, 4)
    assert rc == L.OKKT_ERR_INVALID and "takes no batch" in msg
    assert k.ipopt_strategy_b(big) == (s1, f1, d1) and _direction(k, big) == dir1
    k.finalize_b()
    # the clever-symmetric kind
    itc = iterate_from_record(golden["toy_lps"][0], KS.Class_iterate)
    kc = KS.HIP_KKT_solver("clever_symmetric")
    kc.initialize_b(itc)
    kc.form_system_b(itc)
    rc, msg = _raw(kc, 4)
    assert rc == L.OKKT_ERR_INVALID and "clever-symmetric" in msg
    twin = KS.HIP_KKT_solver("clever_symmetric")
    twin.initialize_b(itc)
    twin.form_system_b(itc)
    itc.delta = 0.0
    want = twin.ipopt_strategy_b(itc)
    itc.delta = 0.0
    assert kc.ipopt_strategy_b(itc) == want and kc.delta_loop == "serial"      # the serial loop runs on the refused handle
    assert _direction(kc, itc) == _direction(twin, itc)
    itc.delta = 0.0
    assert kc.factor_b(1e-8) == 1
    twin.finalize_b()
    kc.finalize_b()
    # before form_system, and NULL outputs
    k = KS.HIP_KKT_solver("symmetric")
    k.initialize_b(it)
    k._set_structure(it)
    rc, msg = _raw(k, 4)
    assert rc == L.OKKT_ERR_INVALID and "form_system" in msg
    assert k._lib.okkt_kkt_ipopt_strategy_batch(k._k, 0.0, None, 4, None, None, None) == L.OKKT_ERR_INVALID
    k.finalize_b()
    it.delta = big.delta = 0.0
