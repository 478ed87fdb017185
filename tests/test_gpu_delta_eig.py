"""The Lanczos bound on lambda_min(H + J' Sigma J) and the delta loop that skips certified attempts on the GPU:
okkt_kkt_min_eig against the dense restatement of lanczos_ref.py on designed small systems, and okkt_kkt_ipopt_strategy_eig against
okkt_kkt_ipopt_strategy on a twin handle -- the same status, the same delta, the same direction bit for bit, fewer factorisations.

Tolerances.  theta_min over the whole space (max_steps >= n, or status 2): 1e-10 ||Q||_2.  rho against the long-double Rayleigh quotient
of the returned vector: rho_margin, the library's own claim.  The inequality rho + rho_margin >= lambda_min is exact in exact arithmetic;
eigvalsh's lambda_min carries an error of its own, n eps ||Q||_2, which is allowed for (the long-double check of rho right beside it
is the sharp one: lambda_min <= rho(v) for every v).  bound >= |theta_min - nearest eigenvalue| holds for the exact Ritz pair; both
sides are computed to eps ||Q||_2, so the comparison carries the floor 1e-10 ||Q||_2 of the theta_min check.  The residual is compared
with its long-double value to the rounding of Q v, 2^-26 || |Q||v| || / ||v||, plus rho_margin (the rho it subtracts)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lanczos_ref as R
from conftest import iterate_from_record
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd.linear_system_solvers import OkktError

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TINY_TOL = 1e-300          # never reached: Lanczos runs to the step limit or to an invariant subspace


def formed(it, kind="symmetric", **opts):
    k = KS.HIP_KKT_solver(kind, **opts)
    k.initialize_b(it)
    k.form_system_b(it)
    return k


@functools.lru_cache(maxsize=None)
def op_case(n, variant):
    """(iterate, Q, eigenvalues of Q, ||Q||_2) of an operator design, computed once."""
    it = R.operator_design(KS.Class_iterate, n, variant)
    Q = R.dense_q(it)
    w = np.linalg.eigvalsh(Q)
    return it, Q, w, max(abs(w[0]), abs(w[-1]))


def check_estimate(it, Q, w, qnorm, sd, info, v, scaled, whole_space):
    n = Q.shape[0]
    assert info["status"] in (0, 1, 2) and 1 <= info["steps"] <= min(64, n)
    if scaled:
        Qop = R.scaled_q(Q, sd)
        wop = np.linalg.eigvalsh(Qop)
        opnorm = max(abs(wop[0]), abs(wop[-1]))
    else:
        Qop, wop, opnorm = Q, w, qnorm
    print(f"n={n} scaled={scaled} steps={info['steps']} status={info['status']} theta_min={info['theta_min']:.6e} lam_min(op)={wop[0]:.6e} "
          f"rho={info['rho']:.6e} lam_min={w[0]:.6e} margin={info['rho_margin']:.3e} bound={info['bound']:.3e} resid={info['resid']:.3e}")
    floor = 1e-10 * opnorm
    if whole_space or info["status"] == 2:
        assert abs(info["theta_min"] - wop[0]) <= floor
    assert wop[0] - floor <= info["theta_min"] and info["theta_max"] <= wop[-1] + floor      # Ritz values lie inside the spectrum
    assert info["bound"] >= np.min(np.abs(wop - info["theta_min"])) * (1.0 - 1e-8) - floor
    # the certificate, on the unscaled Q(0)
    rho_ld, resid_ld, rho_abs_ld, aqn = R.rayleigh_ld(it, v)
    assert info["rho_margin"] == 2.0 ** -26 * info["rho_abs"] and info["rho_abs"] >= 0.0
    assert abs(info["rho"] - rho_ld) <= info["rho_margin"]
    assert abs(info["rho_abs"] - rho_abs_ld) <= 2.0 ** -26 * rho_abs_ld
    assert info["rho"] + info["rho_margin"] >= w[0] - 4 * n * EPS * qnorm
    assert abs(info["resid"] - resid_ld) <= 2.0 ** -26 * aqn + info["rho_margin"] + 1e-300
    if whole_space and not scaled:
        assert abs(info["rho"] - w[0]) <= 1e-10 * qnorm + info["rho_margin"]


@pytest.mark.parametrize("scaled", [0, 1])
@pytest.mark.parametrize("variant", ["full", "m0", "h0"])
@pytest.mark.parametrize("n", [1, 2, 37, 1031])
def test_operator_and_estimate(n, variant, scaled):
    it, Q, w, qnorm = op_case(n, variant)
    k = formed(it)
    for steps in ((64, 3) if n <= 64 else (64, 5)):
        info, v = k.min_eig(steps, TINY_TOL, scaled)
        assert info["steps"] <= steps
        check_estimate(it, Q, w, qnorm, k.schur_diag, info, v, scaled, whole_space=steps >= n)
    # the default tolerance stops no later and certifies as well
    info, v = k.min_eig(0, 0.0, scaled)
    assert info["steps"] <= 32
    check_estimate(it, Q, w, qnorm, k.schur_diag, info, v, scaled, whole_space=False)
    if info["status"] == 0:
        assert info["bound"] <= 2.0 ** -4 * abs(info["theta_min"])
    k.finalize_b()


def test_lanes_per_row_edges_are_in_the_design():
    """The rows of the 'full' design hold lpr - 1, lpr and lpr + 1 entries for the lanes-per-row the handle picks, whatever it picks."""
    for n in (37, 1031):
        it = op_case(n, "full")[0]
        lens = set(np.diff(it.J.tocsr().indptr).tolist())
        lpr = R.pick_lpr(it.J.nnz, it.J.shape[0])
        want = {0, 1, lpr - 1, lpr, lpr + 1, 257, n - 1}       # (the full row skips the empty column of J)
        assert {min(v, n - 1) for v in want} <= lens
        assert np.any(np.diff(it.J.indptr) == 0) and np.any(np.diff(it.H.indptr) == 0)
        sig = it.y / it.s
        assert sig.min() <= 1e-8 * (1 + 1e-12) and sig.max() >= 1e8 * (1 - 1e-12)


def test_kinds_give_the_same_bits():
    it = op_case(37, "full")[0]
    got = []
    for kind, opts in (("schur", {}), ("schur_direct", {}), ("symmetric", {}), ("schur", {"schur_dense_rows": 20})):
        k = formed(it, kind, **opts)
        if opts:
            assert len(k.dense_rows()) >= 2
        info, v = k.min_eig(24, TINY_TOL, 0)
        got.append((info["rho"], info["theta_min"], info["bound"], info["steps"], v.tobytes()))
        k.finalize_b()
    assert all(g == got[0] for g in got[1:])


@pytest.mark.parametrize("scaled", [0, 1])
def test_two_calls_give_the_same_bits(scaled):
    it = op_case(1031, "full")[0]
    k = formed(it, "schur")

    def call(steps):
        info, v = k.min_eig(steps, TINY_TOL, scaled)
        info.pop("seconds_device")
        return {a: np.float64(b).tobytes() for a, b in info.items()}, v.tobytes()
    a = call(12)
    assert call(12) == a
    call(40)                       # the workspace grows
    assert call(12) == a
    k.finalize_b()


def _direction(k, it):
    k.kkt_associate_rhs_b(it, KS.Reduct_affine())
    k.compute_direction_b()
    return k.dir.x.tobytes(), k.dir.y.tobytes(), k.dir.s.tobytes()


def _resident_direction(k, n, m):
    dx, dy, ds = np.zeros(n), np.zeros(m), np.zeros(m)
    assert k._lib.okkt_kkt_get_direction(k._k, L.p_f64(dx), L.p_f64(dy), L.p_f64(ds)) == 0
    return dx.tobytes(), dy.tobytes(), ds.tobytes()


@pytest.mark.parametrize("kind", ["schur", "symmetric"])
def test_min_eig_touches_nothing_of_the_direction(kind):
    it = R.indefinite_design(KS.Class_iterate, 37, -3.7)
    n, m = it.dim(), it.ncon()
    k, twin = formed(it, kind), formed(it, kind)
    assert k.factor_b(16.0) == 1 and twin.factor_b(16.0) == 1
    d0 = _direction(k, it)
    assert _direction(twin, it) == d0
    for scaled in (0, 1):
        info, _ = k.min_eig(40, 0.0, scaled)
        assert info["status"] in (0, 1, 2)
        assert _resident_direction(k, n, m) == d0
    # the resident right-hand side is still the one of kkt_associate_rhs_b: a direction from it, on both handles
    k.compute_direction_b()
    twin.compute_direction_b()
    assert (k.dir.x.tobytes(), k.dir.y.tobytes(), k.dir.s.tobytes()) == (twin.dir.x.tobytes(), twin.dir.y.tobytes(), twin.dir.s.tobytes()) == d0
    k.finalize_b()
    twin.finalize_b()


# ---- the strategy ---------------------------------------------------------------------------------------------------------------------
def run_pair(it, kind, steps, scaled=0, delta_prev=0.0, delta_max=None):
    """okkt_kkt_ipopt_strategy and okkt_kkt_ipopt_strategy_eig on twin handles; the parity every case must show.  Returns
    (status, num_fac_old, num_fac_new, skipped, delta, info)."""
    out = []
    for eig in (0, steps):
        pars = KS.Class_parameters()
        if delta_max is not None:
            pars.delta.max = delta_max
        k = KS.HIP_KKT_solver(kind, pars, hip_delta_eig_steps=eig, hip_delta_eig_scaled=scaled)
        it.delta = delta_prev
        k.initialize_b(it)
        k.form_system_b(it)
        status, nfac, delta = k.ipopt_strategy_b(it)
        d = _direction(k, it)                      # a complete factor exists whatever the status
        out.append((status, nfac, delta, d, k.skipped, k.delta_eig_info))
        k.finalize_b()
    (s0, f0, d0, dir0, sk0, i0), (s1, f1, d1, dir1, sk1, i1) = out
    print(f"{kind} steps={steps} scaled={scaled}: status {s0}/{s1} delta {d0!r}/{d1!r} #fac {f0} -> {f1} + {sk1} skipped; "
          f"Lanczos steps {i1['steps']} rho {i1['rho']!r} margin {i1['rho_margin']!r}")
    assert sk0 == 0 and i0 is None
    assert s1 == s0 and d1 == d0                   # == on doubles
    assert f1 + sk1 == f0
    assert dir1 == dir0
    return s0, f0, f1, sk1, d0, i1


@functools.lru_cache(maxsize=None)
def indef_case(n, lam, cluster=1):
    it = R.indefinite_design(KS.Class_iterate, n, lam, cluster=cluster)
    Q = R.dense_q(it)
    w = np.linalg.eigvalsh(Q)
    seq = R.delta_sequence(float(np.min(np.diag(Q))), 0.0, KS.Class_delta_parameters())
    return it, w, seq


KINDS = ["schur", "schur_direct", "symmetric"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [-3.7, -4e-4, -900.0])
@pytest.mark.parametrize("n", [37, 1031])
def test_strategy_parity_isolated(n, lam, kind):
    it, w, seq = indef_case(n, lam)
    d = KS.Class_delta_parameters()
    # the inputs: lambda_min is the designed one and isolated, no attempt lies within 10 % of -lambda_min
    assert abs(w[0] - lam) <= 1e-12 * abs(lam) + 1e-14 and w[1] > 0.5
    assert R.margin_from_grid(seq, w[0]) >= 0.1
    exact = R.exact_skips(seq, w[0], d.max)
    nfac_ref, delta_ref = R.attempts_until_success(seq, w[0])
    assert exact >= 3
    status, f0, f1, skipped, delta, info = run_pair(it, kind, 64 if n <= 64 else 32)
    assert status == "success" and (f0, delta) == (nfac_ref, delta_ref)
    assert info["steps"] >= 1 and info["rho"] < 0.0
    if n <= 64:
        assert skipped == exact and f1 == 2            # what is left: the first attempt and the one that succeeds
    else:
        assert 1 <= skipped <= exact


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prob", ["indef5", "posdiag_indef5"])
def test_strategy_parity_golden(golden, prob, kind):
    rec = golden[prob]
    it = iterate_from_record(rec, KS.Class_iterate)
    Q = R.dense_q(it)
    w = np.linalg.eigvalsh(Q)
    d = KS.Class_delta_parameters()
    seq = R.delta_sequence(float(np.min(np.diag(Q))), 0.0, d)
    assert R.margin_from_grid(seq, w[0]) >= 0.1
    status, f0, f1, skipped, delta, info = run_pair(it, kind, 64)
    exp = rec["delta_loops"][("symmetric" if kind == "symmetric" else "schur") + "_prev0.0"]
    assert (status, f0, delta) == (exp["status"], exp["num_fac"], exp["delta"])
    assert skipped == R.exact_skips(seq, w[0], d.max)


@pytest.mark.parametrize("steps", [32, 6])
def test_strategy_parity_clustered(steps):
    """Four lowest eigenvalues within 0.3 %: whichever vector of the cluster Lanczos returns, every skipped attempt is one the
    reference's loop failed -- the counts add up, status and delta are the same, and no more is skipped than lambda_min allows."""
    it, w, seq = indef_case(1031, -3.7, 4)
    assert w[3] < -3.69 and w[4] > 0.5
    status, f0, f1, skipped, delta, info = run_pair(it, "schur", steps)
    assert status == "success"
    assert 0 <= skipped <= R.exact_skips(seq, w[0], KS.Class_delta_parameters().max)
    if skipped:
        assert -info["rho"] - info["rho_margin"] <= -w[0] + 4 * 1031 * EPS * max(abs(w[0]), abs(w[-1]))


@pytest.mark.parametrize("kind", KINDS)
def test_convex_iterate_pays_nothing(kind):
    it = R.convex_design(KS.Class_iterate, 37)
    status, f0, f1, skipped, delta, info = run_pair(it, kind, 32)
    assert (status, f0, f1, skipped, delta) == ("success", 1, 1, 0, 0.0)
    assert info["steps"] == 0 and info["rho"] == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_delta_max_below_the_needed_delta(kind):
    """The attempt above delta_max is factored whatever the bound says: the caller may still solve with its (failed) factor."""
    it, w, seq = indef_case(37, -3.7)
    status, f0, f1, skipped, delta, info = run_pair(it, kind, 64, delta_max=1e-3)
    assert status == "failure" and delta == 0.004096
    assert (f0, f1, skipped) == (6, 2, 4)


@pytest.mark.parametrize("scaled", [0, 1])
def test_delta_prev_nonzero(scaled):
    it, w, seq = indef_case(37, -3.7)
    status, f0, f1, skipped, delta, info = run_pair(it, "symmetric", 64, scaled=scaled, delta_prev=2.0)
    assert status == "success" and delta == (2.0 * KS.Class_delta_parameters().dec) * 8.0
    assert (f0, f1, skipped) == (3, 2, 1)
    it.delta = 0.0


def test_scaled_mode_skips_as_well():
    it, w, seq = indef_case(1031, -3.7)
    status, f0, f1, skipped, delta, info = run_pair(it, "schur", 32, scaled=1)
    assert 1 <= skipped <= R.exact_skips(seq, w[0], KS.Class_delta_parameters().max)


def test_refusals(golden):
    it = R.convex_design(KS.Class_iterate, 37)
    k = KS.HIP_KKT_solver("symmetric")
    k.initialize_b(it)
    k._set_structure(it)
    with pytest.raises(OkktError, match="okkt_kkt_form_system has not been called"):
        k.min_eig(8)
    k.form_system_b(it)
    with pytest.raises(OkktError, match="max_steps > 64"):
        k.min_eig(65)
    with pytest.raises(OkktError, match="scaled must be 0 or 1"):
        k.min_eig(8, 0.0, 2)
    info = L.OkktKktEigInfo()
    nf, sk, d = C.c_int32(), C.c_int32(), C.c_double()
    assert k._lib.okkt_kkt_ipopt_strategy_eig(k._k, 0.0, None, 65, 0, C.byref(nf), C.byref(d), C.byref(sk), C.byref(info)) == L.OKKT_ERR_INVALID
    assert b"max_steps > 64" in k._lib.okkt_kkt_last_error(k._k)
    info, v = k.min_eig(8)                              # the handle stays usable
    assert info["status"] in (0, 1, 2) and info["rho"] > 0.0
    k.finalize_b()
    rec = golden["toy_lps"][0]
    itc = iterate_from_record(rec, KS.Class_iterate)
    kc = KS.HIP_KKT_solver("clever_symmetric")
    kc.initialize_b(itc)
    kc.form_system_b(itc)
    with pytest.raises(OkktError, match="clever-symmetric"):
        kc.min_eig(8)
    assert kc._lib.okkt_kkt_ipopt_strategy_eig(kc._k, 0.0, None, 8, 0, C.byref(nf), C.byref(d), C.byref(sk), None) == L.OKKT_ERR_INVALID
    assert b"clever-symmetric" in kc._lib.okkt_kkt_last_error(kc._k)
    assert kc.factor_b(1e-8) == 1                       # usable afterwards
    kc.finalize_b()
