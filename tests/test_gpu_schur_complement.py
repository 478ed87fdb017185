"""GPU tests of Schur mode (okkt_set_schur / okkt_factor_schur / okkt_get_schur / okkt_schur_condense / okkt_schur_expand, DESIGN.md
section 8.4): S against a dense NumPy reference (bound and its reason: tests/schur_case.py), the inertia identities, condense ->
dense solve -> expand against the whole-matrix solve, the factor and solve routes, refactorisation and bitwise reproducibility, and
a cleared set that changes nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_case as sc
from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kkt():
    return sc.kkt()


@pytest.fixture(scope="module")
def whole(kkt):
    K, n, m = kkt
    w = sc.whole_handle(K, n, m)
    yield w
    finalize_b(w)


@pytest.mark.parametrize("ns", [1, 17, 128, 129, 300])
def test_schur_symmetric_kkt(kkt, whole, ns):
    K, n, m = kkt
    idx = sc.mixed_set(n, m, ns, seed=ns)
    A11, _, _, _ = sc.dense_parts(K, idx)
    p1, q1 = sc.inertia_of(np.linalg.eigvalsh(A11))
    h, S = sc.check_schur(K, idx, p1, q1)
    # inertia(A11) from the pivots; inertia(A) = inertia(A11) + inertia(S) (Haynsworth) against the whole factorisation
    assert h.inertia[:2] == (p1, q1) and h.inertia[2:] == (0, 0)
    ps, qs = sc.inertia_of(np.linalg.eigvalsh(S))
    assert (p1 + ps, q1 + qs) == whole.inertia[:2]
    sc.check_solves(h, S, K, whole)
    finalize_b(h)


def test_schur_definite():
    prob = synth.make_problem(2500, 1500, seed=8, well_scaled=True)
    Q = synth.schur_matrix(prob, delta=1e-6)
    n = prob["n"]
    idx = np.random.default_rng(1).choice(n, 64, replace=False)
    h, S = sc.check_schur(Q, idx, n - 64, 0, sym="definite")
    assert h.inertia[:2] == (n - 64, 0)
    assert np.all(np.linalg.eigvalsh(S) > 0)      # S is positive definite exactly when A is
    w = sc.whole_handle(Q, n, 0, sym="definite")
    sc.check_solves(h, S, Q, w, nrhs_list=(1, 4))
    finalize_b(h)
    finalize_b(w)


def test_schur_block_angular_linking_columns():
    prob = synth.block_angular(nblocks=4, n_b=500, m_b=750, n_link=200)
    K = synth.augmented_matrix(prob, delta=1e-8)
    n, m = prob["n"], prob["m"]
    idx = np.arange(n - 200, n)                   # the linking x-columns
    h, S = sc.check_schur(K, idx, n - 200, m)
    w = sc.whole_handle(K, n, m)
    assert w.inertia[:2] == (n, m)
    assert np.all(np.linalg.eigvalsh(S) > 0)      # the linking block of a quasi-definite system: positive definite
    sc.check_solves(h, S, K, w, nrhs_list=(2,))
    finalize_b(h)
    finalize_b(w)


def test_routes_in_process():
    sc.routes()


@pytest.mark.parametrize("env", [{"OKKT_DATAFLOW": "0"}, {"OKKT_FLOW": "0"}], ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_routes_switched(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schur_case.py")], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SCHUR_OK" in r.stdout, (env, r.stdout[-400:], r.stderr[-1500:])


def test_refactor_and_reproducibility(kkt):
    K, n, m = kkt
    idx = sc.mixed_set(n, m, 129, seed=7)
    n1, m1 = n - int((idx < n).sum()), m - int((idx >= n).sum())
    h, S0 = sc.check_schur(K, idx, n1, m1)
    rng = np.random.default_rng(2)
    B = rng.normal(size=(3, n + m))
    R0 = h.schur_condense(B)
    # new values on the same plan: S follows
    K2 = K.copy()
    K2.data = K.data * 1.5
    assert h.ls_factor_schur(K2, n1, m1) == 1
    S2 = h.schur()
    Sref2 = sc.schur_ref(K2, idx)
    assert np.max(np.abs(S2 - Sref2)) <= sc.S_TOL * np.max(np.abs(Sref2))
    assert not np.array_equal(S2, S0)
    # back to the first values: bitwise the first S and r2, twice
    for _ in range(2):
        assert h.ls_factor_schur(K, n1, m1) == 1
        assert np.array_equal(h.schur(), S0)
        assert np.array_equal(h.schur_condense(B), R0)
    finalize_b(h)


def test_device_entry_points(kkt):
    K, n, m = kkt
    idx = sc.mixed_set(n, m, 40, seed=9)
    n1, m1 = n - int((idx < n).sum()), m - int((idx >= n).sum())
    h, S = sc.check_schur(K, idx, n1, m1)
    dim, ns, nrhs = n + m, 40, 3
    vals = np.asarray(K.data, dtype=np.float64)
    B = np.random.default_rng(4).normal(size=(nrhs, dim))
    d_vals = h.dev_upload(vals)
    assert h.ls_factor_schur_dev(d_vals, n1, m1) == 1
    ld = ns + 3
    d_S = h.dev_alloc(8 * ld * ns)
    h.schur_dev(d_S, ld)
    Sd = h.dev_download(d_S, (ns, ld))[:, :ns]
    assert np.array_equal(Sd, S)
    d_B = h.dev_upload(B)
    d_r2 = h.dev_alloc(8 * ns * nrhs)
    h.schur_condense_dev(d_B, d_r2, nrhs)
    R2 = h.dev_download(d_r2, (nrhs, ns))
    assert np.array_equal(R2, h.schur_condense(B))
    X2 = np.linalg.solve(S, R2.T).T
    d_x2 = h.dev_upload(X2)
    d_x = h.dev_alloc(8 * dim * nrhs)
    h.schur_expand_dev(d_B, d_x2, d_x, nrhs)
    assert np.array_equal(h.dev_download(d_x, (nrhs, dim)), h.schur_expand(B, X2))
    for p in (d_vals, d_S, d_B, d_r2, d_x2, d_x):
        h.dev_free(p)
    finalize_b(h)


def test_cleared_set_changes_nothing(kkt):
    K, n, m = kkt
    b = np.random.default_rng(5).normal(size=n + m)
    fresh = linear_solver_HIP("symmetric")
    initialize_b(fresh)
    assert fresh.ls_factor_b(K, n, m) == 1
    x0, d0 = fresh.ls_solve(b), fresh.diag()
    h = sc.schur_handle("symmetric", K, sc.mixed_set(n, m, 50, seed=3))
    assert h.ls_factor_schur(K, n - 25, m - 25) == 1
    h.set_schur([])
    assert h.ls_factor_b(K, n, m) == 1
    assert np.array_equal(h.diag(), d0)
    assert np.array_equal(h.ls_solve(b), x0)
    finalize_b(h)
    finalize_b(fresh)


def test_refusals_leave_the_handle_usable(kkt):
    K, n, m = kkt
    idx = sc.mixed_set(n, m, 20, seed=11)
    n1, m1 = n - int((idx < n).sum()), m - int((idx >= n).sum())
    h = sc.schur_handle("symmetric", K, idx)
    vals = np.asarray(K.data, dtype=np.float64)
    x = np.zeros(n + m)
    # no factor yet: the Schur exports are refused
    assert h._lib.okkt_get_schur(h._h, L.p_f64(np.zeros(400)), 20) == L.OKKT_ERR_INVALID
    assert h.ls_factor_schur(K, n1, m1) == 1
    refused = [
        h._lib.okkt_factor(h._h, L.p_f64(vals), n, m, L.OKKT_SYM_SYMMETRIC, None),
        h._lib.okkt_solve(h._h, L.p_f64(x), L.p_f64(x), 1),
        h._lib.okkt_solve_refine(h._h, L.p_f64(vals), L.p_f64(x), L.p_f64(x), 1, 2, 0.0, None, None),
        h._lib.okkt_condest(h._h, L.p_f64(vals), 2, None),
        h._lib.okkt_forward_error(h._h, L.p_f64(vals), L.p_f64(x), L.p_f64(x), 1, L.p_f64(np.zeros(1)), None),
        h._lib.okkt_dist_set_partition(h._h, 2, 0),
        h._lib.okkt_get_schur(h._h, L.p_f64(np.zeros(400)), 19),      # ld < ns
    ]
    assert refused == [L.OKKT_ERR_INVALID] * len(refused)
    assert h.ls_factor_schur(K, n1, m1) == 1
    sc.check_solves(h, h.schur(), K, sc.whole_handle(K, n, m), nrhs_list=(1,))
    # a NaN in A11 gives flag 0 with the non-finite pivot counted; the factor can still be exported
    bad = vals.copy()
    inner = np.setdiff1d(np.arange(n + m), idx)
    col = inner[0]
    p = K.indptr[col] + int(np.flatnonzero(K.indices[K.indptr[col]:K.indptr[col + 1]] == col)[0])
    bad[p] = np.nan
    assert h.ls_factor_schur(bad, n1, m1) == 0
    assert h.inertia[3] > 0
    h.schur()
    finalize_b(h)
