"""GPU tests of the dense factor of the Schur complement (okkt_schur_factor / okkt_schur_dense_solve / okkt_schur_solve /
okkt_schur_get_factor): designed dense inputs through the caller-supplied path against the NumPy restatement
(ipiv), eigvalsh (inertia) and LAPACK (accuracy; the rules and their reason: tests/schur_factor_case.py), the assembled S, systems
that need the pivoting, the fused solve against its three-call form, the device entry points, the refusals and the interior routes.

Orders: 1, 2, 3 (no panel to speak of), 63, 64, 65 (around two panels of 31 or 32 columns and one 64-wide block of the substitutions),
129 and 300 (several panels, trailing tiles off the diagonal), 1100 (36 panels, a panel taller than the 1024 rows one pass of the
panel's workgroup covers)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ldlt_ref as ref
import schur_case as sc
import schur_factor_case as fc
from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import finalize_b

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [1, 2, 3, 63, 64, 65, 129, 300, 1100]


@pytest.fixture(scope="module")
def kkt():
    return sc.kkt()


@pytest.fixture(scope="module")
def whole(kkt):
    K, n, m = kkt
    w = sc.whole_handle(K, n, m)
    yield w
    finalize_b(w)


@pytest.fixture(scope="module")
def handles(kkt):
    """one analysed Schur-mode handle per order, shared by the cases of this module"""
    K, n, m = kkt
    made = {}

    def get(ns):
        if ns not in made:
            idx = sc.mixed_set(n, m, ns, seed=ns)
            made[ns] = (sc.schur_handle("symmetric", K, idx), idx)
        return made[ns]

    yield get
    for h, _ in made.values():
        finalize_b(h)


DESIGNS = {"antidiagonal": ref.antidiagonal, "definite": ref.definite, "heavy_tail": ref.heavy_tail, "spectrum": ref.spectrum}


@pytest.mark.parametrize("ns", ORDERS)
@pytest.mark.parametrize("design", sorted(DESIGNS))
def test_designed_input(handles, design, ns):
    h, _ = handles(ns)
    r = fc.check_designed(h, DESIGNS[design](ns))
    two = int((r["ipiv"] < 0).sum())
    if design == "antidiagonal":
        assert two == ns - ns % 2
    if design == "definite":
        assert np.array_equal(r["ipiv"], np.arange(1, ns + 1))
    if design == "heavy_tail" and ns >= 63:      # interchanges that reach beyond the panel of their column
        assert any(abs(abs(int(p)) - 1 - k) >= 32 for k, p in enumerate(r["ipiv"]))


@pytest.mark.parametrize("p", [29, 30, 31, 62, 63, 64])
def test_pair_at_a_panel_end(handles, p):
    """a 2 x 2 pivot on the columns p, p + 1 (0-based) around the ends of the first two panels: 30-31 fills a panel to its full
    width, 31-32 has to open the next one, as 61-62 / 62-63 do one panel later; 63-64 and 64-65 straddle the 64-wide block of the
    substitutions"""
    h, _ = handles(129)
    r = fc.check_designed(h, ref.pair_at(129, p))
    assert list(np.flatnonzero(r["ipiv"] < 0)) == [p, p + 1]


@pytest.mark.parametrize("ns", [3, 65, 300])
def test_singular_input(handles, ns):
    h, _ = handles(ns)
    fc.check_designed(h, ref.singular(ns), zero=1)
    assert h.schur_inertia[2:] == (1, 0)


@pytest.mark.parametrize("ns", ORDERS)
def test_assembled_schur_complement(kkt, whole, handles, ns):
    K, n, m = kkt
    h, idx = handles(ns)
    n1, m1 = fc.split(idx, n, m)
    assert h.ls_factor_schur(K, n1, m1) == 1
    S = h.schur()
    assert h.schur_factor() == 1
    assert np.array_equal(h.schur(), S)      # the assembled S is intact
    A11 = sc.dense_parts(K, idx)[0]
    p1, q1 = sc.inertia_of(np.linalg.eigvalsh(A11))
    ps, qs = sc.inertia_of(np.linalg.eigvalsh(S))
    assert h.schur_inertia == (ps, qs, 0, 0)
    assert h.total_inertia == (p1 + ps, q1 + qs, 0, 0) == whole.inertia
    fc.check_reconstruction(h, S)
    fc.check_dense_solve(h, S)
    fc.check_fused(h, K, whole=whole)


@pytest.mark.parametrize("ns", ORDERS)
def test_zeroed_diagonal_needs_pivoting(kkt, ns):
    K, n, m = kkt
    fc.check_needs_pivoting(K, n, m, ns, seed=ns)


def test_device_entry_points(kkt, handles):
    K, n, m = kkt
    ns, nrhs, dim = 65, 3, n + m
    h, idx = handles(ns)
    assert h.ls_factor_schur(K, *fc.split(idx, n, m)) == 1
    assert h.schur_factor() == 1
    LD, ipiv = h.schur_get_factor()
    assert h.schur_factor_dev() == 1
    LD2, ipiv2 = h.schur_get_factor()
    assert np.array_equal(LD, LD2) and np.array_equal(ipiv, ipiv2)
    rng = np.random.default_rng(6)
    B, R2 = rng.normal(size=(nrhs, dim)), rng.normal(size=(nrhs, ns))
    d_B, d_X = h.dev_upload(B), h.dev_alloc(8 * dim * nrhs)
    h.schur_solve_dev(d_B, d_X, nrhs)
    assert np.array_equal(h.dev_download(d_X, (nrhs, dim)), h.schur_solve(B))
    d_R2 = h.dev_upload(R2)
    h.schur_dense_solve_dev(d_R2, d_R2, nrhs)      # in place
    assert np.array_equal(h.dev_download(d_R2, (nrhs, ns)), h.schur_dense_solve(R2))
    # a caller's S in device memory with ld > ns
    S = ref.spectrum(ns, seed=3)
    ld = ns + 5
    Sp = np.zeros((ns, ld))
    Sp[:, :ns] = S.T
    d_S = h.dev_upload(Sp)
    assert h.schur_factor_dev(d_S, ld) == 1
    LDd, ipivd = h.schur_get_factor()
    assert h.schur_factor(S) == 1
    LDh, ipivh = h.schur_get_factor()
    assert np.array_equal(LDd, LDh) and np.array_equal(ipivd, ipivh)
    for p in (d_B, d_X, d_R2, d_S):
        h.dev_free(p)


def test_refusals_leave_the_handle_usable(kkt, whole):
    K, n, m = kkt
    ns = 20
    idx = sc.mixed_set(n, m, ns, seed=11)
    n1, m1 = fc.split(idx, n, m)
    x, x2, S = np.zeros(n + m), np.zeros(ns), ref.spectrum(ns)
    inv = L.OKKT_ERR_INVALID
    # without a set
    assert whole._lib.okkt_schur_factor(whole._h, None, ns, None, None) == inv
    assert whole._lib.okkt_schur_solve(whole._h, L.p_f64(x), L.p_f64(x), 1) == inv
    assert np.array_equal(whole.ls_solve(x), x)
    h = sc.schur_handle("symmetric", K, idx)
    ipiv = np.zeros(ns, dtype=np.int32)
    get = lambda: h._lib.okkt_schur_get_factor(h._h, L.p_f64(np.zeros(ns * ns)), ns, ipiv.ctypes.data_as(L.C.POINTER(L.C.c_int32)))
    # before any factor
    assert h._lib.okkt_schur_factor(h._h, None, ns, None, None) == inv
    assert h._lib.okkt_schur_dense_solve(h._h, L.p_f64(x2), L.p_f64(x2), 1) == inv
    assert h._lib.okkt_schur_solve(h._h, L.p_f64(x), L.p_f64(x), 1) == inv
    assert get() == inv
    assert h._lib.okkt_schur_factor(h._h, L.p_f64(L.f64(S)), ns - 1, None, None) == inv      # ld < ns
    # a caller's S needs no okkt_factor_schur; the whole-system solve does
    assert h.schur_factor(S) == 1
    fc.check_dense_solve(h, S, nrhs_list=(1,))
    assert h._lib.okkt_schur_solve(h._h, L.p_f64(x), L.p_f64(x), 1) == inv
    assert h.ls_factor_schur(K, n1, m1) == 1
    fc.check_dense_solve(h, S, nrhs_list=(1,))      # the factor of a caller's S stays valid
    # the handle's own S: stale after the next okkt_factor_schur
    assert h.schur_factor() == 1
    fc.check_fused(h, K, whole=whole, nrhs_list=(1,))
    assert h.ls_factor_schur(K, n1, m1) == 1
    assert h._lib.okkt_schur_dense_solve(h._h, L.p_f64(x2), L.p_f64(x2), 1) == inv
    assert h._lib.okkt_schur_solve(h._h, L.p_f64(x), L.p_f64(x), 1) == inv
    assert get() == inv
    assert h.schur_factor() == 1
    fc.check_fused(h, K, whole=whole, nrhs_list=(1,))
    # what Schur mode refused before stays refused
    assert h._lib.okkt_solve(h._h, L.p_f64(x), L.p_f64(x), 1) == inv
    finalize_b(h)


def test_routes_in_process():
    fc.routes()


@pytest.mark.parametrize("env", [{"OKKT_DATAFLOW": "0"}, {"OKKT_FLOW": "0"}], ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_routes_switched(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schur_factor_case.py")], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SCHUR_FACTOR_OK" in r.stdout, (env, r.stdout[-400:], r.stderr[-1500:])
