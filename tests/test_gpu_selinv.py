"""Selected inversion on the device (okkt_selinv and its exports): Z = F^-1 on the pattern of the factor against
a dense inverse, at scale against refined solves, the log-determinant, the route switches, reproducibility, the state rules and the
refusals.  The tolerance is justified in selinv_case.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import front_trees as ft  # noqa: E402
import selinv_case as slc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(ft.DESIGNS))
def test_designs_against_dense_inverse(name):
    d, h = slc.design_handle(name)
    slc.check_against_dense(h, d.A, perm=d.perm)
    assert np.array_equal(h.perm(), d.perm)
    finalize_b(h)


def _kkt(convex, seed=5):
    prob = synth.make_problem(1500, 1000, seed=seed, well_scaled=True, convex=convex)
    return prob, synth.augmented_matrix(prob, delta=1e-8)


@pytest.mark.parametrize("convex", [True, False])
def test_indefinite_kkt(convex):
    prob, K = _kkt(convex)
    n, m = prob["n"], prob["m"]
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    assert h.ls_factor_b(K, n, m) in (0, 1)
    slc.check_against_dense(h, K)
    zv = slc.check_on_pattern(h, K)
    # the J' block of K is upper-triangle input: each entry takes its mirror's value, which lies on the pattern (the J block)
    assert np.isfinite(zv).all()
    finalize_b(h)


def test_definite_schur_matrix():
    prob = synth.make_problem(2500, 1500, seed=3, well_scaled=True)
    Q = synth.schur_matrix(prob, delta=1e-6)
    h = linear_solver_HIP("definite")
    initialize_b(h)
    assert h.ls_factor_b(Q, prob["n"], 0) == 1
    _, d = slc.check_against_dense(h, Q)
    assert np.all(d > 0)
    slc.check_on_pattern(h, Q)
    finalize_b(h)


@pytest.mark.parametrize("config", ["S-C3", "S-C5"])
def test_at_scale_against_refined_solves(config):
    prob = synth.make_config(config, seed=0, well_scaled=True)
    n, m = prob["n"], prob["m"]
    K = synth.augmented_matrix(prob, delta=1e-8)
    dim = n + m
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    assert h.ls_factor_b(K, n, m) in (0, 1)
    info = h.selinv()
    assert info["status"] == 0, info
    Z = h.inverse_csc()
    p = h.perm()
    # 32 columns: the root front's last columns, the first (leaf) columns, and columns in between
    picks = np.unique(np.concatenate([np.arange(dim - 8, dim), np.arange(8), np.linspace(8, dim - 9, 16).astype(np.int64)]))
    Zl = Z.tocsc()
    for jp in picks:
        j = p[jp]
        e = np.zeros(dim)
        e[j] = 1.0
        x, _ = h.ls_solve_refine(K, e, max_steps=5)
        ferr, _ = h.forward_error(K, e, x)
        bound = 10.0 * ferr * np.max(np.abs(x)) + 1e-15
        col = Zl.getcol(jp)
        rows = col.indices
        zc = col.toarray().ravel()[rows]
        err = np.max(np.abs(zc - x[p[rows]]))
        assert err <= bound, (config, jp, err, bound, ferr)
    finalize_b(h)


def test_logdet_small_and_directional_derivative():
    for name in ["small-classes-f32-33-64-65-128-129", "deep-chain-6", "fan-in-8"]:
        d, h = slc.design_handle(name)
        ld, sg = h.logdet()
        s_ref, ld_ref = np.linalg.slogdet(slc.dense(d.A))
        assert sg == int(s_ref)
        assert abs(ld - ld_ref) <= 1e-10 * max(1.0, abs(ld_ref)), (name, ld, ld_ref)
        finalize_b(h)
    prob = synth.make_config("S-C3", seed=0, well_scaled=True)
    n, m = prob["n"], prob["m"]
    K = sp.csc_matrix(synth.augmented_matrix(prob, delta=1e-8, with_upper=False))
    K.sort_indices()
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    assert h.ls_factor_b(K, n, m) in (0, 1)
    h.selinv()
    zv = h.inverse_on_pattern()
    rng = np.random.default_rng(1)
    E = rng.normal(size=K.nnz)
    rows = K.indices
    cols = np.repeat(np.arange(K.shape[0]), np.diff(K.indptr))
    w = np.where(rows == cols, 1.0, 2.0)          # off-diagonal entries stand for two entries of the symmetric matrix
    lin = float(np.sum(w * zv * E))
    t = 1e-5 / np.max(np.abs(E))
    lds = []
    for sgn in (1.0, -1.0):
        assert h.ls_factor_b((K.shape[0], K.indptr, K.indices, K.data + sgn * t * E, 0), n, m) in (0, 1)
        lds.append(h.logdet()[0])
    fd = (lds[0] - lds[1]) / (2 * t)
    # central difference: O(t^2) truncation; the rounding of the two log-determinants (sums of n logs) over 2t dominates
    assert abs(fd - lin) <= 1e-3 * max(1.0, abs(lin)), (fd, lin)
    finalize_b(h)


@pytest.mark.parametrize("env", [{"OKKT_DATAFLOW": "0"}, {"OKKT_FLOW": "0"}, {"OKKT_RELEASE_CB": "0"}])
def test_routes_switched(env):
    def run(extra):
        e = dict(os.environ)
        e.update(extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "selinv_case.py")], cwd=ROOT, env=e, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and "SELINV_OK" in r.stdout, (extra, r.stdout[-400:], r.stderr[-1500:])
        return r.stdout.split("SELINV_OK", 1)[1].split()
    base = run({})
    other = run(env)
    assert other == base, env


def test_reproducible_and_state():
    prob, K = _kkt(True, seed=11)
    n, m = prob["n"], prob["m"]
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    assert h.ls_factor_b(K, n, m) == 1
    b = np.random.default_rng(0).normal(size=n + m)
    x0 = h.ls_solve(b)
    i1 = h.selinv()
    Z1, d1 = h.inverse_csc(), h.inverse_diag()
    h.selinv()
    Z2, d2 = h.inverse_csc(), h.inverse_diag()
    assert np.array_equal(Z1.data, Z2.data) and np.array_equal(d1, d2)
    # solves are bitwise unchanged by an interleaved selected inversion
    assert np.array_equal(h.ls_solve(b), x0)
    # new values: the old Z is stale, every export refuses it
    K2 = K.copy()
    K2.data = K.data * 1.5
    assert h.ls_factor_b(K2, n, m) == 1
    for call in (h.inverse_diag, h.inverse_csc, h.inverse_on_pattern):
        with pytest.raises(OkktError, match="no selected inverse"):
            call()
    h.selinv()
    assert not np.array_equal(h.inverse_diag(), d1)
    # back to the first values: the same bits again
    assert h.ls_factor_b(K, n, m) == 1
    h.selinv()
    assert np.array_equal(h.inverse_csc().data, Z1.data) and np.array_equal(h.inverse_diag(), d1)
    # device forms equal the host forms
    d_out = h.dev_alloc(8 * (n + m))
    h.inverse_diag_dev(d_out)
    assert np.array_equal(h.dev_download(d_out, (n + m,)), d1)
    h.dev_free(d_out)
    zv = h.inverse_on_pattern()
    d_z = h.dev_alloc(8 * len(zv))
    h.inverse_on_pattern_dev(d_z)
    assert np.array_equal(h.dev_download(d_z, (len(zv),)), zv, equal_nan=True)
    h.dev_free(d_z)
    # a new analysis releases the arena; the next selinv sizes it for the new plan
    prob2 = synth.make_problem(600, 400, seed=2, well_scaled=True)
    K3 = synth.augmented_matrix(prob2, delta=1e-8)
    assert h.ls_factor_b(K3, 600, 400) in (0, 1)
    with pytest.raises(OkktError, match="no selected inverse"):
        h.inverse_diag()
    i3 = h.selinv()
    assert 0 < i3["arena_bytes"] < i1["arena_bytes"]
    slc.check_against_dense(h, K3)
    finalize_b(h)


def test_refusals():
    prob = synth.make_config("S-small", seed=2, convex=False, neg_shift=50.0, well_scaled=True)
    n, m = prob["n"], prob["m"]
    K0 = synth.augmented_matrix(prob, delta=0.0)
    good = synth.augmented_matrix(synth.make_config("S-small", seed=2, well_scaled=True), delta=1e-8)
    # before a factorisation
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K0)
    with pytest.raises(OkktError, match="complete factorisation"):
        h.selinv()
    with pytest.raises(OkktError, match="complete factorisation"):
        h.logdet()
    assert h.ls_factor_b(good, n, m) in (0, 1)
    h.selinv()
    assert np.isfinite(h.inverse_diag()).all()
    finalize_b(h)
    # an early exit that stopped short, then a complete factorisation on the same handle
    early = linear_solver_HIP("symmetric", early_exit=1)
    initialize_b(early)
    assert early.ls_factor_b(K0, n, m) == 0 and sum(early.inertia) < n + m
    with pytest.raises(OkktError, match="early exit"):
        early.selinv()
    early._lib.okkt_set_early_exit(early._h, 0)
    assert early.ls_factor_b(good, n, m) in (0, 1)
    early.selinv()
    finalize_b(early)
    # Schur mode, then the set cleared
    s = linear_solver_HIP("symmetric")
    initialize_b(s)
    s.set_schur(np.array([0, n]))
    s.analyze(good)
    with pytest.raises(OkktError, match="Schur mode"):
        s.selinv()
    s.set_schur(np.array([], dtype=np.int64))
    assert s.ls_factor_b(good, n, m) in (0, 1)
    s.selinv()
    finalize_b(s)
    # a partitioned handle, then one part again
    p = linear_solver_HIP("symmetric")
    initialize_b(p)
    p.analyze(good)
    assert p._lib.okkt_dist_set_partition(p._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        p.selinv()
    assert p._lib.okkt_dist_set_partition(p._h, 1, 0) == L.OKKT_OK
    assert p.ls_factor_b(good, n, m) in (0, 1)
    p.selinv()
    finalize_b(p)
    # a factor whose flag is 0 is accepted (inertia wrong, pivots finite)
    z = linear_solver_HIP("symmetric")
    initialize_b(z)
    assert z.ls_factor_b(K0, n, m) == 0
    info = z.selinv()
    assert info["status"] in (0, 1) and (info["status"] == 1) == (info["nonfinite"] > 0)
    finalize_b(z)


@pytest.mark.parametrize("kind", ["symmetric", "schur"])
def test_through_kkt_layer(kind):
    import ctypes as C
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    rng = np.random.default_rng(0)
    it = KS.Class_iterate(x=rng.normal(size=prob["n"]), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                          grad=rng.normal(size=prob["n"]), cons=prob["s"] + 0.1 * rng.normal(size=prob["m"]), a_norm_penalty_par=1e-4)
    delta = 1e-8
    k = KS.HIP_KKT_solver(kind, KS.Class_parameters())
    k.initialize_b(it)
    k.form_system_b(it)
    k.factor_b(delta)
    dim, nnz = C.c_int64(), C.c_int64()
    k._check(k._lib.okkt_kkt_get_matrix(k._k, C.byref(dim), C.byref(nnz), None, None, None), "okkt_kkt_get_matrix")
    cp = np.zeros(dim.value + 1, dtype=np.int64)
    rv = np.zeros(max(nnz.value, 1), dtype=np.int64)
    nz = np.zeros(max(nnz.value, 1))
    k._check(k._lib.okkt_kkt_get_matrix(k._k, C.byref(dim), C.byref(nnz), L.p_i64(cp), L.p_i64(rv), L.p_f64(nz)), "okkt_kkt_get_matrix")
    A = slc.dense(sp.csc_matrix((nz[:nnz.value], rv[:nnz.value], cp), shape=(dim.value, dim.value)))
    A[np.arange(it.dim()), np.arange(it.dim())] += delta      # the shift the factorisation adds on the first n pivots
    ls = linear_solver_HIP.of_kkt(k)
    ls.selinv()
    d = ls.inverse_diag()
    ref = np.diag(np.linalg.inv(A))
    assert np.max(np.abs(d - ref)) <= slc.tolerance(A, ls) * np.max(np.abs(ref)), kind
    if kind == "schur":
        assert np.all(d > 0)
    ls._finalize()      # a borrowed handle: the KKT solver still owns it
    k.finalize_b()
