"""GPU tests of the Schur route made whole: the dense inverse S^-1 from the Bunch-Kaufman factor, selected
inversion, the log-determinant, the condition estimate, the forward error bound and GMRES-IR through the route, the state rules and
the dispatchers beside ls_solve_robust.  References: numpy.linalg.inv / slogdet of the dense matrix, the restatements of the plain
route's tests (condest_ref, gmres_ref, pivots_ref), and the plain route itself where no pivoting is needed.  The tolerance rules are
those of schur_route_case.py and selinv_case.py.  Measured values are printed as SCHUR_ROUTE {json} lines."""
import json

import numpy as np
import pytest
import scipy.sparse as sp

import dense_ldlt_ref as ref
import front_trees as ft
import gmres_ref as gr
import pivots_ref as pr
import schur_case as sc
import schur_factor_case as fc
import schur_route_case as rc
import schur_trees as sct
import selinv_case as slc
from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def record(**kw):
    print("SCHUR_ROUTE " + json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))


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
    """one analysed Schur-mode handle per set size, shared by the dense cases: they factor a caller's S"""
    K, n, m = kkt
    made = {}

    def get(ns):
        if ns not in made:
            made[ns] = sc.schur_handle("symmetric", K, np.random.default_rng(ns).permutation(n + m)[:ns])
        return made[ns]

    yield get
    for h in made.values():
        finalize_b(h)


# ---- 1. the dense inverse of a caller's S --------------------------------------------------------------------------------------------

CASES = rc.dense_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dense_inverse(handles, case):
    name, ns, make = case
    S = make()
    h = handles(ns)
    assert h.schur_factor(S) == 1
    Z = h.schur_inverse()
    assert h.schur_inverse_nonfinite == 0
    assert np.array_equal(Z, Z.T)      # both triangles written, the same bits
    LD, ipiv = h.schur_get_factor()
    g = rc.dense_growth(LD, ipiv, S)
    tol = rc.dense_tolerance(S, g)
    Sinv = np.linalg.inv(rc.full(S))
    err = float(np.max(np.abs(Z - Sinv)) / np.max(np.abs(Sinv)))
    record(test="dense_inverse", name=name, err=err, tol=tol, growth=g, two_by_two=int((ipiv < 0).sum()))
    assert err <= tol, (name, err, tol)
    assert np.array_equal(h.schur_inverse(), Z)      # deterministic


def test_dense_inverse_on_the_device_with_a_wider_ld(handles):
    ns, ld = 65, 70
    h = handles(ns)
    assert h.schur_factor(ref.spectrum(ns, seed=3)) == 1
    Z = h.schur_inverse()
    d_Z = h.dev_upload(np.full((ns, ld), -7.0))
    h.schur_inverse_dev(d_Z, ld)
    out = h.dev_download(d_Z, (ns, ld))
    assert np.array_equal(out[:, :ns].T, Z) and np.all(out[:, ns:] == -7.0)
    with pytest.raises(OkktError, match="ld < ns"):
        h.schur_inverse_dev(d_Z, ns - 1)
    h.dev_free(d_Z)


@pytest.mark.parametrize("ns", [3, 65])
def test_dense_inverse_of_a_singular_input(handles, ns):
    h = handles(ns)
    assert h.schur_factor(ref.singular(ns)) == 0
    Z = h.schur_inverse()      # the divisions give what they give: no error
    bad = int(np.count_nonzero(~np.isfinite(Z)))
    assert bad > 0 and h.schur_inverse_nonfinite == bad
    assert h.schur_factor(ref.definite(ns)) == 1      # the handle goes on
    h.schur_inverse()
    assert h.schur_inverse_nonfinite == 0


# ---- 2. selected inversion through the route on designed trees --------------------------------------------------------------------------

TREES = ["set-65-small-only", "set-257", "task-chains-under-big", "fan-in-8", "lone-roots-then-set", "forest-3-roots", "set-2049-thin"]


def pattern_mask(Z):
    return sp.csc_matrix((np.ones(len(Z.data), dtype=bool), Z.indices, Z.indptr), shape=Z.shape).toarray()


@pytest.mark.parametrize("name", TREES)
def test_selinv_on_designed_trees(name):
    d = sct.build(name, values="plain")
    ns = sct.set_size(d)
    n1 = d.n - ns
    n1pos = sct.interior_positive(d)
    h = sct.schur_handle(d)
    assert h.ls_factor_schur(d.A, n1pos, n1 - n1pos) == 1
    assert h.schur_factor() == 1
    info = h.schur_selinv()
    assert info["status"] == 0 and info["nonfinite"] == 0, info
    D = slc.dense(d.A)
    Ainv = np.linalg.inv(D)
    scale = float(np.max(np.abs(Ainv)))
    p = h.perm()
    assert np.array_equal(p, d.perm)
    Z = h.inverse_csc()
    Zc = Z.tocoo()
    assert np.all(Zc.row >= Zc.col)
    err = float(np.max(np.abs(Zc.data - Ainv[p[Zc.row], p[Zc.col]])))
    dg = h.inverse_diag()
    err_d = float(np.max(np.abs(dg - np.diag(Ainv))))
    A = sp.csc_matrix(d.A)
    A.sort_indices()
    zv = h.inverse_on_pattern()
    rows, cols = A.indices, np.repeat(np.arange(d.n), np.diff(A.indptr))
    ok = np.isfinite(zv)
    assert len(zv) == A.nnz and ok[rows >= cols].all()
    err_p = float(np.max(np.abs(zv[ok] - Ainv[rows[ok], cols[ok]])))
    record(test="selinv_tree", name=name, ns=ns, n=d.n, err=err / scale, err_diag=err_d / scale, err_pattern=err_p / scale,
           seconds_device=info["seconds_device"])
    assert max(err, err_d, err_p) <= slc.Z_TOL * scale, (name, err, err_d, err_p, scale)
    assert np.array_equal(Z.diagonal(), dg[p])
    # the set's block is S^-1, bit for bit: the full lower triangle
    Zs = Z[n1:, n1:].toarray()
    assert np.array_equal(Zs, np.tril(h.schur_inverse()))
    # the same bits twice
    info2 = h.schur_selinv()
    Z2 = h.inverse_csc()
    assert info2["nonfinite"] == 0 and np.array_equal(Z2.data, Z.data) and np.array_equal(Z2.indices, Z.indices)
    # the same design factored whole
    w = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(w)
    w.set_perm(d.perm)
    assert w.ls_factor_b(d.A, d.npos, d.nneg) == 1
    w.selinv()
    Zw = w.inverse_csc()
    both = pattern_mask(Z) & pattern_mask(Zw)
    assert both.sum() >= 0.99 * len(Z.data)
    diff = float(np.max(np.abs((Z.toarray() - Zw.toarray())[both])))
    assert diff <= slc.Z_TOL * scale, (name, diff, scale)
    finalize_b(w)
    finalize_b(h)


# ---- 3. a matrix that needs the pivoting ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [17, 40])
def test_zeroed_diagonal_through_the_route(kkt, ns):
    K, n, m = kkt
    idx = sc.mixed_set(n, m, ns, seed=ns)
    n1, m1 = fc.split(idx, n, m)
    K0 = fc.zeroed_diagonal(K, idx)
    h = sc.schur_handle("symmetric", K0, idx)
    assert h.ls_factor_schur(K0, n1, m1) == 1
    assert h.schur_factor() == 1
    A = synth.symmetrize_lower(K0).toarray()
    Ainv = np.linalg.inv(A)
    lam = np.abs(np.linalg.eigvalsh(A))
    cond2 = float(lam.max() / lam.min())
    p = h.perm()
    g = rc.whole_growth(h, A[np.ix_(p, p)])
    tol = max(1e-8, 100.0 * EPS * g * cond2)
    scale = float(np.max(np.abs(Ainv)))
    info = h.schur_selinv()
    assert info["status"] == 0 and info["nonfinite"] == 0, info
    Zc = h.inverse_csc().tocoo()
    err = float(np.max(np.abs(Zc.data - Ainv[p[Zc.row], p[Zc.col]])) / scale)
    err_d = float(np.max(np.abs(h.inverse_diag() - np.diag(Ainv))) / scale)
    # the log-determinant
    ld, sg = h.schur_logdet()
    sg_ref, ld_ref = np.linalg.slogdet(A)
    # the condition estimate
    norm1 = float(np.abs(A).sum(axis=0).max())
    exact = norm1 * float(np.abs(Ainv).sum(axis=0).max())
    ce = [h.schur_condest(K0) for _ in range(3)]
    # the forward error bound
    b = np.random.default_rng(ns).normal(size=n + m)
    x = h.schur_solve(b)
    xt = pr.long_double_solution(K0, b)
    true_err = pr.fwd_err(x, xt)
    ferr, berr = h.schur_forward_error(K0, b, x)
    x0, ri = h.schur_solve_refine(K0, b, max_steps=0)
    record(test="zeroed_diagonal", ns=ns, cond2=cond2, growth=g, tol=tol, err=err, err_diag=err_d, logdet=ld, logdet_ref=float(ld_ref),
           cond1=ce[0]["cond1"], exact=exact, ferr=float(ferr), true_err=true_err, berr=float(berr), omega=ri["omega"])
    assert max(err, err_d) <= tol, (ns, err, err_d, tol)
    assert sg == int(sg_ref) and abs(ld - ld_ref) <= 1e-10 * max(1.0, abs(ld_ref)), (ld, sg, ld_ref, sg_ref)
    assert abs(ce[0]["norm1"] - norm1) <= 1e-13 * norm1
    assert exact / 3.0 <= ce[0]["cond1"] <= exact * (1 + 1e-10), (ce[0], exact)
    assert ce[0] == ce[1] == ce[2] and ce[0]["status"] == 0
    assert len(h.condest_indices()) > 0
    assert np.array_equal(x0, x)
    assert ferr >= true_err, (ferr, true_err)
    assert berr == ri["omega"], (berr, ri)
    finalize_b(h)


# ---- 4. agreement with the plain route where no pivoting is needed --------------------------------------------------------------------------

def test_condest_agrees_with_the_plain_route(kkt, whole):
    K, n, m = kkt
    idx = np.random.default_rng(20).choice(n + m, 20, replace=False)
    h = sc.schur_handle("symmetric", K, idx)
    assert h.ls_factor_schur(K, *fc.split(idx, n, m)) == 1
    assert h.schur_factor() == 1
    a, b = h.schur_condest(K), whole.condest(K)
    record(test="condest_vs_plain", schur=a, plain=b)
    assert a["status"] == 0 and a["norm1"] == b["norm1"]
    assert abs(a["inv_norm1"] - b["inv_norm1"]) <= 1e-8 * b["inv_norm1"], (a, b)
    finalize_b(h)


# ---- 5. GMRES-IR ------------------------------------------------------------------------------------------------------------------------

def test_gmres_through_the_route():
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-4)
    F = synth.augmented_matrix(prob, delta=1e-4 + 10.0)      # the shift at which plain refinement stalls (test_gpu_gmres.py)
    idx = sc.mixed_set(n, m, 20, seed=20)
    h = sc.schur_handle("symmetric", F, idx)
    assert h.ls_factor_schur(F, *fc.split(idx, n, m)) == 1
    assert h.schur_factor() == 1
    B = np.random.default_rng(4).normal(size=(5, n + m))
    resid, solve = gr.LongResidual(ft.full_csr(sp.tril(A))), gr.dense_solver(ft.full_csr(sp.tril(F)))
    refs = [gr.gmres_ir(resid, solve, b)[1] for b in B]
    for nr in (1, 5):
        X, info = h.schur_solve_gmres(A, B[:nr], restart=30, max_iters=200)
        record(test="gmres", nrhs=nr, iterations=info["iterations"], cycles=info["cycles"], solves=info["solves"], omega0=info["omega0"],
               omega=info["omega"], ref_iterations=[r["iterations"] for r in refs[:nr]])
        assert info["status"] == 0 and info["omega"] <= EPS, info
        assert np.all(info["omega_per_rhs"] <= EPS)
        assert abs(info["iterations"] - max(r["iterations"] for r in refs[:nr])) <= 2, (info, refs[:nr])
        X2, info2 = h.schur_solve_gmres(A, B[:nr], restart=30, max_iters=200)
        assert np.array_equal(X, X2) and info2["iterations"] == info["iterations"]
        # max_iters = 0: schur_solve's bits
        X0, info0 = h.schur_solve_gmres(A, B[:nr], max_iters=0)
        assert np.array_equal(X0, h.schur_solve(B[:nr])) and info0["iterations"] == 0 and info0["status"] == 1
        # rhs may alias sol
        buf = B[:nr].copy()
        vals = h._values(A)
        h._check(h._lib.okkt_schur_solve_gmres(h._h, L.p_f64(vals), L.p_f64(buf), L.p_f64(buf), nr, 30, 200, 0.0, None, None), "okkt_schur_solve_gmres")
        assert np.array_equal(buf, X)
    # the device entry point
    d_A, d_B, d_X = h.dev_upload(h._values(A)), h.dev_upload(B), h.dev_alloc(8 * B.size)
    h.schur_solve_gmres_dev(d_A, d_B, d_X, nrhs=5)
    assert np.array_equal(h.dev_download(d_X, B.shape), X)
    for q in (d_A, d_B, d_X):
        h.dev_free(q)
    finalize_b(h)


# ---- 6. state rules -----------------------------------------------------------------------------------------------------------------------

def new_calls(h, K, b, x):
    """every new call that needs the whole route, by name"""
    return {"schur_selinv": h.schur_selinv, "schur_logdet": h.schur_logdet, "schur_condest": lambda: h.schur_condest(K),
            "schur_forward_error": lambda: h.schur_forward_error(K, b, x), "schur_solve_gmres": lambda: h.schur_solve_gmres(K, b)}


def test_state_rules(kkt, whole):
    K, n, m = kkt
    ns = 20
    idx = sc.mixed_set(n, m, ns, seed=11)
    n1, m1 = fc.split(idx, n, m)
    b = np.random.default_rng(1).normal(size=n + m)
    x = np.zeros(n + m)
    # a handle not in Schur mode
    for name, call in list(new_calls(whole, K, b, x).items()) + [("schur_inverse", whole.schur_inverse)]:
        with pytest.raises(OkktError, match="not in Schur mode"):
            call()
    assert np.array_equal(whole.ls_solve(x), x)
    h = sc.schur_handle("symmetric", K, idx)
    assert h.ls_factor_schur(K, n1, m1) == 1
    # before schur_factor
    for name, call in list(new_calls(h, K, b, x).items()) + [("schur_inverse", h.schur_inverse)]:
        with pytest.raises(OkktError, match="no okkt_schur_factor has succeeded"):
            call()
    for export in (h.inverse_diag, h.inverse_csc, h.inverse_on_pattern):
        with pytest.raises(OkktError, match="no selected inverse"):
            export()
    # after schur_factor(S_caller): everything but schur_inverse is refused
    S = ref.spectrum(ns)
    assert h.schur_factor(S) == 1
    Sinv = np.linalg.inv(S)
    assert np.max(np.abs(h.schur_inverse() - Sinv)) <= 1e-8 * np.max(np.abs(Sinv))
    for name, call in new_calls(h, K, b, x).items():
        with pytest.raises(OkktError, match="caller's S"):
            call()
    # the handle's own S: everything works
    assert h.schur_factor() == 1
    xs = h.schur_solve(b)
    for export in (h.inverse_diag, h.inverse_csc, h.inverse_on_pattern):
        with pytest.raises(OkktError, match="no selected inverse"):
            export()
    h.schur_selinv()
    d0 = h.inverse_diag()
    # the plain calls keep refusing on the same handle
    for call in (h.selinv, lambda: h.condest(K), lambda: h.ls_solve_gmres(K, b), h.logdet):
        with pytest.raises(OkktError, match="Schur mode"):
            call()
    assert np.array_equal(h.inverse_diag(), d0)      # a refusal does not cost the selected inverse
    # a new okkt_schur_factor makes the selected inverse stale
    assert h.schur_factor() == 1
    with pytest.raises(OkktError, match="no selected inverse"):
        h.inverse_diag()
    h.schur_selinv()
    assert np.array_equal(h.inverse_diag(), d0)
    # a new ls_factor_schur: the dense factor and the selected inverse are stale
    assert h.ls_factor_schur(K, n1, m1) == 1
    for name, call in list(new_calls(h, K, b, x).items()) + [("schur_inverse", h.schur_inverse)]:
        with pytest.raises(OkktError, match="okkt_schur_factor again"):
            call()
    with pytest.raises(OkktError, match="no selected inverse"):
        h.inverse_csc()
    # after every refusal the handle still solves
    assert h.schur_factor() == 1
    assert np.array_equal(h.schur_solve(b), xs)
    finalize_b(h)


# ---- 7. the dispatchers ------------------------------------------------------------------------------------------------------------------

def check_dispatch(h, K, b, mode):
    direct = {"schur": (h.schur_condest, h.schur_forward_error, h.schur_selinv, h.schur_logdet, h.schur_solve_gmres),
              "plain": (h.condest, h.forward_error, h.selinv, h.logdet, h.ls_solve_gmres)}[mode]
    x, _ = h.ls_solve_robust(K, b)
    assert h.condest_robust(K) == direct[0](K)
    assert h.forward_error_robust(K, b, x) == direct[1](K, b, x)
    ia = h.selinv_robust()
    da = h.inverse_diag()
    ib = direct[2]()
    assert np.array_equal(da, h.inverse_diag()) and ia["nonfinite"] == ib["nonfinite"] == 0
    assert h.logdet_robust() == direct[3]()
    xa, fa = h.ls_solve_gmres_robust(K, b)
    xb, fb = direct[4](K, b)
    assert np.array_equal(xa, xb) and fa["iterations"] == fb["iterations"] and fa["omega"] == fb["omega"]
    return da


def test_dispatchers(kkt):
    # ends in Schur mode
    Ks, n, m, tiny, partners = pr.designed_kkt()
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    flag, info = h.ls_factor_robust(Ks, n, m)
    assert flag == 1 and info["mode"] == "schur"
    b = np.random.default_rng(2).normal(size=n + m)
    check_dispatch(h, Ks, b, "schur")
    finalize_b(h)
    # ends in the ordinary mode
    K, n, m = kkt
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    flag, info = h.ls_factor_robust(K, n, m)
    assert flag == 1 and info["mode"] == "plain"
    check_dispatch(h, K, np.random.default_rng(3).normal(size=n + m), "plain")
    finalize_b(h)
