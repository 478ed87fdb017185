"""GPU tests of the threshold pivot report, of refinement through the Schur route and of the robust driver.

The multipliers are compared with the column maxima of |L| from okkt_get_factor_csc for EXACT equality: both read the same stored bits
and a maximum does not round.  The tie rule, the empty last column and the non-finite rule are pinned by writing one value into the
input where the factor's value is known exactly.  The robust route runs on the designed KKT system of pivots_ref.designed_kkt, whose
restatement (test_pivots_host.py) fixes what the device has to report.  Measured values are printed as PIVOTS {json} lines."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, csc_arrays, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import pivots_ref as pr  # noqa: E402
import schur_case as sc  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52

DESIGNS = ["small-classes-f32-33-64-65-128-129", "task-chains-under-big", "thin-tall-k1-2-127-128-c2100", "mixed-level-scatter",
           "edge-k256-c0", "edge-k1025-c1", "forest-3-roots"]


def record(**kw):
    print("PIVOTS " + json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))


def design_handle(d):
    h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(h)
    h.set_perm(d.perm)
    return h


def check_against_factor(h, ncols=None, us=(1.0, 0.1, 1e-8)):
    """multipliers(), the counts for every u and the order of rejected_pivots() against the column maxima of the handle's own
    factor_csc(); returns (g, partner)"""
    gr, pref = pr.column_maxima(h.factor_csc(), h.perm(), ncols)
    for u in us:
        rep = h.pivot_report(u)
        g, p = h.multipliers()
        assert np.array_equal(g, gr) and np.array_equal(p, pref)
        ref, rej = pr.report(gr, u)
        assert rep["u"] == u
        assert (rep["rejected"], rep["nonfinite_cols"], rep["max_multiplier"], rep["max_col"]) == \
               (ref["rejected"], ref["nonfinite_cols"], ref["max_multiplier"], ref["max_col"]), (u, rep, ref)
        idx, par = h.rejected_pivots()
        assert np.array_equal(idx, rej) and np.array_equal(par, pref[rej])
    return gr, pref


@pytest.mark.parametrize("values", ["plain", "ipm"])
@pytest.mark.parametrize("name", DESIGNS)
def test_multipliers_equal_the_column_maxima_of_L(name, values):
    d = ft.build(ft.DESIGNS[name][0], values=values)
    h = design_handle(d)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) in (0, 1)
    b = ft.rhs(d.n, 1)[0]
    x_before = h.ls_solve(b)
    g, p = check_against_factor(h)
    # two reports are identical bit for bit (the second one scans again: the factor in between makes the first stale)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) in (0, 1)
    rep = h.pivot_report(1e-8)
    assert rep["seconds_device"] > 0
    g2, p2 = h.multipliers()
    assert g.tobytes() == g2.tobytes() and p.tobytes() == p2.tobytes()
    # no existing call changes
    assert h.ls_solve(b).tobytes() == x_before.tobytes()
    # a column with no row below the diagonal: the last column of every root
    for nd in d.nodes:
        if nd["parent"] is None:
            c = d.perm[nd["col0"] + nd["k"] - 1]
            assert g[c] == 0.0 and p[c] == -1
    record(case=name, values=values, max_multiplier=float(g.max()), rejected_1e8=int(rep["rejected"]), seconds_device=rep["seconds_device"])
    finalize_b(h)


def dense_pow2(n, seed=0):
    """A dense symmetric matrix of order n at natural ordering (one front) whose first column gives multipliers that are known
    exactly: A[0, 0] = 1, so L[:, 0] = A[:, 0]; |A[i, 0]| <= 1/2, a diagonal that dominates."""
    rng = np.random.default_rng(seed)
    A = np.tril(rng.choice([-0.5, 0.25, -0.125], size=(n, n)))
    A[np.arange(n), np.arange(n)] = 4.0 * n
    A[0, 0] = 1.0
    return A


@pytest.mark.parametrize("n", [6, 300])
def test_pinned_rules_in_one_front(n):
    """One dense front at natural ordering (n = 6: a wave of the small-front kernel, n = 300: a workgroup of the big-front kernel).
    L[:, 0] = A[:, 0] exactly, so one written value pins each rule; the other columns are checked against factor_csc."""
    h = linear_solver_HIP("symmetric", ordering=1, **ft.NO_RELAX)
    initialize_b(h)
    lo, hi = 2, n - 2
    # the tie rule: +-1 at two rows of column 0, everything else in it at most 1/2: the lower row wins
    A = dense_pow2(n)
    A[lo, 0], A[hi, 0] = -1.0, 1.0
    assert h.ls_factor_b(sp.csc_matrix(A), n, 0) in (0, 1)
    assert np.array_equal(h.perm(), np.arange(n))
    g, p = check_against_factor(h)
    assert g[0] == 1.0 and p[0] == lo
    # the empty last column
    assert g[n - 1] == 0.0 and p[n - 1] == -1
    # a non-finite entry: the first such row, whatever stands below it
    for bad, worse in ((np.nan, np.inf), (np.inf, np.nan)):
        A = dense_pow2(n)
        A[lo + 1, 0], A[hi, 0] = bad, worse
        assert h.ls_factor_b(sp.csc_matrix(A), n, 0) == 0
        g, p = check_against_factor(h)
        assert g[0] == np.inf and p[0] == lo + 1
        rep = h.pivot_report(1.0)
        assert rep["max_multiplier"] == np.inf and rep["max_col"] == 0 and rep["nonfinite_cols"] >= 1
        assert rep["rejected"] >= rep["nonfinite_cols"]
    finalize_b(h)


def test_pinned_rules_across_the_chunks_of_a_tall_column():
    """thin-tall: the k = 1 front has one column of 2100 rows below the diagonal, scanned as two chunks (front rows 1 .. 2048 and
    2049 .. 2100).  With its diagonal entry set to 1 its multipliers are its input entries: a tie between the chunks goes to the
    lower row, and an Inf in the second chunk beats every finite value of the first."""
    d = ft.build(ft.DESIGNS["thin-tall-k1-2-127-128-c2100"][0])
    nd = next(x for x in d.nodes if x["k"] == 1)
    rows = d.perm[nd["rows"]]             # original labels of the front's rows; rows[0] is the pivot
    c = rows[0]

    def with_entries(entries):
        A = sp.lil_matrix(d.A)
        A[c, c] = 1.0
        for r, v in entries:
            o = rows[r]
            A[max(o, c), min(o, c)] = v
        A = sp.csc_matrix(A)
        A.sort_indices()
        assert A.nnz == d.A.nnz
        return A

    h = design_handle(d)
    assert h.ls_factor_b(with_entries([(7, -16.0), (2090, 16.0)]), d.npos, d.nneg) in (0, 1)
    g, p = check_against_factor(h, us=(1e-8,))
    assert g[c] == 16.0 and p[c] == rows[7]
    assert h.ls_factor_b(with_entries([(7, 16.0), (2060, np.inf), (2090, np.nan)]), d.npos, d.nneg) == 0
    g, p = check_against_factor(h, us=(1e-8,))
    assert g[c] == np.inf and p[c] == rows[2060]
    finalize_b(h)


def test_schur_mode_interior_and_set():
    """Schur mode, a random set of 40 on the synthetic KKT system.  okkt_get_factor_csc serves Schur mode (its interior columns are the
    panels of L; the last supernode's hold S), so the interior is checked against it for exact equality; the set's variables report 0 / -1."""
    K, n, m = sc.kkt()
    idx = sc.mixed_set(n, m, 40, seed=40)
    h = sc.schur_handle("symmetric", K, idx)
    assert h.ls_factor_schur(K, n - int((idx < n).sum()), m - int((idx >= n).sum())) == 1
    g, p = check_against_factor(h, ncols=n + m - 40)
    assert np.all(g[idx] == 0.0) and np.all(p[idx] == -1)
    inner = np.setdiff1d(np.arange(n + m), idx)
    assert np.count_nonzero(g[inner]) > 0.5 * len(inner)
    assert np.isin(p[inner], idx).any()      # interior columns keep their rows towards the set
    # state: the report needs the interior's factor, not the dense one, and goes stale with the next okkt_factor_schur
    assert h.ls_factor_schur(K, n - int((idx < n).sum()), m - int((idx >= n).sum())) == 1
    with pytest.raises(OkktError, match="no pivot report"):
        h.multipliers()
    finalize_b(h)


def test_scaled_factor_is_reported_as_stored():
    K, n, m = sc.kkt()
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.set_scaling("ruiz")
    assert h.ls_factor_b(K, n, m) == 1
    g, _ = check_against_factor(h, us=(1e-8, 1.0))
    plain = linear_solver_HIP("symmetric")
    initialize_b(plain)
    assert plain.ls_factor_b(K, n, m) == 1
    plain.pivot_report()
    assert not np.array_equal(plain.multipliers()[0], g)     # L~, not L
    with pytest.raises(OkktError, match="scaling"):
        h.ls_factor_robust(K, n, m)
    finalize_b(h)
    finalize_b(plain)


def test_of_kkt_reports_the_kkt_factor():
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    rng = np.random.default_rng(0)
    it = KS.Class_iterate(x=rng.normal(size=prob["n"]), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                          grad=rng.normal(size=prob["n"]), cons=prob["s"] + 0.1 * rng.normal(size=prob["m"]), a_norm_penalty_par=1e-4)
    k = KS.HIP_KKT_solver("symmetric", KS.Class_parameters())
    k.initialize_b(it)
    k.form_system_b(it)
    k.factor_b(1e-8)
    ls = linear_solver_HIP.of_kkt(k)
    g, _ = check_against_factor(ls, us=(1e-8,))
    assert np.isfinite(g).all() and g.max() > 0
    k.factor_b(1e-6)           # the KKT level's next factorisation makes the report stale
    with pytest.raises(OkktError, match="no pivot report"):
        ls.multipliers()
    ls._finalize()
    k.finalize_b()


def test_state_rules_and_refusals():
    K, n, m = sc.kkt(300, 200)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    lib = h._lib
    info = L.OkktPivotInfo()
    g = np.zeros(n + m)
    assert lib.okkt_pivot_report(h._h, 1e-8, C.byref(info)) == L.OKKT_ERR_INVALID          # not analysed
    h.analyze(K)
    assert lib.okkt_pivot_report(h._h, 1e-8, C.byref(info)) == L.OKKT_ERR_INVALID          # before a factorisation
    assert "complete factorisation" in lib.okkt_last_error(h._h).decode()
    assert h.ls_factor_b(K, n, m) == 1
    assert lib.okkt_get_multipliers(h._h, L.p_f64(g), None) == L.OKKT_ERR_INVALID           # before a report
    assert lib.okkt_get_rejected_pivots(h._h, None, None, 0) == L.OKKT_ERR_INVALID
    for u in (1.5, np.inf, -np.inf, np.nan):
        assert lib.okkt_pivot_report(h._h, u, C.byref(info)) == L.OKKT_ERR_INVALID, u
    first = h.pivot_report(0.0)                 # u <= 0: the reference's ma97_u
    assert first["u"] == 1e-8
    g1, p1 = h.multipliers()
    # another u on the unchanged factor recounts without scanning again: the time stays the first scan's
    again = h.pivot_report(1.0)
    assert again["seconds_device"] == first["seconds_device"] and again["rejected"] == int(np.sum(g1 > 1.0))
    assert again["max_multiplier"] == first["max_multiplier"] and again["max_col"] == first["max_col"]
    # the _dev getter
    dg, dp = h.dev_alloc(8 * (n + m)), h.dev_alloc(8 * (n + m))
    h.multipliers_dev(dg, dp)
    assert np.array_equal(h.dev_download(dg, (n + m,)), g1) and np.array_equal(h.dev_download(dp, (n + m,), np.int64), p1)
    h.dev_free(dg)
    h.dev_free(dp)
    # partner_out may be NULL
    assert lib.okkt_get_multipliers(h._h, L.p_f64(g), None) == L.OKKT_OK and np.array_equal(g, g1)
    # the next factorisation makes the report stale, the handle stays usable
    assert h.ls_factor_b(K, n, m) == 1
    assert lib.okkt_get_multipliers(h._h, L.p_f64(g), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_rejected_pivots(h._h, None, None, 0) == L.OKKT_ERR_INVALID
    h.pivot_report()
    assert np.array_equal(h.multipliers()[0], g1)
    # a factorisation whose flag was 0 is accepted (the wrong inertia asked for)
    assert h.ls_factor_b(K, n + 1, m - 1) == 0
    assert h.pivot_report()["max_multiplier"] == first["max_multiplier"]
    # a definite handle
    dfn = linear_solver_HIP("definite")
    initialize_b(dfn)
    P = sp.csc_matrix(sp.tril(K[:n, :n]))
    assert dfn.ls_factor_b(P, n, 0) in (0, 1)
    check_against_factor(dfn, us=(1e-8,))
    finalize_b(dfn)
    # an early exit that stopped short, then a complete factorisation on the same handle
    prob = synth.make_config("S-small", seed=2, convex=False, neg_shift=50.0, well_scaled=True)
    ne, me = prob["n"], prob["m"]
    K0 = synth.augmented_matrix(prob, delta=0.0)
    good = synth.augmented_matrix(synth.make_config("S-small", seed=2, well_scaled=True), delta=1e-8)
    e = linear_solver_HIP("symmetric", early_exit=1)
    initialize_b(e)
    assert e.ls_factor_b(K0, ne, me) == 0 and sum(e.inertia) < ne + me
    with pytest.raises(OkktError, match="early exit"):
        e.pivot_report()
    e._lib.okkt_set_early_exit(e._h, 0)
    assert e.ls_factor_b(good, ne, me) in (0, 1)
    assert e.pivot_report()["nonfinite_cols"] == 0
    finalize_b(e)
    # a partitioned handle, then one part again
    pt = linear_solver_HIP("symmetric")
    initialize_b(pt)
    pt.analyze(K)
    assert pt._lib.okkt_dist_set_partition(pt._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        pt.pivot_report()
    assert pt._lib.okkt_dist_set_partition(pt._h, 1, 0) == L.OKKT_OK
    assert pt.ls_factor_b(K, n, m) == 1
    assert pt.pivot_report()["max_multiplier"] == first["max_multiplier"]
    finalize_b(pt)
    finalize_b(h)


# ---- refinement through the Schur route --------------------------------------------------------------------------------------------

def test_schur_solve_refine():
    """On random sets of the synthetic KKT system: omega falls to <= 2^-52 where schur_solve alone leaves it above; max_steps = 0 is
    schur_solve bit for bit; rhs may alias sol; refused after a factor of a caller's S; the existing refusals stay."""
    K, n, m = sc.kkt()
    dim = n + m
    whole = sc.whole_handle(K, n, m)
    for ns in (17, 300):
        idx = sc.mixed_set(n, m, ns, seed=ns)
        h = sc.schur_handle("symmetric", K, idx)
        n1, m1 = n - int((idx < n).sum()), m - int((idx >= n).sum())
        assert h.ls_factor_schur(K, n1, m1) == 1
        assert h.schur_factor() == 1 and h.total_inertia == (n, m, 0, 0)
        B = ft.rhs(dim, 5, seed=ns)
        X0 = h.schur_solve(B)
        _, om0 = whole.residual(K, B, X0)
        X, info = h.schur_solve_refine(K, B, max_steps=5)
        _, om = whole.residual(K, B, X)
        record(case="schur_solve_refine", ns=ns, omega_plain=om0, omega_refined=om, steps=info["steps"], status=info["status"])
        assert np.all(om0 > EPS) and np.all(om <= EPS) and info["status"] == 0 and 1 <= info["steps"] <= 5
        assert np.array_equal(info["omega_per_rhs"], om) and info["omega0"] == om0.max()
        # max_steps = 0 returns okkt_schur_solve's x
        Xz, iz = h.schur_solve_refine(K, B, max_steps=0)
        assert Xz.tobytes() == X0.tobytes() and iz["steps"] == 0 and iz["status"] == 1
        # device pointers, rhs aliasing sol
        d_nz, d_x = h.dev_upload(csc_arrays(K)[3]), h.dev_upload(B)
        di, dom = h.schur_solve_refine_dev(d_nz, d_x, d_x, nrhs=5, max_steps=5)
        assert h.dev_download(d_x, B.shape).tobytes() == X.tobytes() and di["steps"] == info["steps"] and np.array_equal(dom, om)
        h.dev_free(d_nz)
        h.dev_free(d_x)
        # a factor of a caller's S: A is not this handle's matrix
        S = h.schur()
        assert h.schur_factor(S) == 1
        h.schur_solve(B)                    # the plain solve goes on working
        with pytest.raises(OkktError, match="caller's S"):
            h.schur_solve_refine(K, B)
        assert h.schur_factor() == 1
        assert h.schur_solve_refine(K, B, max_steps=5)[0].tobytes() == X.tobytes()
        # a new okkt_factor_schur makes the dense factor stale
        assert h.ls_factor_schur(K, n1, m1) == 1
        with pytest.raises(OkktError, match="okkt_schur_factor again"):
            h.schur_solve_refine(K, B)
        # the existing refusals in Schur mode stay
        with pytest.raises(OkktError, match="Schur mode"):
            h.ls_solve_refine(K, B)
        with pytest.raises(OkktError, match="Schur mode"):
            h.condest(K)
        finalize_b(h)
    with pytest.raises(OkktError, match="not in Schur mode"):
        whole.schur_solve_refine(K, np.ones(dim))
    finalize_b(whole)


# ---- the robust route --------------------------------------------------------------------------------------------------------------

def robust_handle():
    h = linear_solver_HIP("symmetric", ordering=1)
    initialize_b(h)
    return h


def test_robust_route_on_the_designed_kkt():
    """The device reports the restatement's rounds, sets and counts exactly, ends with flag 1 and the whole inertia, and its refined
    solution has status 0.  The forward error (against the long-double reference solution) is held to the restatement's own on the
    same input with the margin of test_gpu_full_size.py for the same comparison: e_device <= 2 e_restatement + 1e-12."""
    K, n, m, tiny, partners = pr.designed_kkt()
    flag_r, info_r, F = pr.robust_rounds(K, n, m, max_rounds=3)
    b = np.random.default_rng(7).normal(size=n + m)
    x_r, ri_r = pr.solve_refine(F, b, 5)
    xt = pr.long_double_solution(K, b)
    h = robust_handle()
    # the plain static route first: the designed columns are rejected with exact powers of two, and its solve is visibly inaccurate
    assert h.ls_factor_b(K, n, m) == 1
    rep = h.pivot_report(1e-8)
    g, p = h.multipliers()
    idx, par = h.rejected_pivots()
    assert rep["rejected"] == len(tiny) and np.array_equal(idx, tiny) and np.array_equal(par, partners) and np.all(g[tiny] == 2.0 ** 40)
    assert rep["max_multiplier"] == 2.0 ** 40 and rep["max_col"] == tiny[0]
    x0 = h.ls_solve(b)
    _, om0 = h.residual(K, b, x0)
    flag, info = h.ls_factor_robust(K, n, m, u=1e-8, max_rounds=3)
    assert flag == flag_r == 1 and h.total_inertia == (n, m, 0, 0)
    assert info["rounds"] == info_r["rounds"] and info["rejected"] == info_r["rejected"] and info["mode"] == info_r["mode"] == "schur"
    assert np.array_equal(info["set"], info_r["set"])
    assert info["max_multiplier"][0] == info_r["max_multiplier"][0] == 2.0 ** 40
    assert info["max_multiplier"][1] == pytest.approx(info_r["max_multiplier"][1], rel=1e-10)
    x, ri = h.ls_solve_robust(K, b, max_steps=5)
    e_h, e_r = pr.fwd_err(x, xt), pr.fwd_err(x_r, xt)
    record(case="robust", omega0_static=float(om0), omega0=ri["omega0"], omega=ri["omega"], steps=ri["steps"], fwd_err_device=e_h,
           fwd_err_restatement=e_r, fwd_err_static=pr.fwd_err(x0, xt), rounds=info["rounds"], rejected=info["rejected"],
           max_multiplier=info["max_multiplier"])
    assert om0 >= 1e-8
    assert ri["status"] == 0 and ri["omega"] <= EPS and ri_r["status"] == 0
    assert e_h <= 2.0 * e_r + 1e-12, (e_h, e_r)
    # the handle is in Schur mode with the final set; clearing it gives the ordinary handle back
    h.set_schur([])
    assert h.ls_factor_b(K, n, m) == 1
    finalize_b(h)


def test_robust_route_with_nothing_rejected():
    K, n, m, _, _ = pr.designed_kkt(tiny=(), tiny_sigma=())
    b = np.random.default_rng(7).normal(size=n + m)
    h = robust_handle()
    flag, info = h.ls_factor_robust(K, n, m)
    assert flag == 1 and info["mode"] == "plain" and info["rounds"] == 1 and info["rejected"] == [0] and len(info["set"]) == 0
    assert h._ns == 0
    x, ri = h.ls_solve_robust(K, b, max_steps=5)
    plain = robust_handle()
    assert plain.ls_factor_b(K, n, m) == 1
    xp, rp = plain.ls_solve_refine(K, b, max_steps=5)
    assert x.tobytes() == xp.tobytes() and ri["steps"] == rp["steps"] and ri["omega"] == rp["omega"]
    h.ls_solve(b)            # not in Schur mode: the ordinary calls work
    finalize_b(h)
    finalize_b(plain)


def test_robust_route_refuses_a_set_past_max_set():
    K, n, m, tiny, _ = pr.designed_kkt(n=48, m=80, tiny=tuple(range(0, 36)), tiny_sigma=())
    h = robust_handle()
    with pytest.raises(OkktError, match="max_set = 64") as ei:
        h.ls_factor_robust(K, n, m)
    assert "'rejected': 36" in str(ei.value)
    # the handle is left without a set and usable
    assert h._ns == 0
    assert h.ls_factor_b(K, n, m) == 1
    b = np.ones(n + m)
    assert np.isfinite(h.ls_solve(b)).all()
    with pytest.raises(OkktError, match="ls_factor_robust has not succeeded"):
        h.ls_solve_robust(K, b)
    # an explicit max_set and a round limit on the first design
    K1, n1, m1, _, _ = pr.designed_kkt()
    with pytest.raises(OkktError, match="max_set = 4"):
        h.ls_factor_robust(K1, n1, m1, max_set=4)
    with pytest.raises(OkktError, match="after 1 rounds"):
        h.ls_factor_robust(K1, n1, m1, max_rounds=1)
    assert h.ls_factor_robust(K1, n1, m1)[0] == 1
    finalize_b(h)
