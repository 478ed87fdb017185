"""GPU tests: the numeric phase on the fronts that relaxed amalgamation forms from designed trees (relaxed_trees.py), against the
simplicial oracle on the same permutation.  test_gpu_front_shapes.py and its relatives switch amalgamation off so that the designed
fronts are the ones factored; every production run has it on.  Here the merged fronts are predicted by the model of the merge rule,
and what the header promises "relaxation zeros included" is held to it: the stored pattern of L is the model's, every entry at a
relaxation-zero position is exactly 0.0 (it is 0 - sum 0 * x through the whole elimination, and zero rows times an inverse block on
the explicit-inverse route: anything else is memory nobody zeroed or a wrong scatter index), and the selected inverse, the pivot
report, the factor as an operator, the sparse right-hand sides, the batches and Schur mode work on the merged fronts.
Measured values are printed as RELAXED {json} lines.

Not covered here: partitioned and multi-GPU runs on relaxed trees; eigs, condest, GMRES and refinement, which reach the factor only
through the solve passes checked here."""
import json
import os
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle
from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ops_ref as fr  # noqa: E402
import front_trees as ft  # noqa: E402
import relaxed_trees as rt  # noqa: E402
import schur_trees as sct  # noqa: E402
import selinv_case as slc  # noqa: E402
import test_gpu_batch as gb  # noqa: E402
import test_gpu_front_shapes as fs  # noqa: E402
import test_gpu_pivots as pv  # noqa: E402
import test_gpu_schur_trees as gst  # noqa: E402
from test_gpu_front_shapes import TOL_BATCH, TOL_D, TOL_L, TOL_X  # noqa: E402
from test_relaxed_trees import expected_reach  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble

# "ipm" values, designs with a merged front of more than 384 pivot columns (explicit inverses of 1024-column blocks): forward error of
# the HIP solve / the oracle's (worst of two vectors each), measured on MI355X (the RELAXED lines of one run of this file).
# The oracle's own error on these systems is 8.0e-14 .. 4.0e-11.  The merged fronts behave as the designed ones do: the explicit
# inverses are no worse than the oracle's substitution but on k = 385 / c = 1, now one padded 1024-column block of 387 columns
# (1.96 x; 1.45 x unmerged).  forest-3-roots merges nothing: its fronts, and its figure (2.80 measured again), are those of
# test_gpu_front_shapes.py.
IPM_INV_RATIO = {
    "mixed-level": 0.11, "mixed-level-scatter": 0.33, "fan-in-8": 0.30, "deep-chain-6": 0.07, "edge-k385-c1": 1.96, "edge-k1023-c128": 0.21,
    "any-frac-under-over": 0.27, "forest-3-roots": fs.IPM_INV_RATIO["forest-3-roots"],
}


def record(**kw):
    print("RELAXED " + json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))


def hip_solver(opts, **more):
    h = linear_solver_HIP("symmetric", ordering=2, **dict(opts, **more))
    initialize_b(h)
    return h


def factored(d, opts, **more):
    h = hip_solver(opts, **more)
    h.set_perm(d.perm)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
    return h


_REF = {}


def reference(name, values="plain", seed=0):
    """(design, options, model, oracle factor, full matrix, right-hand sides, true solutions); cached, nobody changes it."""
    key = (name, values, seed)
    if key not in _REF:
        d, opts, m = rt.design(name, values=values, seed=seed)
        o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
        o.ls_factor_b(d.A, d.npos, d.nneg)
        M = ft.full_csr(d.A)
        B = ft.rhs(d.n, 5)
        XT = np.array([ft.true_solution(M, o.ls_solve, b) for b in B])
        _REF[key] = (d, opts, m, o, M, B, XT)
    return _REF[key]


class _Stored:
    """The model's stored pattern where fs.check_factor asks a design for the pattern of L."""

    def __init__(self, m):
        self.m = m

    def l_pattern(self):
        return self.m.stored_pattern()


def zero_slots(m):
    """Positions, in the data of a CSC with the model's stored pattern, of the relaxation zeros."""
    S = m.stored_pattern()
    S.data = np.arange(1, S.nnz + 1, dtype=np.float64)
    pick = S.multiply(m.zero_pattern()).tocsc()
    return pick.data.astype(np.int64) - 1


def check_factor(m, o, inertia, D, Lh, tol_d=TOL_D, tol_l=TOL_L):
    """fs.check_factor on the model's stored pattern (exact), and every relaxation zero exactly 0.0"""
    e = fs.check_factor(_Stored(m), o, inertia, D, Lh, tol_d=tol_d, tol_l=tol_l)
    Lh = sp.csc_matrix(Lh)
    Lh.sort_indices()
    z = Lh.data[zero_slots(m)]
    assert len(z) == m.fingerprint()["nnzL_stored"] - m.nnzL
    bad = np.flatnonzero(z != 0.0)
    assert len(bad) == 0, (len(bad), len(z), z[bad[:5]])
    return e


def route_of(m):
    return "inverse" if any(k > 384 and f > rt.SMALL_MAX for k, f in m.shapes) else "substitution"


# ---- a, b: the factor and the solves, plain values --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rt.GPU_DESIGNS)
def test_relaxed_fronts_plain_values(name):
    """One design under its relaxation options: the statistics and the stored pattern of the model, inertia, D and L against the
    oracle, zeros at the relaxation zeros; three solves of one vector (the last two bitwise equal), batches of 1, 4 and 5 right-hand
    sides each column within TOL_BATCH of its single solve, every solution within TOL_X of the true one; then new values on the same
    handle give bit for bit the D, L and x of a fresh handle."""
    d, opts, m, o, M, B, XT = reference(name)
    h = hip_solver(opts)
    h.set_perm(d.perm)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == o.ls_factor_b(d.A, d.npos, d.nneg)
    assert np.array_equal(h.perm(), d.perm)
    st = h.stats()
    fp = m.fingerprint()
    assert {k: st[k] for k in fp} == fp
    xs = [h.ls_solve(B[0]) for _ in range(3)]
    for x in xs:
        assert ft.fwd_err(x, XT[0]) <= TOL_X
    assert np.array_equal(xs[1], xs[2])
    e_d, e_l = check_factor(m, o, h.inertia, h.diag(), h.factor_csc())
    singles = np.array([h.ls_solve(b) for b in B])
    errs = [ft.fwd_err(x, xt) for x, xt in zip(singles, XT)]
    assert max(errs) <= TOL_X, errs
    for nrhs in (1, 4, 5):
        X = fs.solve_batch(h, B[:nrhs])
        for r in range(nrhs):
            assert np.max(np.abs(X[r] - singles[r])) <= TOL_BATCH * np.max(np.abs(singles[r])), (nrhs, r)
            assert ft.fwd_err(X[r], XT[r]) <= TOL_X, (nrhs, r)
    d2 = ft.build(rt.DESIGNS[name][0], seed=1)
    assert np.array_equal(d2.A.indices, d.A.indices) and np.array_equal(d2.A.indptr, d.A.indptr)
    runs = []
    for hh in (h, hip_solver(opts)):
        if hh is not h:
            hh.set_perm(d.perm)
        hh.ls_factor_b(d2.A, d2.npos, d2.nneg)
        runs.append((hh.inertia, hh.diag(), hh.factor_csc().data, [hh.ls_solve(B[0]) for _ in range(3)], fs.solve_batch(hh, B)))
        finalize_b(hh)
    (i1, D1, L1, x1, X1), (i2, D2, L2, x2, X2) = runs
    assert i1 == i2 and np.array_equal(D1, D2) and np.array_equal(L1, L2)
    assert not np.any(L1[zero_slots(m)] != 0.0)
    for a, b in zip(x1, x2):
        assert np.array_equal(a, b)
    assert np.array_equal(X1, X2)
    record(name=name, values="plain", route=route_of(m), fronts=m.shapes if len(m.shapes) <= 8 else len(m.shapes), err=max(errs), e_d=e_d, e_l=e_l,
           zeros=int(fp["nnzL_stored"] - fp["nnzL"]))


# ---- c: "ipm" values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rt.GPU_DESIGNS)
def test_relaxed_fronts_ipm_values(name):
    """One design, "ipm" values: inertia, D, L and the zeros as above; the forward error of two right-hand sides at most 2 x the
    oracle's where no merged front has more than 384 pivot columns -- measured 0.54 .. 1.25 x (the oracle at 6e-15 .. 5e-13) --
    and at most 2 x the ratio measured on MI355X (IPM_INV_RATIO, 0.07 .. 2.8 x) on the explicit-inverse designs.  D and L within
    TOL_D / TOL_L as for the plain values (measured at most 7.3e-12 and 7.9e-14)."""
    d, opts, m, o, M, B, XT = reference(name, "ipm")
    h = hip_solver(opts)
    h.set_perm(d.perm)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == o.ls_factor_b(d.A, d.npos, d.nneg)
    assert tuple(h.inertia[:3]) == (d.npos, d.nneg, 0)
    e_d, e_l = check_factor(m, o, h.inertia, h.diag(), h.factor_csc(), tol_d=np.inf, tol_l=np.inf)
    e_h = max(ft.fwd_err(h.ls_solve(b), xt) for b, xt in zip(B[:2], XT[:2]))
    e_o = max(ft.fwd_err(o.ls_solve(b), xt) for b, xt in zip(B[:2], XT[:2]))
    finalize_b(h)
    route = route_of(m)
    assert (route == "inverse") == (name in rt.EXPLICIT_INVERSE or name == "forest-3-roots")
    record(name=name, values="ipm", route=route, e_hip=e_h, e_oracle=e_o, ratio=e_h / e_o, e_d=e_d, e_l=e_l)
    assert e_d <= TOL_D and e_l <= TOL_L, (e_d, e_l)
    bound = 2.0 if route == "substitution" else 2.0 * IPM_INV_RATIO[name]
    assert e_h <= bound * e_o, (e_h, e_o)


# ---- d: what the header promises "relaxation zeros included" --------------------------------------------------------------------------
class Case:
    """One factored handle per design, shared by the tests of part d, with the long-double reference built from its exports."""

    def __init__(self, name):
        self.name = name
        self.d, self.opts, self.m, self.o, self.M, self.B, self.XT = reference(name)
        self.h = h = factored(self.d, self.opts)
        self.n = self.d.n
        self.F = fr.Factor(h.factor_csc(), h.diag(), h.perm())
        assert np.array_equal(self.F.colcount, 1 + np.diff(self.m.stored_pattern().indptr))        # the zeros are counted: they are summed over
        self.levels = int(h.stats()["nlevels"])
        self.gprod = fr.product_bound(self.F.cmax, self.F.rmax, self.levels)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.mark.parametrize("name", rt.PROMISE_DESIGNS)
def test_selected_inverse_on_the_stored_pattern(name):
    """Z against the dense inverse under selinv_case's tolerance rule; its pattern is the model's stored pattern with the diagonal --
    at the relaxation zeros of L the inverse is in general not zero, and has to be there; logdet against numpy's."""
    d, opts, m = reference(name)[:3]
    h = factored(d, opts)
    Z, _ = slc.check_against_dense(h, d.A, perm=d.perm)
    Z = sp.csc_matrix(Z)
    Z.sort_indices()
    P = (m.stored_pattern() + sp.identity(d.n, format="csc")).tocsc()
    P.sort_indices()
    assert np.array_equal(Z.indptr, P.indptr) and np.array_equal(Z.indices, P.indices)
    Zl = sp.tril(Z, -1).tocsc()
    Zl.sort_indices()
    at_zeros = Zl.data[zero_slots(m)]
    assert np.count_nonzero(at_zeros) >= 0.99 * len(at_zeros)          # checked against the dense inverse above, and not zero
    sign, logabs = np.linalg.slogdet(slc.dense(d.A))
    v, s = h.logdet()
    assert s == int(sign) and abs(v - logabs) <= 1e-10 * max(1.0, abs(logabs)), (v, logabs)
    record(test="selinv", name=name, zeros=len(at_zeros), max_inverse_at_zeros=float(np.max(np.abs(at_zeros))), logdet=v)
    finalize_b(h)


@pytest.mark.parametrize("name", rt.PROMISE_DESIGNS)
def test_pivot_report_on_merged_fronts(name):
    """The multipliers are the column maxima of the stored L exactly; within TOL_L max|L| of the oracle's; a partner is never a
    relaxation-zero row."""
    c = case(name)
    d, m, h = c.d, c.m, c.h
    g, p = pv.check_against_factor(h)
    Lo = abs(c.o.L()).tocsc()
    g_o = np.asarray(Lo.max(axis=0).todense()).ravel()
    assert np.max(np.abs(g[d.perm] - g_o)) <= TOL_L * Lo.max()
    Zp = m.zero_pattern()
    cols = np.flatnonzero(p[d.perm] >= 0)
    rows = d.iperm[p[d.perm][cols]]
    assert len(cols) >= d.n - len(m.fronts) and np.all(rows > cols)
    assert not np.asarray(Zp[rows, cols]).ravel().any()
    record(test="pivots", name=name, max_multiplier=float(g.max()))


@pytest.mark.parametrize("name", rt.PROMISE_DESIGNS)
def test_factor_as_operator_on_merged_fronts(name):
    """The half solves, the products and the quadratic form against the long-double restatement (factor_ops_ref.py) fed the handle's
    factor_csc() and diag(), under the bounds of test_gpu_factor_ops.py; okkt_factor_error within its bound."""
    c = case(name)
    F, h, n = c.F, c.h, c.n
    worst = {}
    # backward of forward is the solve, bit for bit; the forward half's residual
    B = ft.rhs(n, 5, seed=15)
    Zf = h.ls_solve_forward(B)
    assert h.ls_solve_backward(Zf).tobytes() == fs.solve_batch(h, B).tobytes()
    for b, z in zip(B[:3], Zf[:3]):
        assert np.all(np.isfinite(z))
        pb = F.rhs_to_factor(b)
        dz = F.d.astype(LD) * z.astype(LD)
        res = np.abs(pb - F.mul_L(dz))
        bound = fr.gamma(F.rowcount + c.levels + 1).astype(LD) * (F.mul_L(np.abs(dz), True) + np.abs(pb))
        worst["forward"] = max(worst.get("forward", 0.0), float(np.max(res / bound)))
        assert np.all(res <= bound)
    # L and L^T
    for k in (1, 3, 5):
        X = np.atleast_2d(gfo_vectors(n, k, seed=30 + k))
        Ut = h.factor_multiply("LT", X if k > 1 else X[0]).reshape(k, -1)
        Yt = h.factor_multiply("L", X if k > 1 else X[0]).reshape(k, -1)
        for x, ut, yt in zip(X, Ut, Yt):
            eu = np.abs(ut.astype(LD) - F.mul_LT(x))
            bu = fr.gamma(F.colcount).astype(LD) * F.mul_LT(np.abs(x), True)
            ey = np.abs(yt.astype(LD) - F.mul_L(x))
            by = fr.gamma(F.rowcount + c.levels).astype(LD) * F.mul_L(np.abs(x), True)
            worst["LT"] = max(worst.get("LT", 0.0), float(np.max(eu / bu)))
            worst["L"] = max(worst.get("L", 0.0), float(np.max(ey / by)))
            assert np.all(eu <= bu) and np.all(ey <= by), worst
    # L D L^T and |L||D||L^T|
    X = gfo_vectors(n, 4, seed=41)
    Y, Ya = h.factor_multiply("LDLT", X), h.factor_multiply("ABS_LDLT", X)
    for x, y, ya in zip(X, Y, Ya):
        env = c.gprod * F.mul_LDLT(x, True)
        e1 = np.abs(y.astype(LD) - F.mul_LDLT(x))
        e2 = np.abs(ya.astype(LD) - F.mul_LDLT(x, True))
        worst["LDLT"] = max(worst.get("LDLT", 0.0), float(np.max(e1 / env)), float(np.max(e2 / env)))
        assert np.all(e1 <= env) and np.all(e2 <= env) and np.all(ya >= 0), worst
    assert np.max(np.abs(Y[0] - c.M @ X[0])) <= 1e-10 * np.max(np.abs(c.M @ X[0]))
    # the quadratic form
    qp, qn = h.quadform(B)
    assert np.all(qp >= 0) and np.all(qn <= 0)
    dg = h.diag()
    for r in range(5):
        ep, en = fr.quadform_exact(dg, Zf[r])
        for got, ex in ((qp[r], ep), (qn[r], en)):
            assert abs(Fraction(float(got)) - ex) <= Fraction(2 * fr.U) * abs(ex)
    # okkt_factor_error
    info = h.factor_error(c.d.A, 2)
    ref, _, _ = fr.factor_error(F, c.d.A, 2)
    tol = 2 * c.gprod
    for k in ("norm_abs_ldlt", "norm_f", "rho"):
        assert abs(info[k] - ref[k]) <= tol * ref[k], k
    bound = fr.eta_bound(F.cmax, F.rmax, c.levels)
    assert 0 <= info["eta_row"] < n and info["eta"] <= bound
    record(test="factor_ops", name=name, worst_fraction_of_bound=worst, eta=info["eta"], eta_host=ref["eta"], eta_bound=bound)


def gfo_vectors(n, k, seed):
    """k vectors with entries of both signs and mixed magnitudes (the recipe of test_gpu_factor_ops.py)"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(k, n)) * 10.0 ** rng.integers(-2, 3, size=(k, n))


@pytest.mark.parametrize("name", rt.PROMISE_DESIGNS)
def test_sparse_right_hand_side_on_the_leaf_of_a_merged_chain(name):
    """b on the lowest node of a merged chain: okkt_solve_sparse returns the numbers of okkt_solve of the densified b at the
    requested entries (np.array_equal, the work vectors poisoned before every call), with the sets of the host call -- which are the
    model's (test_relaxed_trees.py)."""
    c = case(name)
    d, m, h = c.d, c.m, c.h
    _, _, _, row, A, _ = expected_reach(name)
    leaf = d.nodes[m.fronts[min(A)]["members"][0]]
    rows = np.array([row, int(d.perm[leaf["col0"] + leaf["k"] - 1])], dtype=np.int64)
    vals = np.array([1.5, -0.25])
    b = np.zeros(d.n)
    b[rows] = vals
    ref = fs.solve_batch(h, b[None, :])[0]
    poison = np.random.default_rng(99).normal(size=d.n) * 1e30
    other = m.fronts[0] if min(A) != 0 else m.fronts[-1]
    wants = {"all": None, "support": rows, "elsewhere": d.perm[other["col0"]:other["col0"] + 3], "duplicate": np.array([rows[0], rows[1], rows[0]])}
    for what, want in wants.items():
        assert np.max(np.abs(fs.solve_batch(h, poison[None, :]))) > 1e25
        x, info = h.ls_solve_sparse((rows, vals), want)
        expect = ref if want is None else ref[want]
        assert np.array_equal(x, expect), (what, float(np.max(np.abs(x - expect))))
        hinfo, _ = h.sparse_reach(rows, want)
        for k in ("nsuper", "fwd_reach", "bwd_reach", "fwd_run", "bwd_run", "fringe", "fringe_entries", "fwd_panel_bytes", "bwd_panel_bytes", "pruned"):
            assert info[k] == hinfo[k], (k, what)
        assert info["fwd_reach"] == len(A) and info["nsuper"] == len(m.fronts)


@pytest.mark.parametrize("mode", gb.MODES)
@pytest.mark.parametrize("name", rt.BATCH_DESIGNS)
def test_batches_on_merged_small_fronts(name, mode):
    """B = 3 items on a plan whose merged fronts all stay small: each item bitwise the factor and the solutions of a fresh handle."""
    d, opts, m = rt.design(name)
    A = sp.csc_matrix(d.A)
    plan = gb.Plan(A.indptr, A.indices, A.data, d.npos, d.nneg, perm=d.perm, ordering=2, **opts)
    vals = plan.values(3)
    ref = [gb.single(plan, vals[b], gb.rhs_sets(plan.dim, b)) for b in range(3)]
    h = plan.handle()
    st = h.stats()
    assert {k: st[k] for k in m.fingerprint()} == m.fingerprint() and st["n_big_fronts"] == 0
    assert h.batch_query()["eligible"] == 1
    h.batch_reserve(3, nrhs_max=max(gb.NRHS), mode=mode)
    flags = h.ls_factor_batch(vals, plan.n, plan.m)
    assert h.batch_mode_used() == mode
    assert [int(f) for f in flags] == [r["flag"] for r in ref] == [1, 1, 1]
    assert h.batch_inertia == [r["inertia"] for r in ref]
    for k, nrhs in enumerate(gb.NRHS):
        X = h.ls_solve_batch(np.stack([gb.rhs_sets(plan.dim, b)[k] for b in range(3)]))
        for b in range(3):
            assert gb.same(X[b], ref[b]["X"][k]), (nrhs, b)
    gb.check_factors(h, ref, range(3))
    S = m.stored_pattern()
    for r in ref:
        assert np.array_equal(r["L"].indptr, S.indptr) and np.array_equal(r["L"].indices, S.indices)
        assert not np.any(r["L"].data[zero_slots(m)] != 0.0)
    h.batch_release()
    finalize_b(h)


# ---- e: the routes (subprocesses) -----------------------------------------------------------------------------------------------------
VARIANTS = ["default", "DATAFLOW=0", "SOLVE_MID=0", "TASKS=0", "RELEASE_CB=0", "DEBUG_POISON=1", "panel_nb=64,small_front_max=32"]
_RUNS = {}


def run_case(variant, names, debug=False):
    key = (variant, tuple(names), debug)
    if key not in _RUNS:
        env, opts = fs.VARIANTS[variant]
        e = dict(os.environ)
        e.update(env)
        if debug:
            e["OKKT_DEBUG_FRONTS"] = "1"
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "case.npz")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "relaxed_trees_case.py"), out, json.dumps(opts), *names],
                               cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "CASE_OK" in r.stdout, (variant, r.stdout[-400:], r.stderr[-1500:])
            with np.load(out) as z:
                res = {k: z[k] for k in z.files}
        _RUNS[key] = (res, r.stderr)
    return _RUNS[key]


def check_case(res, name):
    d, opts, m, o, M, B, XT = reference(name)
    Lh = sp.csc_matrix((res[f"{name}/Lx"], res[f"{name}/Li"], res[f"{name}/Lp"]), shape=(d.n, d.n))
    assert np.array_equal(res[f"{name}/perm"], d.perm)
    check_factor(m, o, res[f"{name}/inertia"], res[f"{name}/D"], Lh)
    singles = res[f"{name}/singles"]
    errs = [ft.fwd_err(x, xt) for x, xt in zip(singles, XT)]
    assert max(errs) <= TOL_X, errs
    rep = res[f"{name}/rep"]
    assert np.array_equal(rep[1], rep[2]) and ft.fwd_err(rep[0], XT[0]) <= TOL_X
    for nrhs in (1, 4, 5):
        X = res[f"{name}/X{nrhs}"]
        for r in range(nrhs):
            assert np.max(np.abs(X[r] - singles[r])) <= TOL_BATCH * np.max(np.abs(singles[r])), (nrhs, r)
            assert ft.fwd_err(X[r], XT[r]) <= TOL_X, (nrhs, r)
    for k in ("D", "Lx", "inertia", "X"):
        assert np.array_equal(res[f"{name}/same/{k}"], res[f"{name}/fresh/{k}"]), k
    assert not np.any(res[f"{name}/same/Lx"][zero_slots(m)] != 0.0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_relaxed_designs_under_route_switches(variant):
    """mixed-level, fan-in-8, edge-k1023-c128 and chain-under-sep under the route switches: the checks of the plain-values test.
    Without released CBs the results are bitwise those of the default run."""
    res, _ = run_case(variant, rt.VARIANT_DESIGNS)
    for name in rt.VARIANT_DESIGNS:
        check_case(res, name)
    if variant == "RELEASE_CB=0":
        base, _ = run_case("default", rt.VARIANT_DESIGNS)
        for k in base:
            assert np.array_equal(res[k], base[k]), k


def test_every_merged_big_front_takes_its_route():
    """OKKT_DEBUG_FRONTS: each merged front of more than small_max rows is scheduled as a big front with the model's level, f and k
    (once per factorisation: the case factors every design three times), and nothing else is."""
    _, err = run_case("default", rt.VARIANT_DESIGNS, debug=True)
    routes = fs.parse_routes(err)
    for name in rt.VARIANT_DESIGNS:
        m = reference(name)[2]
        big = sorted(set(routes[name][0]))
        record(test="routes", name=name, big=big, model=m.big_fronts())
        assert big == m.big_fronts(), (name, big, m.big_fronts())
    big = {name: reference(name)[2].big_fronts() for name in rt.VARIANT_DESIGNS}
    assert (1, 760, 760) in big["mixed-level"] and (1, 550, 550) in big["fan-in-8"] and big["edge-k1023-c128"] == [(0, 1152, 1152)]
    assert big["chain-under-sep"] == []


# ---- f: Schur mode --------------------------------------------------------------------------------------------------------------------
_SREF = {}


def schur_reference(ns):
    """The reference of schur_trees.reference for the last ns columns of deep-chain-6 as the Schur set (there the set is the last
    designed node; here it may be a part of it): S and r2 in long double from refined solves with A11, the oracle's own S and r2."""
    if ns in _SREF:
        return _SREF[ns]
    name = rt.SCHUR_DESIGN
    if ns == ft.build(rt.DESIGNS[name][0]).nodes[-1]["k"]:          # the whole root: schur_trees' own case, shared with its tests
        _SREF[ns] = sct.reference(name)
        return _SREF[ns]
    d, opts, _, o, M, B, XT = reference(name)
    n1 = d.n - ns
    Mp = M[d.perm][:, d.perm].tocsr()
    Mp.sort_indices()
    A11, A21, A22 = Mp[:n1, :n1].tocsr(), Mp[n1:, :n1].tocsr(), Mp[n1:, n1:].toarray()
    D, Lo = o.diag(), o.L().tocsr()
    Bp = B[:, d.perm]
    L11, L21 = Lo[:n1, :n1], Lo[n1:, :n1]
    S_or = A22 - ((L21 @ sp.diags(D[:n1])) @ L21.T).toarray()
    Y1 = spla.spsolve_triangular((L11 + sp.identity(n1)).tocsr(), Bp[:, :n1].T.copy(), lower=True, unit_diagonal=True)
    R2_or = Bp[:, n1:] - (L21 @ Y1).T
    o1 = oracle.linear_solver_ORACLE("symmetric", perm=np.arange(n1, dtype=np.int64))
    n1pos = int((D[:n1] > 0).sum())
    o1.ls_factor_b(sp.tril(A11).tocsc(), n1pos, n1 - n1pos)
    A21l = A21.toarray().astype(LD)
    touch = np.flatnonzero(np.diff(A21.indptr) > 0)
    S_ref = A22.astype(LD)
    X = np.array([ft.true_solution(A11, o1.ls_solve, a) for a in A21[touch].toarray()]).astype(LD)
    S_ref[:, touch] -= A21l @ X.T
    X1 = np.array([ft.true_solution(A11, o1.ls_solve, b) for b in Bp[:, :n1]]).astype(LD)
    R2_ref = Bp[:, n1:].astype(LD) - X1 @ A21l.T
    S64, R264 = S_ref.astype(np.float64), R2_ref.astype(np.float64)
    smax, rmax = float(np.max(np.abs(S_ref))), float(np.max(np.abs(R2_ref)))
    pat = sp.csr_matrix((np.ones(L21.nnz), L21.indices, L21.indptr), shape=L21.shape)
    reached = (pat @ pat.T).toarray() > 0          # (i, j) of S differs from A22 where an interior column holds both rows
    _SREF[ns] = sct.Ref(name=name, d=d, ns=ns, n1=n1, idx=d.perm[n1:], n1pos=n1pos, n1neg=n1 - n1pos, M=M, B=B, XT=XT, A22=A22, S_ref=S_ref,
                        R2_ref=R2_ref, S64=S64, R264=R264, smax=smax, rmax=rmax, S_oracle=S_or, R2_oracle=R2_or,
                        e_oracle_S=float(np.max(np.abs(S_or - S_ref)) / smax), e_oracle_r2=float(np.max(np.abs(R2_or - R2_ref)) / rmax),
                        X2=np.linalg.solve(S64, R264.T).T.copy(), reached=reached, eig=np.linalg.eigvalsh(S64))
    return _SREF[ns]


@pytest.mark.parametrize("ns", [100, 300])
def test_schur_mode_on_merged_fronts(ns):
    """deep-chain-6 under the default amalgamation with its last ns columns as the Schur set (300: the root; 100: a part of it, and the
    rest of the root merges with the front below into (400, 500)): the statistics of the model, S against the long-double Schur
    complement, r2, the expansion and the fused solve under the rules of test_gpu_schur_trees.py."""
    r = schur_reference(ns)
    d, opts = r.d, reference(rt.SCHUR_DESIGN)[1]
    m = rt.merged(d, opts, nschur=ns)
    h = hip_solver(opts)
    h.set_schur(r.idx)
    h.set_perm(d.perm)
    h.analyze(d.A)
    assert np.array_equal(h.perm(), d.perm)
    st = h.stats()
    assert {k: st[k] for k in m.fingerprint()} == m.fingerprint()
    batches = (1, 4, 5)
    res = sct.device_results(h, d, r.n1pos, r.n1neg, r.B, r.X2, batches=batches)
    fig = gst.check_results(r, res, "plain", batches)
    record(test="schur", ns=ns, fronts=m.shapes, **{k: fig[k] for k in ("e_S", "e_oracle_S", "e_r2", "e_oracle_r2", "err_expand", "err_solve")})
    for nr in batches:
        assert np.array_equal(h.schur_solve(r.B[:nr]).reshape(nr, -1), res[f"xs/{nr}"])
    finalize_b(h)
