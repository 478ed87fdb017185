"""GPU tests of the symmetric equilibration before the factorisation (okkt_set_scaling, okkt_get_scaling, okkt_kkt_set_ls_scaling;
DESIGN.md section 8.8).  The scaling is a power of two, so everything is compared exactly: s against the numpy restatement
(scaling_ref.py), the factor and the solves against a plain handle that factors the prescaled matrix under the same ordering.
Measured values are printed as SCALING {json} lines."""
import json
import math
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import scaling_ref as sr  # noqa: E402
import test_gpu_condest as tc  # noqa: E402
import test_gpu_kkt_solvers as tk  # noqa: E402
import test_gpu_schur_dense_rows as td  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def record(**kw):
    def conv(v):
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, (np.floating, np.integer)):
            return v.item()
        return v
    print("SCALING " + json.dumps({k: conv(v) for k, v in kw.items()}))


# ---- the shared inputs: (A, sym, npos, nneg, perm, handle options), built once ------------------------------------------------------

_CASES = None


def _ordering_of(A):
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(A)
    p = h.perm()
    finalize_b(h)
    return p


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    for name, A in sr.small_cases().items():
        dim = sr.arrays(A)[0]
        nneg = sr.inertia_counts(A)[1]
        out[name] = dict(A=A, sym="symmetric", n=dim - nneg, m=nneg, opts={})      # (a zero eigenvalue is counted with the positive ones)
    prob = synth.make_config("S-small", seed=1)
    K = synth.augmented_matrix(prob, delta=1e-4)          # with its upper J' block, as the reference builds it
    out["S-small-K"] = dict(A=K, sym="symmetric", n=prob["n"], m=prob["m"], opts={})
    out["S-small-Q"] = dict(A=synth.schur_matrix(prob, delta=1e-4), sym="definite", n=prob["n"], m=0, opts={})
    d = ft.build(ft.DESIGNS["edge-k129-c700"][0], values="ipm")       # a big front: the dataflow launch factors scaled values
    out["edge-k129-c700"] = dict(A=sp.csc_matrix(d.A), sym="symmetric", n=d.npos, m=d.nneg, opts=dict(ft.NO_RELAX), perm=d.perm)
    for c in out.values():
        if "perm" not in c:
            c["perm"] = _ordering_of(c["A"])
        c["ref"] = {}
    _CASES = out
    return out


CASE_NAMES = ["arrow-300", "dups-upper-67", "zero-row-40", "n1", "tridiagonal-67", "S-small-K", "S-small-Q", "edge-k129-c700"]


def ref_scaling(c, sweeps):
    if sweeps not in c["ref"]:
        c["ref"][sweeps] = sr.ruiz(c["A"], sweeps)
    return c["ref"][sweeps]


def handle(c, scaling=None, sweeps=0, s=None):
    """a handle with the case's ordering; the pattern is analysed, so that a caller's vector can be set"""
    h = linear_solver_HIP(c["sym"], ordering=2, **c["opts"])
    initialize_b(h)
    h.set_perm(c["perm"])
    h.analyze(c["A"])
    if scaling is not None:
        h.set_scaling(scaling, sweeps, s)
    return h


def factor_parts(h):
    Lf = h.factor_csc()
    return h.diag(), Lf.indptr.copy(), Lf.indices.copy(), Lf.data.copy()


def same_factor(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def solve(h, B):
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(np.ascontiguousarray(B)), L.p_f64(X), B.shape[0]), "okkt_solve")
    return X


def solve_dev_in_place(h, B):
    d = h.dev_upload(B)
    h.ls_solve_dev(d, d, B.shape[0])
    X = h.dev_download(d, B.shape)
    h.dev_free(d)
    return X


# ---- 1. the scaling itself --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_scaling_equals_the_restatement(name):
    c = cases()[name]
    h = handle(c)
    for sweeps in (1, 3, 10):
        s_ref, _, iref = ref_scaling(c, sweeps)
        h.set_scaling("ruiz", sweeps)
        flag = h.ls_factor_b(c["A"], c["n"], c["m"])
        s, info = h.scaling(), h.scaling_info()
        record(test="scaling", name=name, sweeps=sweeps, flag=flag, rowmax_min=info["rowmax_min"], rowmax_max=info["rowmax_max"],
               zero_rows=info["zero_rows"], s_min=float(s.min()), s_max=float(s.max()))
        assert np.array_equal(s, s_ref), (name, sweeps, np.flatnonzero(s != s_ref)[:5])
        assert (info["mode"], info["sweeps"]) == (L.OKKT_SCALE_RUIZ, sweeps)
        assert info["rowmax_min"] == iref["rowmax_min"] and info["rowmax_max"] == iref["rowmax_max"], (info, iref)
        assert info["zero_rows"] == iref["zero_rows"]
        h.ls_factor_b(c["A"], c["n"], c["m"])
        assert np.array_equal(h.scaling(), s) and h.scaling_info() == info           # two calls: identical bits
        d = h.dev_alloc(8 * max(len(s), 1))
        h.scaling_dev(d)
        assert np.array_equal(h.dev_download(d, s.shape), s)
        h.dev_free(d)
    if name == "zero-row-40":
        assert info["zero_rows"] == 1 and s[11] == 1.0
    else:
        assert info["zero_rows"] == 0 and 0.45 < info["rowmax_min"] and info["rowmax_max"] <= 2.0
    finalize_b(h)


# ---- 2., 3. the factor and the solves against a plain handle on the prescaled matrix -------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_factor_and_solves_are_those_of_the_prescaled_matrix(name):
    c = cases()[name]
    s = ref_scaling(c, 10)[0]
    P = sr.prescaled(c["A"], s)
    dim = len(s)
    hs, hp = handle(c, "ruiz"), handle(c)
    for n, m in (((c["n"] - 1, c["m"] + 1),) if c["sym"] == "symmetric" and c["n"] > 0 else ()) + ((c["n"], c["m"]),):
        fs, fp = hs.ls_factor_b(c["A"], n, m), hp.ls_factor_b(P, n, m)
        assert fs == fp and hs.inertia == hp.inertia, (name, fs, fp, hs.inertia, hp.inertia)
        if (n, m) != (c["n"], c["m"]):
            assert fs == 0                                             # the wrong inertia: flag 0 on both
        assert same_factor(factor_parts(hs), factor_parts(hp)), name
    assert np.array_equal(hs.scaling(), s)
    B = np.random.default_rng(21).normal(size=(5, dim))
    for nr in (1, 3, 5):
        want = s * solve(hp, s * B[:nr])
        assert np.array_equal(solve(hs, B[:nr]), want, equal_nan=True), (name, nr)
        assert np.array_equal(solve_dev_in_place(hs, B[:nr]), want, equal_nan=True), (name, nr)
    record(test="prescaled", name=name, flag=fs, inertia=list(hs.inertia), factor_ms=hs.stats()["last_factor_ms"],
           factor_ms_plain=hp.stats()["last_factor_ms"])
    # 4. a caller's power-of-two vector gives the same factor and the same solves
    hu = handle(c, "user", s=s)
    assert hu.ls_factor_b(c["A"], c["n"], c["m"]) == hp.ls_factor_b(P, c["n"], c["m"]) and hu.inertia == hp.inertia
    assert same_factor(factor_parts(hu), factor_parts(hp))
    assert np.array_equal(solve(hu, B), s * solve(hp, s * B), equal_nan=True)
    iu = hu.scaling_info()
    assert np.array_equal(hu.scaling(), s) and (iu["mode"], iu["sweeps"]) == (L.OKKT_SCALE_USER, 0)
    assert iu["rowmax_min"] == ref_scaling(c, 10)[2]["rowmax_min"] and iu["rowmax_max"] == ref_scaling(c, 10)[2]["rowmax_max"]
    for h in (hs, hp, hu):
        finalize_b(h)


def test_user_vector_that_is_no_power_of_two():
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    A = synth.augmented_matrix(prob, delta=1e-4)
    c = dict(A=A, sym="symmetric", n=prob["n"], m=prob["m"], opts={}, perm=_ordering_of(A))
    s = sr.ruiz_unrounded(A, 10)
    assert np.any(np.frexp(s)[0] != 0.5)
    hu, hp = handle(c, "user", s=s), handle(c)
    assert hu.ls_factor_b(A, c["n"], c["m"]) == 1 and hp.ls_factor_b(A, c["n"], c["m"]) == 1
    assert np.array_equal(hu.scaling(), s)
    B = np.random.default_rng(22).normal(size=(3, len(s)))
    _, om_u = hu.residual(A, B, solve(hu, B))
    _, om_p = hp.residual(A, B, solve(hp, B))
    record(test="user_general", omega_scaled=om_u, omega_plain=om_p)
    assert np.all(om_u <= 4.0 * om_p), (om_u, om_p)       # the two extra roundings per entry
    finalize_b(hu)
    finalize_b(hp)


# ---- 5. the solve family on a scaled handle ---------------------------------------------------------------------------------------

def test_refine_gmres_forward_error_condest():
    c = cases()["S-small-K"]
    A = c["A"]
    hs, hn = handle(c, "ruiz"), handle(c)
    assert hs.ls_factor_b(A, c["n"], c["m"]) == 1 and hn.ls_factor_b(A, c["n"], c["m"]) == 1
    B = np.random.default_rng(23).normal(size=(3, A.shape[0]))
    out = {}
    for tag, h in (("scaled", hs), ("plain", hn)):
        X0, i0 = h.ls_solve_refine(A, B, max_steps=0)
        assert np.array_equal(X0, solve(h, B))
        Xr, ir = h.ls_solve_refine(A, B, max_steps=5)
        Xg0, ig0 = h.ls_solve_gmres(A, B, max_iters=0)
        assert np.array_equal(Xg0, solve(h, B)) and ig0["iterations"] == 0
        Xg, ig = h.ls_solve_gmres(A, B)
        ferr, berr = h.forward_error(A, B, X0)
        _, om0 = h.residual(A, B, X0)
        ce = h.condest(A)
        out[tag] = dict(omega0=i0["omega0"], refine_status=ir["status"], refine_omega=ir["omega"], gmres_status=ig["status"],
                        gmres_omega=ig["omega"], gmres_iterations=ig["iterations"], ferr=float(np.max(ferr)), norm1=ce["norm1"],
                        inv_norm1=ce["inv_norm1"], cond1=ce["cond1"])
        assert np.array_equal(berr, om0) and np.all(np.isfinite(ferr))
        if tag == "scaled":
            assert ig["status"] == 0 and ig["omega"] <= EPS, ig
            assert ir["omega"] <= i0["omega0"]
    record(test="solve_family", name="S-small-K", **{f"{k}_{t}": v for t, o in out.items() for k, v in o.items()})
    assert out["scaled"]["norm1"] == out["plain"]["norm1"]           # ||F||_1 of the unscaled matrix, bit for bit
    finalize_b(hs)
    finalize_b(hn)


def test_condest_bracket_on_a_scaled_handle(monkeypatch):
    """the estimate of ||F^-1||_1 through x = S F~^-1 S b must satisfy the checks of test_gpu_condest.py against the dense inverse: that
    test itself runs here, on its S-small case, with its handles scaled"""
    def scaled_factored(A, npos, nneg, perm=None, **o):
        h = linear_solver_HIP("symmetric", **o)
        initialize_b(h)
        if perm is not None:
            h.set_perm(perm)
        h.set_scaling("ruiz")
        h.ls_factor_b(A, npos, nneg)
        assert h.scaling_info()["mode"] == L.OKKT_SCALE_RUIZ
        return h
    prob = synth.make_config("S-small", seed=3, well_scaled=True)                 # the S-small case of that test
    K = sp.csc_matrix(sp.tril(synth.augmented_matrix(prob, delta=1e-8)))
    monkeypatch.setattr(tc, "CASES", [("S-small", K, tc.cr.dense_symmetric(K), False)])
    monkeypatch.setattr(tc, "factored", scaled_factored)
    tc.test_condest_against_dense_inverse_and_restatement(2)


# ---- 6. the log-determinant -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["arrow-300", "S-small-K", "tridiagonal-67"])
def test_logdet(name):
    c = cases()[name]
    s, e, _ = ref_scaling(c, 10)
    hs, hp = handle(c, "ruiz"), handle(c)
    hs.ls_factor_b(c["A"], c["n"], c["m"])
    hp.ls_factor_b(sr.prescaled(c["A"], s), c["n"], c["m"])
    v, sg = hs.logdet()
    vp, sgp = hp.logdet()
    esum = int(e.sum())
    want = vp - 2.0 * math.log(2.0) * esum
    record(test="logdet", name=name, logdet=v, logdet_prescaled=vp, exponent_sum=esum, sign=sg)
    assert sg == sgp
    assert abs(v - want) <= 8 * EPS * (abs(vp) + 2.0 * math.log(2.0) * abs(esum)), (v, want)
    finalize_b(hs)
    finalize_b(hp)


# ---- 7. a non-finite entry -------------------------------------------------------------------------------------------------------

def test_nan_entry():
    c = cases()["S-small-K"]
    A = sp.csc_matrix(c["A"], copy=True)
    low = np.flatnonzero(A.indices[A.indptr[5]:A.indptr[6]] > 5)
    A.data[A.indptr[5] + low[0]] = np.nan
    hs, hn = handle(c, "ruiz"), handle(c)
    fs, fn = hs.ls_factor_b(A, c["n"], c["m"]), hn.ls_factor_b(A, c["n"], c["m"])
    s = hs.scaling()
    record(test="nan", flag=fs, inertia=list(hs.inertia), inertia_plain=list(hn.inertia))
    assert fs == 0 and fn == 0 and hs.inertia == hn.inertia and hs.inertia[3] > 0
    assert np.all(np.isfinite(s)) and np.all(s > 0)
    finalize_b(hs)
    finalize_b(hn)


# ---- 8. the refusals, each followed by a call that works ---------------------------------------------------------------------------

def test_refusals_and_back_to_none():
    c = cases()["S-small-K"]
    A, n, m = c["A"], c["n"], c["m"]
    dim = A.shape[0]
    b = np.random.default_rng(24).normal(size=dim)

    def works(h):
        assert h.ls_factor_b(A, n, m) == 1 and np.all(np.isfinite(h.ls_solve(b)))

    h = handle(c)
    lib = h._lib
    msg = lambda: lib.okkt_last_error(h._h).decode()
    out = np.zeros(dim)
    # no scaled factorisation yet
    assert lib.okkt_get_scaling(h._h, L.p_f64(out), None) == L.OKKT_ERR_INVALID and "scaling" in msg()
    works(h)
    assert lib.okkt_get_scaling(h._h, L.p_f64(out), None) == L.OKKT_ERR_INVALID           # a plain factor holds no scaling
    # bad arguments
    for args, what in (((7, 0, None), "mode"), ((L.OKKT_SCALE_RUIZ, 65, None), "sweeps"), ((L.OKKT_SCALE_USER, 0, None), "NULL")):
        assert lib.okkt_set_scaling(h._h, *args) == L.OKKT_ERR_INVALID and what in msg()
        works(h)
    for bad in (np.nan, np.inf, 0.0, -2.0):
        v = np.ones(dim)
        v[17] = bad
        assert lib.okkt_set_scaling(h._h, L.OKKT_SCALE_USER, 0, L.p_f64(v)) == L.OKKT_ERR_INVALID and "s_user[17]" in msg()
    works(h)
    assert lib.okkt_get_scaling(h._h, L.p_f64(out), None) == L.OKKT_ERR_INVALID           # none of the refused calls took effect
    # a caller's vector given for another dimension: refused by the next factorisation
    small = sp.identity(5, format="csc")
    h5 = linear_solver_HIP("symmetric")
    initialize_b(h5)
    h5.analyze(small)
    h5.set_scaling("user", s=np.full(5, 2.0))
    assert h5.ls_factor_b(small, 5, 0) == 1 and np.array_equal(h5.ls_solve(np.ones(5)), np.ones(5))
    with pytest.raises(OkktError, match="another dimension"):
        h5.ls_factor_b(sp.identity(6, format="csc"), 6, 0)
    h5.set_scaling("none")
    assert h5.ls_factor_b(sp.identity(6, format="csc"), 6, 0) == 1
    finalize_b(h5)
    # selected inversion of a scaled factor, then of a plain one
    h.set_scaling("ruiz")
    works(h)
    with pytest.raises(OkktError, match="scaled factor"):
        h.selinv()
    assert h.logdet()[1] != 0
    # Schur mode and partitions while a scaling is on
    idx = np.array([0, n], dtype=np.int64)
    assert lib.okkt_set_schur(h._h, 2, L.p_i64(idx)) == L.OKKT_ERR_INVALID and "scaling" in msg()
    assert lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_ERR_INVALID and "scaling" in msg()
    works(h)
    assert h.scaling_info()["mode"] == L.OKKT_SCALE_RUIZ
    # a factor call refused for its arguments leaves the scaled factor, and its s, as they were: also with a new vector waiting
    x_before, s_before = h.ls_solve(b), h.scaling()
    h.set_scaling("user", s=np.full(dim, 8.0))
    with pytest.raises(OkktError, match="does not match"):
        h.ls_factor_b(A, n + 1, m)
    assert np.array_equal(h.scaling(), s_before) and np.array_equal(h.ls_solve(b), x_before)
    h.set_scaling("none")
    works(h)
    assert h.selinv()["status"] == 0
    # after NONE: the factor and the solution of a handle that never had a scaling
    h0 = handle(c)
    works(h0)
    assert same_factor(factor_parts(h), factor_parts(h0)) and np.array_equal(h.ls_solve(b), h0.ls_solve(b))
    finalize_b(h0)
    finalize_b(h)
    # a scaling on a handle in Schur mode or partitioned, then on the same handle out of it
    g = linear_solver_HIP("symmetric")
    initialize_b(g)
    msg = lambda: lib.okkt_last_error(g._h).decode()
    g.set_schur(idx)
    g.analyze(A)
    assert lib.okkt_set_scaling(g._h, L.OKKT_SCALE_RUIZ, 0, None) == L.OKKT_ERR_INVALID and "Schur mode" in msg()
    g.set_schur(np.array([], dtype=np.int64))
    g.analyze(A)
    assert lib.okkt_dist_set_partition(g._h, 2, 0) == L.OKKT_OK
    assert lib.okkt_set_scaling(g._h, L.OKKT_SCALE_RUIZ, 0, None) == L.OKKT_ERR_INVALID and "partitioned" in msg()
    assert lib.okkt_dist_set_partition(g._h, 1, 0) == L.OKKT_OK
    g.set_scaling("ruiz", 3)
    works(g)
    assert np.array_equal(g.scaling(), ref_scaling(c, 3)[0])
    # a re-analysis keeps the mode and drops the vector
    g.analyze(sp.identity(4, format="csc"))
    assert lib.okkt_get_scaling(g._h, L.p_f64(out), None) == L.OKKT_ERR_INVALID
    assert g.ls_factor_b(sp.identity(4, format="csc"), 4, 0) == 1 and g.scaling_info()["sweeps"] == 3
    finalize_b(g)


# ---- 9. the KKT level ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,opts", [("symmetric", {}), ("schur", {}), ("schur", dict(schur_dense_rows=-1))])
def test_kkt_delta_loop_is_unchanged(kind, opts):
    prob = synth.make_config("S-small", seed=5, convex=False, well_scaled=True)
    if opts:
        prob = td.with_dense_rows(prob, 3, seed=5)
    got = {}
    for on in (0, 1):
        it = tk.synth_iterate(prob, KS.Class_iterate)
        k = KS.HIP_KKT_solver(kind, hip_ls_scaling=on, **opts)
        k.initialize_b(it)
        k.form_system_b(it)
        status, num_fac, delta = k.ipopt_strategy_b(it)
        flag = k.factor_b(delta)                                     # a complete factorisation at the delta the loop ended with
        # okkt_kkt_condest keeps describing the unscaled system: its exact ||F||_1 does not move
        got[on] = (status, num_fac, delta, flag, tuple(k.inertia), k.condest()["norm1"])
        ls = linear_solver_HIP.of_kkt(k)
        if on:
            info = ls.scaling_info()
            assert info["mode"] == L.OKKT_SCALE_RUIZ and info["sweeps"] == 10 and 0.45 < info["rowmax_min"] and info["rowmax_max"] <= 2.0
        else:
            assert ls._lib.okkt_get_scaling(ls._h, L.p_f64(np.zeros(ls._dim)), None) == L.OKKT_ERR_INVALID
        ls._finalize()
        k.finalize_b()
    record(test="kkt_delta_loop", kind=kind, dense_rows=bool(opts), off=list(got[0][:3]), on=list(got[1][:3]))
    assert got[0] == got[1] and got[0][1] >= 1, got


@pytest.mark.parametrize("kind", ["schur", "symmetric"])
def test_kkt_directions_pass_the_oracle_comparison(kind, monkeypatch):
    """test_gpu_kkt_solvers.py's comparison with the oracle, its tolerances included, run with kkt!hip_ls_scaling = 1"""
    plain = tk.test_kkt_solver

    def scaled(rec_or_it, kind, delta=None, Iterate=KS.Class_iterate, **opts):
        inertia, k = plain(rec_or_it, kind, delta=delta, Iterate=Iterate, hip_ls_scaling=1, **opts)
        ls = linear_solver_HIP.of_kkt(k)
        assert ls.scaling_info()["mode"] == L.OKKT_SCALE_RUIZ
        ls._finalize()
        return inertia, k
    monkeypatch.setattr(tk, "test_kkt_solver", scaled)
    tk.test_synthetic_directions_vs_oracle("S-small", 0, kind)


def test_kkt_bordered_directions_pass_the_oracle_comparison(monkeypatch):
    """test_gpu_schur_dense_rows.py's comparison with the oracle run with kkt!hip_ls_scaling = 1"""
    plain = td.solver
    monkeypatch.setattr(td, "solver", lambda kind, it, delta=None, **opts: plain(kind, it, delta, hip_ls_scaling=1, **opts))
    td.test_directions_against_the_oracle("schur", 3, 4)


def test_kkt_clever_symmetric_refuses():
    k = KS.HIP_KKT_solver("clever_symmetric", hip_ls_scaling=1)
    prob = synth.make_config("S-tiny", seed=0, well_scaled=True)
    with pytest.raises(OkktError, match="okkt_kkt_set_rescale"):
        k.initialize_b(tk.synth_iterate(prob, KS.Class_iterate))
    # the handle stays usable
    assert k._lib.okkt_kkt_set_rescale(k._k, 0, 1e-2, 1.0) == L.OKKT_OK
    k.finalize_b()


# ---- 10. what the scaling buys on the natural spread --------------------------------------------------------------------------------

def test_measured_accuracy_on_s_small():
    c = cases()["S-small-K"]
    A = c["A"]
    b = np.random.default_rng(25).normal(size=A.shape[0])
    vals, xs = {}, {}
    for tag, mode in (("plain", None), ("scaled", "ruiz")):
        h = handle(c, mode)
        assert h.ls_factor_b(A, c["n"], c["m"]) == 1
        x, info = h.ls_solve_refine(A, b, max_steps=0)
        xs[tag] = x
        ferr, _ = h.forward_error(A, b, x)
        ce = h.condest(A)
        vals[tag] = dict(omega0=info["omega0"], ferr=float(ferr), cond1=ce["cond1"], factor_ms=h.stats()["last_factor_ms"],
                         solve_ms=h.stats()["last_solve_ms"])
        finalize_b(h)
    # a factorisation that never pivots is invariant under an exact scaling: recorded, not required (an underflow would break it)
    record(test="accuracy", name="S-small-K", solution_bitwise_equal=bool(np.array_equal(xs["plain"], xs["scaled"])),
           **{f"{k}_{t}": v for t, o in vals.items() for k, v in o.items()})
    assert all(np.isfinite(v) for o in vals.values() for v in o.values())
