"""GPU tests of the factor as an operator: the half solves, the quadratic form, the products with L, L^T,
L D L^T and |L||D||L^T|, and okkt_factor_error, on designed trees (front_trees.py) against the long-double reference of
factor_ops_ref.py built from the handle's own factor_csc(), diag(), perm() and scaling().

The designs are the smallest of the catalogue that put a front on every solve route (thresholds: small_front_max = 128 in
okkt_default_opts; NB = 128, solve_mid = 384 and kSolveBlock = 1024 in solve.hip / numeric.h) and on every path of the product kernels
(factor_ops.h: 8-column groups against 1024-row chunks for L^T x, 256-row blocks against 512-column blocks for L x):
  small-classes-f32-33-64-65-128-129   the one-wave kernels up to f = 128 and the first big front (f = 129, k = 113: thin) under a small root
  edge-k129-c700                       k = 129: the first pivot block past the thin route (mid), under a wide root (k = 701)
  thin-k128-f2049                      k = 128: the last thin pivot block, columns of 2048 rows (three row chunks), a wide root of 1922
                                       columns (four column blocks, two 1024-column inverses)
  mixed-level-scatter                  thin, mid, wide and small children of different classes under one parent, scattered contribution
                                       blocks, a forest with two roots; also run with a power-of-two Ruiz scaling
The bounds (u = 2^-53, gamma_m = m u / (1 - m u), c_j / r_i the column / row counts of L with the unit diagonal, h the levels of the
tree) hold for any summation order: they are conditions, not tuned numbers.  Measured values are printed as FACTOR_OPS {json}."""
import ctypes as C
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ops_ref as fr  # noqa: E402
import front_trees as ft  # noqa: E402

pytestmark = pytest.mark.gpu
U = fr.U
LD = np.longdouble

DESIGNS = ["small-classes-f32-33-64-65-128-129", "edge-k129-c700", "thin-k128-f2049", "mixed-level-scatter"]
CASES = [(name, False) for name in DESIGNS] + [("mixed-level-scatter", True)]
IDS = [name + ("+ruiz" if sc else "") for name, sc in CASES]


def record(**kw):
    print("FACTOR_OPS " + json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))


class Case:
    """One factored handle per (design, scaling), shared by the tests of the module, with the reference built from its exports."""

    def __init__(self, name, scaled):
        self.name, self.scaled = name, scaled
        self.d = d = ft.build(ft.DESIGNS[name][0])
        self.h = h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
        initialize_b(h)
        h.set_perm(d.perm)
        if scaled:
            h.set_scaling("ruiz")
        assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
        s = h.scaling() if scaled else None
        if scaled:
            assert np.all(np.frexp(s)[0] == 0.5) and len(np.unique(s)) > 1      # powers of two, not all the same
        self.F = fr.Factor(h.factor_csc(), h.diag(), h.perm(), s)
        _, cnt = h.etree()
        assert np.array_equal(self.F.colcount, cnt)       # c_j of okkt_get_etree: no relaxation zeros in these designs
        self.levels = int(h.stats()["nlevels"])
        self.n = d.n
        self.gprod = fr.product_bound(self.F.cmax, self.F.rmax, self.levels)


_CASES = {}


def case(name, scaled=False):
    if (name, scaled) not in _CASES:
        _CASES[(name, scaled)] = Case(name, scaled)
    return _CASES[(name, scaled)]


def solve_batch(h, B):
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(np.ascontiguousarray(B)), L.p_f64(X), B.shape[0]), "okkt_solve")
    return X


def vectors(n, k, seed):
    """k vectors with entries of both signs and mixed magnitudes"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(k, n)) * 10.0 ** rng.integers(-2, 3, size=(k, n))


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_backward_of_forward_is_the_solve_bit_for_bit(name, scaled):
    c = case(name, scaled)
    h = c.h
    for nrhs in (1, 2, 3, 4, 5, 7):
        B = ft.rhs(c.n, nrhs, seed=10 + nrhs)
        X = solve_batch(h, B)
        Z = h.ls_solve_forward(B)
        assert Z.shape == B.shape and np.all(np.isfinite(Z))
        X2 = h.ls_solve_backward(Z)
        assert X2.tobytes() == X.tobytes(), nrhs
    # a column's z does not depend on the batch it travelled in
    B = ft.rhs(c.n, 7, seed=3)
    Z = h.ls_solve_forward(B)
    for r in (0, 3, 4, 6):
        assert h.ls_solve_forward(B[r]).tobytes() == Z[r].tobytes()
    # rhs aliased to z, z aliased to sol
    buf = np.ascontiguousarray(B.copy())
    h._check(h._lib.okkt_solve_forward(h._h, L.p_f64(buf), L.p_f64(buf), 7), "okkt_solve_forward")
    assert buf.tobytes() == Z.tobytes()
    h._check(h._lib.okkt_solve_backward(h._h, L.p_f64(buf), L.p_f64(buf), 7), "okkt_solve_backward")
    assert buf.tobytes() == solve_batch(h, B).tobytes()


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_forward_half_solve_residual(name, scaled):
    """z finite and P S b - L (D z), in long double, within gamma_{r_i + h + 1} (|L||D||z| + |P S b|)_i"""
    c = case(name, scaled)
    F = c.F
    B = ft.rhs(c.n, 3, seed=21)
    Z = c.h.ls_solve_forward(B)
    worst = 0.0
    for b, z in zip(B, Z):
        assert np.all(np.isfinite(z))
        pb = F.rhs_to_factor(b)
        dz = F.d.astype(LD) * z.astype(LD)
        res = np.abs(pb - F.mul_L(dz))
        bound = fr.gamma(F.rowcount + c.levels + 1).astype(LD) * (F.mul_L(np.abs(dz), True) + np.abs(pb))
        worst = max(worst, float(np.max(res / bound)))
        assert np.all(res <= bound), float(np.max(res / bound))
    record(test="forward", case=name, scaled=scaled, worst_fraction_of_bound=worst)


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_products_with_L_and_LT(name, scaled):
    """|u^ - u|_j <= gamma_{c_j} (|L^T||x|)_j and |y^ - y|_i <= gamma_{r_i + h} (|L||v|)_i, for batches of 1, 3 and 5 columns"""
    c = case(name, scaled)
    F, h = c.F, c.h
    worst = {"LT": 0.0, "L": 0.0}
    for k in (1, 3, 5):
        X = vectors(c.n, k, seed=30 + k)
        Ut = h.factor_multiply("LT", X if k > 1 else X[0]).reshape(k, -1)
        Yt = h.factor_multiply("L", X if k > 1 else X[0]).reshape(k, -1)
        for x, ut, yt in zip(X, Ut, Yt):
            eu = np.abs(ut.astype(LD) - F.mul_LT(x))
            bu = fr.gamma(F.colcount).astype(LD) * F.mul_LT(np.abs(x), True)
            ey = np.abs(yt.astype(LD) - F.mul_L(x))
            by = fr.gamma(F.rowcount + c.levels).astype(LD) * F.mul_L(np.abs(x), True)
            worst["LT"] = max(worst["LT"], float(np.max(eu / bu)))
            worst["L"] = max(worst["L"], float(np.max(ey / by)))
            assert np.all(eu <= bu), float(np.max(eu / bu))
            assert np.all(ey <= by), float(np.max(ey / by))
    # two calls give the same bits; x may alias y
    X = vectors(c.n, 5, seed=39)
    for op in ("L", "LT", "LDLT", "ABS_LDLT"):
        Y = h.factor_multiply(op, X)
        assert h.factor_multiply(op, X).tobytes() == Y.tobytes()
        assert h.factor_multiply(op, X[4]).tobytes() == Y[4].tobytes()
        buf = np.ascontiguousarray(X.copy())
        h._check(h._lib.okkt_factor_multiply(h._h, L.OKKT_OP[op], L.p_f64(buf), L.p_f64(buf), 5), "okkt_factor_multiply")
        assert buf.tobytes() == Y.tobytes()
    record(test="L_LT", case=name, scaled=scaled, worst_fraction_of_bound=worst)


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_products_LDLT_and_ABS_LDLT(name, scaled):
    """error <= gamma_{cmax + rmax + h + 2} (|L||D||L^T||x|)_i in original coordinates; with the scaling on, the reference places S^-1
    and P, and the product is F x of the UNSCALED matrix up to the factorisation's error"""
    c = case(name, scaled)
    F, h = c.F, c.h
    X = vectors(c.n, 4, seed=41)
    Y = h.factor_multiply("LDLT", X)
    Ya = h.factor_multiply("ABS_LDLT", X)
    worst = 0.0
    for x, y, ya in zip(X, Y, Ya):
        env = c.gprod * F.mul_LDLT(x, True)
        e1 = np.abs(y.astype(LD) - F.mul_LDLT(x))
        e2 = np.abs(ya.astype(LD) - F.mul_LDLT(x, True))
        worst = max(worst, float(np.max(e1 / env)), float(np.max(e2 / env)))
        assert np.all(e1 <= env) and np.all(e2 <= env), worst
        assert np.all(ya >= 0)
    M = ft.full_csr(c.d.A)
    assert np.max(np.abs(Y[0] - M @ X[0])) <= 1e-10 * np.max(np.abs(M @ X[0]))
    record(test="LDLT", case=name, scaled=scaled, worst_fraction_of_bound=worst)


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_product_of_the_solution_returns_the_right_hand_side(name, scaled):
    """|LDLT(x^) - b|_i <= gamma_{cmax + rmax + h + 2} (|L||D||L^T||x^|)_i + omega (|F||x^| + |b|)_i with omega of residual()"""
    c = case(name, scaled)
    F, h = c.F, c.h
    b = ft.rhs(c.n, 1, seed=51)[0]
    x = h.ls_solve(b)
    _, omega = h.residual(c.d.A, b, x)
    y = h.factor_multiply("LDLT", x)
    Mx = fr.Matrix(c.d.A).mul(x, absolute=True)
    bound = c.gprod * F.mul_LDLT(x, True) + LD(omega) * (Mx + np.abs(b))
    err = np.abs(y.astype(LD) - b.astype(LD))
    record(test="identity", case=name, scaled=scaled, omega=float(omega), worst_fraction_of_bound=float(np.max(err / bound)))
    assert np.all(err <= bound), float(np.max(err / bound))


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_quadform(name, scaled):
    """|q^ - q| <= 2 u |q| against the exact sums over the device's own z and D; two calls bitwise equal; q_pos >= 0 >= q_neg"""
    c = case(name, scaled)
    h = c.h
    B = ft.rhs(c.n, 5, seed=61)
    qp, qn = h.quadform(B)
    qp2, qn2 = h.quadform(B)
    assert qp.tobytes() == qp2.tobytes() and qn.tobytes() == qn2.tobytes()
    q1 = h.quadform(B[4])
    assert (q1[0], q1[1]) == (qp[4], qn[4])
    assert np.all(qp >= 0) and np.all(qn <= 0)
    Z = h.ls_solve_forward(B)
    d = h.diag()
    worst = Fraction(0)
    for r in range(5):
        ep, en = fr.quadform_exact(d, Z[r])
        for got, ex in ((qp[r], ep), (qn[r], en)):
            err = abs(Fraction(float(got)) - ex)
            assert err <= Fraction(2 * U) * abs(ex), float(err / abs(ex))
            worst = max(worst, err / abs(ex) if ex else Fraction(0))
    # b' F^-1 b
    x = h.ls_solve(B[0])
    assert abs((qp[0] + qn[0]) - B[0] @ x) <= 1e-9 * (qp[0] - qn[0])
    record(test="quadform", case=name, scaled=scaled, worst_relative_error=float(worst))


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_factor_error(name, scaled):
    """norm_abs_ldlt and rho within 2 gamma_{cmax + rmax + h + 2} of the host values, eta at or below the bound of section 8.12, two
    calls bitwise equal"""
    c = case(name, scaled)
    F, h = c.F, c.h
    info = h.factor_error(c.d.A, 2)
    again = h.factor_error(c.d.A, 2)
    assert info == again
    ref, quot, _ = fr.factor_error(F, c.d.A, 2)
    tol = 2 * c.gprod
    assert abs(info["norm_abs_ldlt"] - ref["norm_abs_ldlt"]) <= tol * ref["norm_abs_ldlt"]
    assert abs(info["norm_f"] - ref["norm_f"]) <= tol * ref["norm_f"]
    assert abs(info["rho"] - ref["rho"]) <= tol * ref["rho"]
    bound = fr.eta_bound(F.cmax, F.rmax, c.levels)
    record(test="factor_error", case=name, scaled=scaled, rho=info["rho"], eta=info["eta"], eta_row=info["eta_row"], eta_host=ref["eta"],
           eta_bound=bound, cmax=F.cmax, rmax=F.rmax, levels=c.levels)
    assert 0 <= info["eta_row"] < c.n and info["probes"] == 2
    assert info["eta"] <= bound
    assert h.factor_error(c.d.A, 0)["probes"] == 2
    # more probes: the maximum cannot fall; five probes take two passes
    five = h.factor_error(c.d.A, 5)
    assert five["probes"] == 5 and five["eta"] >= info["eta"] and five["eta"] <= bound
    assert (five["rho"], five["norm_f"], five["norm_abs_ldlt"]) == (info["rho"], info["norm_f"], info["norm_abs_ldlt"])


def test_factor_error_negative_control():
    """The values with the largest diagonal entry multiplied by 1 + 2^-20 against the factor of the unperturbed matrix: eta is at least
    half of the quotient the perturbed row must produce, which lies above the bound (test_factor_ops_host.py confirms that)."""
    c = case(fr.CONTROL)
    F, h = c.F, c.h
    Ap, row, quotient = fr.perturbed(c.d.A, F)
    bound = fr.eta_bound(F.cmax, F.rmax, c.levels)
    assert quotient / 2 > bound
    info = h.factor_error(Ap, 2)
    record(test="negative_control", eta=info["eta"], eta_row=info["eta_row"], row=row, quotient=quotient, bound=bound)
    assert info["eta"] >= quotient / 2
    assert info["eta_row"] == row


def test_device_pointer_forms_give_the_same_bits():
    c = case("small-classes-f32-33-64-65-128-129")
    h, n = c.h, c.n
    B = ft.rhs(n, 5, seed=71)
    d_b = h.dev_upload(B)
    d_y = h.dev_alloc(B.nbytes)
    try:
        h.ls_solve_forward_dev(d_b, d_y, 5)
        Z = h.dev_download(d_y, B.shape)
        assert Z.tobytes() == h.ls_solve_forward(B).tobytes()
        h.ls_solve_backward_dev(d_y, d_y, 5)
        assert h.dev_download(d_y, B.shape).tobytes() == solve_batch(h, B).tobytes()
        qp, qn = h.quadform_dev(d_b, 5)
        qp2, qn2 = h.quadform(B)
        assert qp.tobytes() == qp2.tobytes() and qn.tobytes() == qn2.tobytes()
        for op in ("L", "LT", "LDLT", "ABS_LDLT"):
            h.factor_multiply_dev(op, d_b, d_y, 5)
            assert h.dev_download(d_y, B.shape).tobytes() == h.factor_multiply(op, B).tobytes()
        d_v = h.dev_upload(L.f64(sp.csc_matrix(c.d.A).data))
        assert h.factor_error_dev(d_v, 2) == h.factor_error(c.d.A, 2)
        h.dev_free(d_v)
    finally:
        h.dev_free(d_b)
        h.dev_free(d_y)


def test_of_kkt_serves_the_kkt_factor_with_its_shift():
    """The level-1 handle of a KKT solver: the factor is that of K + delta on the H block, the shift the factorisation added at assembly.
    okkt_factor_error takes the values WITHOUT the shift (k.matrix()) and adds it itself: with delta = 1e-2 an ignored shift would show
    as eta ~ 1e-4."""
    prob = synth.make_config("S-small", seed=0, well_scaled=True)
    rng = np.random.default_rng(0)
    it = KS.Class_iterate(x=rng.normal(size=prob["n"]), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                          grad=rng.normal(size=prob["n"]), cons=prob["s"] + 0.1 * rng.normal(size=prob["m"]), a_norm_penalty_par=1e-4)
    k = KS.HIP_KKT_solver("symmetric", KS.Class_parameters())
    k.initialize_b(it)
    k.form_system_b(it)
    delta = 1e-2
    assert k.factor_b(delta) == 1
    K0 = k.matrix()
    ls = linear_solver_HIP.of_kkt(k)
    n = K0.shape[0]
    Kd = sp.csc_matrix(K0 + sp.diags(np.concatenate([np.full(it.dim(), delta), np.zeros(n - it.dim())])))
    F = fr.Factor(ls.factor_csc(), ls.diag(), ls.perm())
    levels = int(ls.stats()["nlevels"])
    b = rng.normal(size=n)
    assert ls.ls_solve_backward(ls.ls_solve_forward(b)).tobytes() == ls.ls_solve(b).tobytes()
    y = ls.factor_multiply("LDLT", b)
    ref = fr.Matrix(Kd).mul(b).astype(np.float64)
    assert np.max(np.abs(y - ref)) <= 1e-10 * np.max(np.abs(ref))
    info = ls.factor_error(K0, 2)
    host, _, _ = fr.factor_error(F, Kd, 2)
    bound = fr.eta_bound(F.cmax, F.rmax, levels)
    record(test="of_kkt", eta=info["eta"], eta_host=host["eta"], rho=info["rho"], bound=bound)
    tol = 2 * fr.product_bound(F.cmax, F.rmax, levels)
    assert abs(info["norm_f"] - host["norm_f"]) <= tol * host["norm_f"] and abs(info["rho"] - host["rho"]) <= tol * host["rho"]
    assert info["eta"] <= bound
    ls._finalize()


def _all_calls(h, n, nrhs=1, op=L.OKKT_OP_LDLT, probes=2, vals=None):
    """return codes of the host forms of the five calls"""
    lib = h._lib
    b = np.ones(max(nrhs, 1) * n)
    x = np.zeros_like(b)
    q = np.zeros(max(nrhs, 1))
    info = L.OkktFactorErrorInfo()
    return [lib.okkt_solve_forward(h._h, L.p_f64(b), L.p_f64(x), nrhs), lib.okkt_solve_backward(h._h, L.p_f64(b), L.p_f64(x), nrhs),
            lib.okkt_quadform(h._h, L.p_f64(b), nrhs, L.p_f64(q), L.p_f64(q.copy())),
            lib.okkt_factor_multiply(h._h, op, L.p_f64(b), L.p_f64(x), nrhs),
            lib.okkt_factor_error(h._h, L.p_f64(vals), probes, C.byref(info))]


def test_refusals_leave_the_handle_usable():
    d = ft.build(ft.DESIGNS["small-classes-f32-33-64-65-128-129"][0])
    vals = L.f64(sp.csc_matrix(d.A).data)
    h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(h)
    h.set_perm(d.perm)
    h.analyze(d.A)
    # before a factorisation
    assert _all_calls(h, d.n, vals=vals) == [L.OKKT_ERR_INVALID] * 5
    assert "complete factorisation" in h._lib.okkt_last_error(h._h).decode()
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
    b = ft.rhs(d.n, 1)[0]
    x = h.ls_solve(b)
    assert _all_calls(h, d.n, vals=vals) == [L.OKKT_OK] * 5
    # nrhs < 0, an unknown op, too many probes
    assert _all_calls(h, d.n, nrhs=-1, vals=vals)[:4] == [L.OKKT_ERR_INVALID] * 4
    assert _all_calls(h, d.n, op=7, vals=vals)[3] == L.OKKT_ERR_INVALID
    assert _all_calls(h, d.n, probes=9, vals=vals)[4] == L.OKKT_ERR_INVALID
    assert _all_calls(h, d.n, nrhs=0, vals=vals)[:4] == [L.OKKT_OK] * 4
    assert h.ls_solve(b).tobytes() == x.tobytes()
    # after an early exit that stopped short
    h._check(h._lib.okkt_set_early_exit(h._h, 1), "okkt_set_early_exit")
    if h.ls_factor_b(d.A, d.nneg, d.npos) == 0 and h._lib.okkt_solve(h._h, L.p_f64(b), L.p_f64(np.zeros(d.n)), 1) == L.OKKT_ERR_INVALID:
        assert _all_calls(h, d.n, vals=vals) == [L.OKKT_ERR_INVALID] * 5
    h._check(h._lib.okkt_set_early_exit(h._h, 0), "okkt_set_early_exit")
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
    assert h.ls_solve(b).tobytes() == x.tobytes()
    finalize_b(h)
    # Schur mode
    h = linear_solver_HIP("symmetric", **ft.NO_RELAX)
    initialize_b(h)
    h.set_schur([0, 1])
    h.analyze(d.A)
    assert h.ls_factor_schur(d.A, d.npos - int(np.sum(np.sign(d.A.diagonal()[[0, 1]]) > 0)), d.nneg - int(np.sum(np.sign(d.A.diagonal()[[0, 1]]) < 0))) in (0, 1)
    assert _all_calls(h, d.n, vals=vals) == [L.OKKT_ERR_INVALID] * 5
    assert "Schur mode" in h._lib.okkt_last_error(h._h).decode()
    assert np.all(np.isfinite(h.schur_condense(b)))
    finalize_b(h)


def test_no_existing_call_changes():
    """okkt_solve after the new calls is bitwise what it was before them"""
    d = ft.build(ft.DESIGNS["edge-k129-c700"][0])
    h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(h)
    h.set_perm(d.perm)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
    B = ft.rhs(d.n, 5)
    X = solve_batch(h, B)
    h.factor_multiply("LDLT", B)
    h.quadform(B)
    h.factor_error(d.A)
    h.ls_solve_forward(B[:3])
    assert solve_batch(h, B).tobytes() == X.tobytes()
    h.ls_solve_backward(B[:2])
    assert solve_batch(h, B).tobytes() == X.tobytes()
    finalize_b(h)
