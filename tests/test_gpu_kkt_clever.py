"""GPU tests: the clever-symmetric kind of the KKT layer (csrc/kkt.hip: k_clever_groups, k_clever_rescale, k_clever_assemble,
k_clever_true_diag, k_clever_xdiag, k_clever_symrhs, k_clever_crhs, k_clever_rhs, k_clever_res, k_clever_unscale, k_clever_y and the
host index work of okkt_kkt_compute_indicies) on designs with designed groups of parallel rows (kkt_designs.CLEVER_DESIGNS), in the
three rescale modes: the grouping equals the designed one and the oracle's, the pattern of M, every value of U, g, D, Q = D M D, the x
diagonal under delta = shift, 0 and a negative delta, System_rhs, symrhs, crhs, the unscaling, dy, ds and the N err within the
rounding bound of its exact value (tests/kkt_exact.py); the direction's forward error against the refined solution of the full KKT
system, measured against the oracle's Clever_Symmetric_KKT_solver on the device's permutation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import front_trees as FT
import kkt_designs as KD
import kkt_exact as KE
import oracle
from oracle import kkt_oracle as KO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD = KD.CLEVER_DESIGNS
ALL = list(CD)
ETA = (0.5, 0.25, 0.375)
SINGLETONS = ["b8", "b64", "jc64_tiny"]
U = 2.0 ** -53
assert_within = KE.assert_within

# e_hip / e_oracle of test_forward_error_against_the_full_system as measured on an MI355X (the CLEVER lines of a run regenerate it).
FWD_RATIO = {
    ("cg_mix", "none"): 0.069, ("cg_mix", "u_only"): 0.14, ("cg_mix", "u_and_x"): 1.0,
    ("cg_big", "none"): 0.02, ("cg_big", "u_only"): 0.018, ("cg_big", "u_and_x"): 1.0,
    ("cg_h0", "none"): 0.026, ("cg_h0", "u_only"): 0.034, ("cg_h0", "u_and_x"): 1.0,
    ("cg_n1m2", "none"): 1.3, ("cg_n1m2", "u_only"): 0.9, ("cg_n1m2", "u_and_x"): 1.0,
    ("b8", "none"): 0.02, ("b8", "u_only"): 0.02, ("b8", "u_and_x"): 1.0,
    ("b64", "none"): 0.055, ("b64", "u_only"): 0.061, ("b64", "u_and_x"): 1.0,
    ("jc64_tiny", "none"): 0.053, ("jc64_tiny", "u_only"): 0.018, ("jc64_tiny", "u_and_x"): 1.0,
    ("m0", "none"): 0.04, ("m0", "u_only"): 0.04, ("m0", "u_and_x"): 1.0,
}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kkt_clever") / "case.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kkt_clever_case.py"), out] + ALL, cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "CASE_OK" in r.stdout, (r.stdout[-400:], r.stderr[-2000:])
    return dict(np.load(out))


def groups_of(case, tag):
    p, ind, rat = case[f"{tag}/gptr"], case[f"{tag}/mind"], case[f"{tag}/mratio"]
    return [([int(j) for j in ind[p[g]:p[g + 1]]], [float(r) for r in rat[p[g]:p[g + 1]]]) for g in range(len(p) - 1)]


def mat(case, tag, which="Ax"):
    p = case[f"{tag}/Ap"]
    return sp.csc_matrix((case[f"{tag}/{which}"], case[f"{tag}/Ai"], p), shape=(len(p) - 1, len(p) - 1))


cases = pytest.mark.parametrize("rescale", KD.RESCALES)
designs = pytest.mark.parametrize("name", ALL)


# ---- 1. the grouping -----------------------------------------------------------------------------------------------------------------
@cases
@designs
def test_grouping_is_the_designed_one_and_the_oracles(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    got = groups_of(case, tag)
    assert got == d.groups
    first, ogroups = KO.compute_indicies(d.J)
    assert [int(v) for v in case[f"{tag}/first"]] == first == [mem[0] for mem, _ in got]
    assert got == [([r.ind for r in g.ls], [r.ratio for r in g.ls]) for g in ogroups]
    # every row in exactly one group (row_grp / row_ratio have no default to fall back on); member u = fl(s / y)
    assert sorted(j for mem, _ in got for j in mem) == list(range(d.m))
    assert np.array_equal(case[f"{tag}/mu"], (d.s / d.y)[case[f"{tag}/mind"]])


# ---- 2. the pattern of M, one analysis -----------------------------------------------------------------------------------------------
@cases
@designs
def test_pattern_of_m_and_one_analysis(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    ptr, idx = KE.clever_pattern(d.H, d.J, case[f"{tag}/first"])
    assert np.array_equal(case[f"{tag}/Ap"], ptr) and np.array_equal(case[f"{tag}/Ai"], idx)
    assert int(case[f"{tag}/n_analyze"]) == 1                 # two form_system, four factor!, one direction


# ---- 3. U, g, D, Q, the x diagonal, schur_diag -----------------------------------------------------------------------------------
@cases
@designs
def test_u_g_d_exact(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    rU, rg = KE.clever_u_g_ratios(d.groups, d.s / d.y, case[f"{tag}/gU"], case[f"{tag}/g"])
    assert_within(rU, (tag, "U"))
    assert_within(rg, (tag, "g"))
    p = KD.point(d)
    xinf = float(np.max(np.abs(p["x"]))) if d.n else 0.0
    assert_within(KE.clever_d_ratios(rescale, p["mu"], xinf, d.n, case[f"{tag}/gU"], case[f"{tag}/D"]), (tag, "D"))
    assert np.array_equal(case[f"{tag}/D_after"], case[f"{tag}/D"])
    assert_within(KE.diag_ratios(case[f"{tag}/sd"], d.H, d.J, d.y / d.s), (tag, "schur_diag"))


@cases
@designs
def test_matrix_exact_under_every_delta(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    args = (d.H, d.J, case[f"{tag}/first"], case[f"{tag}/gU"], case[f"{tag}/D"])
    assert_within(KE.clever_q_ratios(mat(case, tag), *args, "scaled"), (tag, "Q"))
    assert np.array_equal(case[f"{tag}/Ax2"], case[f"{tag}/Ax"])            # a second form_system: the same bits
    assert_within(KE.clever_q_ratios(mat(case, tag, "Ax_s"), *args, "true"), (tag, "Q, delta = shift"))
    assert_within(KE.clever_q_ratios(mat(case, tag, "Ax_0"), *args, "scaled"), (tag, "Q, delta = 0"))
    assert_within(KE.clever_q_ratios(mat(case, tag, "Ax_n"), *args, "true"), (tag, "Q, delta < 0"))
    # shift -> 0 -> negative -> shift on one formed system: every diagonal restored, nothing else touched
    assert np.array_equal(case[f"{tag}/Ax_s2"], case[f"{tag}/Ax_s"])
    assert np.array_equal(case[f"{tag}/Ax_0"], case[f"{tag}/Ax"])
    off = np.ones(len(case[f"{tag}/Ax"]), bool)
    A = mat(case, tag)
    for j in range(d.n):
        off[A.indptr[j] + list(A.indices[A.indptr[j]:A.indptr[j + 1]]).index(j)] = False
    for which in ("Ax_s", "Ax_n"):
        assert np.array_equal(case[f"{tag}/{which}"][off], case[f"{tag}/Ax"][off])


# ---- 4. System_rhs ---------------------------------------------------------------------------------------------------------------
def current_iterate(d):
    J2, s2, y2 = KD.moved(d)
    p = KD.point(d)
    return J2, s2, y2, p["grad"], p["cons"], p["mu"], 1e-4


@cases
@designs
def test_system_rhs_exact(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    J2, s2, y2, grad, cons, mu, pen = current_iterate(d)
    for r, what in zip(KE.rhs_ratios(J2, grad, cons, s2, y2, mu, pen, ETA, case[f"{tag}/rD"], case[f"{tag}/rP"], case[f"{tag}/rC"]),
                       ("dual_r", "primal_r", "comp_r")):
        assert_within(r, (tag, what))


# ---- 5. the direction's vector kernels -----------------------------------------------------------------------------------------------
@cases
@designs
def test_direction_vectors_exact(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    c = {k: case[f"{tag}/{k}"] for k in ("rP", "rC", "symrhs", "crhs", "sol", "v", "dx", "dy", "ds", "g", "gU", "D")}
    assert_within(KE.clever_symrhs_ratios(c["rP"], c["rC"], d.y, c["symrhs"]), (tag, "symrhs"))
    assert_within(KE.clever_crhs_ratios(d.groups, c["g"], c["symrhs"], c["crhs"]), (tag, "crhs"))
    assert_within(KE.clever_unscale_ratios(c["sol"], c["D"], d.n, c["dx"], c["v"]), (tag, "dx, v"))
    assert_within(KE.clever_dy_ratios(d.groups, d.s / d.y, c["symrhs"], c["crhs"], c["gU"], c["v"], c["dy"]), (tag, "dy"))
    assert_within(KE.ds_ratios(d.J, c["dx"], c["rP"], c["ds"]), (tag, "ds"))


# ---- 6. N err ------------------------------------------------------------------------------------------------------------------------
@cases
@designs
def test_kkt_error_exact(case, name, rescale):
    KE.check_err(case, CD[name], f"{name}/{rescale}", KD.shift(CD[name]))


# ---- 7. inertia ----------------------------------------------------------------------------------------------------------------------
@cases
@designs
def test_inertia_at_the_shift(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    for which in ("flag_s", "flag_s2"):
        assert [int(v) for v in case[f"{tag}/{which}"]] == [1, d.n, d.m_new, 0, 0], (tag, which)


# ---- 8. forward error against the full system ----------------------------------------------------------------------------------------
def block_err(x, xt):
    return float(np.max(np.abs(x - xt)) / np.max(np.abs(xt))) if len(xt) and np.max(np.abs(xt)) > 0 else 0.0


def true_direction(d, rD, rP, rC):
    """(dx, dy) of [[H + delta I, J']; [J, -diag(s / y)]] (dx, -dy) = (rD, rP + rC / y) at the factor iterate, delta = shift(d): the
    oracle's solve refined with long-double residuals."""
    n, m = d.n, d.m
    Hs = (d.H + sp.tril(d.H, -1).T + KD.shift(d) * sp.identity(n)).tocsc()
    K = sp.bmat([[Hs, d.J.T], [d.J, -sp.diags(d.s / d.y)]], format="csr") if m else sp.csr_matrix(Hs)
    K.sort_indices()
    ls = oracle.linear_solver_ORACLE("symmetric")
    assert ls.ls_factor_b(sp.tril(K).tocsc(), n, m) == 1
    x = FT.true_solution(K, ls.ls_solve, np.concatenate([rD, rP + rC / d.y]))
    return x[:n], -x[n:]


def fwd_errors(case, name, rescale):
    d, tag = CD[name], f"{name}/{rescale}"
    rD, rP, rC = (case[f"{tag}/{k}"] for k in ("rD", "rP", "rC"))
    tx, ty = true_direction(d, rD, rP, rC)
    p = KD.point(d)
    J2, s2, y2 = KD.moved(d)
    ko = KO.pick_KKT_solver("clever_symmetric", perm=case[f"{tag}/perm"])
    ko.kkt_system_rescale = rescale
    it = KO.Iterate(x=p["x"], y=d.y, s=d.s, mu=p["mu"], J=d.J, H=d.H, grad=p["grad"], cons=p["cons"])
    ko.initialize_b(it)
    ko.form_system_b(it)
    assert ko.factor_b(KD.shift(d)) == 1
    ko.kkt_associate_rhs_b(KO.Iterate(x=p["x"], y=y2, s=s2, mu=p["mu"], J=J2, H=d.H, grad=p["grad"], cons=p["cons"]), KO.Class_reduction_factors(*ETA))
    ko.rhs = KO.System_rhs(rD, rP, rC)              # the device's right-hand side, bit for bit
    ko.compute_direction_b()
    e_hip = max(block_err(case[f"{tag}/dx"], tx), block_err(case[f"{tag}/dy"], ty))
    e_or = max(block_err(ko.dir.x, tx), block_err(ko.dir.y, ty))
    return e_hip, e_or, (d.n + d.m_new) * U


@cases
@designs
def test_forward_error_against_the_full_system(case, name, rescale):
    """e_hip <= 2 max(1, r) max(e_oracle, (n + m_new) u): r the ratio measured on the MI355X (FWD_RATIO), 2 the run-to-run and
    box-to-box allowance, the floor keeps two errors at rounding level from being compared with each other.  Under u_and_x the
    reference keeps the UNscaled x diagonal in the scaled system when delta != 0 (clever_symmetric.jl:494-519), so its direction --
    the device's and the oracle's alike -- solves a perturbed system: both errors are then far above rounding and the check holds the
    device to the oracle's."""
    e_hip, e_or, floor = fwd_errors(case, name, rescale)
    ratio = e_hip / max(e_or, floor)
    print("CLEVER " + json.dumps(dict(name=name, rescale=rescale, e_hip=e_hip, e_oracle=e_or, floor=floor, ratio=ratio)))
    assert e_hip <= 2.0 * max(1.0, FWD_RATIO[(name, rescale)]) * max(e_or, floor), (name, rescale, e_hip, e_or)


# ---- 9. two routes to one direction ----------------------------------------------------------------------------------------------
@cases
@pytest.mark.parametrize("name", SINGLETONS)
def test_singleton_designs_agree_with_the_symmetric_kind(case, name, rescale):
    """No two non-empty rows parallel: M is K with the empty rows merged, and the clever and the symmetric kind (its solve refined, as
    the clever kind's is) reach the direction of the same full system by independent routes: dx and dy agree, block by block, to the
    bound of test_forward_error_against_the_full_system; ds = J dx - rP row by row to |J| times that difference of dx plus the
    rounding of the two row products."""
    d, tag = CD[name], f"{name}/{rescale}"
    assert int(case[f"{name}/symmetric/flag"]) == 1
    for k in ("rD", "rP", "rC"):
        assert np.array_equal(case[f"{tag}/{k}"], case[f"{name}/symmetric/{k}"])
    e_hip, e_or, floor = fwd_errors(case, name, rescale)
    bound = 2.0 * max(1.0, FWD_RATIO[(name, rescale)]) * max(e_or, floor)
    for k in ("dx", "dy"):
        a, b = case[f"{tag}/{k}"], case[f"{name}/symmetric/{k}"]
        assert block_err(a, b) <= bound, (tag, k, block_err(a, b), bound)
    dxs = case[f"{name}/symmetric/dx"]
    aJ = abs(d.J).tocsr()
    kmax = int(np.diff(aJ.indptr).max())
    lim = (aJ @ np.ones(d.n)) * bound * np.max(np.abs(dxs)) + 2.0 * KE.gamma(kmax + 1) * (aJ @ np.abs(dxs) + np.abs(case[f"{tag}/rP"]))
    assert np.all(np.abs(case[f"{tag}/ds"] - case[f"{name}/symmetric/ds"]) <= lim), (tag, "ds")


# ---- the accessor of the intermediates ---------------------------------------------------------------------------------------------
def test_clever_vectors_refuses_other_kinds_and_the_wrong_state():
    from onephase_jl_amd import kkt_system_solver as KS
    d = CD["cg_h0"]
    p = KD.point(d)
    it = KS.Class_iterate(x=p["x"], y=d.y, s=d.s, mu=p["mu"], J=d.J, H=d.H, grad=p["grad"], cons=p["cons"])
    k = KS.HIP_KKT_solver("symmetric")
    k.initialize_b(it)
    k.form_system_b(it)
    with pytest.raises(KS.OkktError, match="clever-symmetric solver only"):
        k.clever_vectors(direction=False)
    k.finalize_b()
    k = KS.HIP_KKT_solver("clever_symmetric")
    k.initialize_b(it)
    with pytest.raises(KS.OkktError, match="after form_system"):
        k.clever_vectors(direction=False)
    k.form_system_b(it)
    assert np.array_equal(k.clever_vectors(direction=False)["D"], np.ones(d.n + d.m_new))
    assert k.factor_b(KD.shift(d)) == 1
    with pytest.raises(KS.OkktError, match="no direction"):
        k.clever_vectors()
    k.kkt_associate_rhs_b(it, KS.Reduct_affine())
    k.compute_direction_b()
    v = k.clever_vectors()
    assert np.array_equal(v["sol"][: d.n], k.dir.x)             # rescale none: D = 1
    k.kkt_associate_rhs_b(it, KS.Reduct_stable())               # System_rhs overwrites the scratch symrhs lived in
    with pytest.raises(KS.OkktError, match="no direction"):
        k.clever_vectors()
    k.compute_direction_b()
    k.clever_vectors()
    assert k.factor_b(KD.shift(d)) == 1                         # a further factor!: the vectors belong to the old factorisation
    with pytest.raises(KS.OkktError, match="no direction"):
        k.clever_vectors()
    assert len(k.clever_vectors(direction=False)["D"]) == d.n + d.m_new
    k.finalize_b()
