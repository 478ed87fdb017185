"""Helper of test_gpu_kkt_clever.py (run as a subprocess).  argv: output .npz, design names of kkt_designs.CLEVER_DESIGNS.  Per design
and per rescale mode of the clever-symmetric kind: the grouping, U, g and D of form_system; the matrix after form_system, after a
second form_system, after factor! with delta = kkt_designs.shift, 0, a negative delta and the shift again; then System_rhs of a moved
current iterate, its direction, the intermediate vectors of okkt_kkt_get_clever_vectors and the N err.  Per design also the symmetric
kind's direction (its solve refined) for the same iterates and delta.  The test checks the arrays against kkt_exact."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import kkt_designs as KD  # noqa: E402
from onephase_jl_amd import kkt_system_solver as KS  # noqa: E402

ETA = KS.Class_reduction_factors(0.5, 0.25, 0.375)
NEG_DELTA = -0.375


def iterate(d, J=None, s=None, y=None):
    p = KD.point(d)
    return KS.Class_iterate(x=p["x"], y=d.y if y is None else y, s=d.s if s is None else s, mu=p["mu"], J=d.J if J is None else J, H=d.H,
                            grad=p["grad"], cons=p["cons"], a_norm_penalty_par=1e-4)


def factor(k, delta, may_refuse):
    """(flag, inertia, matrix values) of factor!(delta).  may_refuse (delta = 0 and the negative delta, where the matrix is singular
    or indefinite by design): a refused factorisation is recorded as flag -99 and the matrix is still read."""
    try:
        flag, inertia = k.factor_b(delta), k.inertia
    except KS.OkktError:
        if not may_refuse:
            raise
        flag, inertia = -99, (-1, -1, -1, -1)
    return np.array([flag] + [int(v) for v in inertia]), k.matrix().data


def direction(k, d, res, tag):
    J2, s2, y2 = KD.moved(d)
    k.kkt_associate_rhs_b(iterate(d, J2, s2, y2), ETA)
    k.compute_direction_b()
    e = k.kkt_err_norm
    res.update({f"{tag}/rD": k.rhs.dual_r, f"{tag}/rP": k.rhs.primal_r, f"{tag}/rC": k.rhs.comp_r, f"{tag}/dx": k.dir.x, f"{tag}/dy": k.dir.y,
                f"{tag}/ds": k.dir.s, f"{tag}/err": np.array([e.error_D, e.error_P, e.error_mu, e.overall, e.rhs_norm, e.ratio])})


def run(d, rescale, res, tag):
    pars = KS.Class_parameters()
    pars.kkt.kkt_solver_type = "clever_symmetric"
    pars.kkt.kkt_system_rescale = rescale
    k = KS.pick_KKT_solver(pars)
    it = iterate(d)
    k.initialize_b(it)
    k.form_system_b(it)
    A = k.matrix()
    first, info = k.get_indicies(with_values=True)
    g = np.full(d.m, np.nan)
    for grp in info:
        for row in grp["ls"]:
            g[row["ind"]] = row["g"]
    res.update({f"{tag}/first": np.array(first, np.int64), f"{tag}/gptr": np.cumsum([0] + [len(grp["ls"]) for grp in info]),
                f"{tag}/mind": np.array([r["ind"] for grp in info for r in grp["ls"]], np.int64),
                f"{tag}/mratio": np.array([r["ratio"] for grp in info for r in grp["ls"]]),
                f"{tag}/mu": np.array([r["u"] for grp in info for r in grp["ls"]]),
                f"{tag}/gU": np.array([grp["u"] for grp in info]), f"{tag}/g": g, f"{tag}/D": k.clever_vectors(direction=False)["D"],
                f"{tag}/Ap": A.indptr, f"{tag}/Ai": A.indices, f"{tag}/Ax": A.data, f"{tag}/sd": k.schur_diag.copy()})
    k.form_system_b(it)
    res[f"{tag}/Ax2"] = k.matrix().data
    for name, delta in (("s", KD.shift(d)), ("0", 0.0), ("n", NEG_DELTA), ("s2", KD.shift(d))):
        res[f"{tag}/flag_{name}"], res[f"{tag}/Ax_{name}"] = factor(k, delta, may_refuse=name in ("0", "n"))
    direction(k, d, res, tag)
    v = k.clever_vectors()
    res.update({f"{tag}/{key}": v[key] for key in ("symrhs", "crhs", "sol", "v")})
    res[f"{tag}/D_after"] = v["D"]
    res[f"{tag}/n_analyze"] = np.array(k.linear_solver_stats()["n_analyze_calls"])
    res[f"{tag}/perm"] = k.linear_solver_perm()
    k.finalize_b()


out, names = sys.argv[1], sys.argv[2:]
res = {}
for name in names:
    d = KD.CLEVER_DESIGNS[name]
    print(f"okkt-case: clever design {name}", file=sys.stderr, flush=True)
    for rescale in KD.RESCALES:
        run(d, rescale, res, f"{name}/{rescale}")
    k = KS.HIP_KKT_solver("symmetric", hip_ls_refine_steps=3)
    it = iterate(d)
    k.initialize_b(it)
    k.form_system_b(it)
    res[f"{name}/symmetric/flag"] = np.array(k.factor_b(KD.shift(d)))
    direction(k, d, res, f"{name}/symmetric")
    k.finalize_b()
np.savez(out, **res)
print("CASE_OK", json.dumps(len(res)))
