"""Helper of test_gpu_kkt_assembly.py (run as a subprocess: OKKT_SCHUR_GROUPS and OKKT_DENSE_DOT are read once per process).
argv: output .npz, mode, design names of kkt_designs.DESIGNS.  mode "q": the Schur kind's matrix only; "full": for the schur,
schur_direct, symmetric and clever_symmetric kinds the matrix of two form_system calls and schur_diag, then (designs with factor = True) one factor
at kkt_designs.shift, System_rhs of a moved current iterate and its direction with the N err.  The test checks the arrays against
kkt_exact."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import kkt_designs as KD  # noqa: E402
from onephase_jl_amd import kkt_system_solver as KS  # noqa: E402

ETA = KS.Class_reduction_factors(0.5, 0.25, 0.375)    # 1 - eta exact: the rhs reference sees the device's factors


def iterate(d, J=None, s=None, y=None, seed=0):
    p = KD.point(d, seed)
    return KS.Class_iterate(x=p["x"], y=d.y if y is None else y, s=d.s if s is None else s, mu=p["mu"], J=d.J if J is None else J, H=d.H,
                            grad=p["grad"], cons=p["cons"], a_norm_penalty_par=1e-4)


def run(d, kind, res, tag, full, last=0.0, grad_nan=False):
    opts = {"schur_dense_rows": d.dense} if kind in ("schur", "schur_direct") and d.dense else {}
    k = KS.HIP_KKT_solver(kind, **opts)
    it = iterate(d)
    k.initialize_b(it)
    k.form_system_b(it)
    A = k.matrix()
    res.update({f"{tag}/Ap": A.indptr, f"{tag}/Ai": A.indices, f"{tag}/Ax": A.data, f"{tag}/sd": k.schur_diag.copy(),
                f"{tag}/drows": k.dense_rows()})
    if full:
        k.form_system_b(it)
        res[f"{tag}/Ax2"] = k.matrix().data
    if full and d.factor:
        res[f"{tag}/flag"] = np.array(k.factor_b(KD.shift(d)))
        J2, s2, y2 = KD.moved(d, last=last)
        cur = iterate(d, J2, s2, y2)
        if grad_nan:
            cur.grad = cur.grad.copy(); cur.grad[len(cur.grad) // 2] = np.nan
        k.kkt_associate_rhs_b(cur, ETA)
        try:
            k.compute_direction_b()
        except KS.OkktError:
            if not grad_nan:
                raise
        e = k.kkt_err_norm
        res.update({f"{tag}/rD": k.rhs.dual_r, f"{tag}/rP": k.rhs.primal_r, f"{tag}/rC": k.rhs.comp_r, f"{tag}/dx": k.dir.x, f"{tag}/dy": k.dir.y,
                    f"{tag}/ds": k.dir.s, f"{tag}/err": np.array([e.error_D, e.error_P, e.error_mu, e.overall, e.rhs_norm, e.ratio])})
    k.finalize_b()


out, mode, names = sys.argv[1], sys.argv[2], sys.argv[3:]
res = {}
for name in names:
    if name.startswith("special:"):
        # special:<kind>:<design>:<last>:<grad_nan>
        _, kind, dn, last, gn = name.split(":")
        run(KD.DESIGNS[dn], kind, res, name, True, last=float(last), grad_nan=gn == "1")
        continue
    d = KD.DESIGNS[name]
    print(f"okkt-case: design {name}", file=sys.stderr, flush=True)
    for kind in (("schur",) if mode == "q" else ("schur", "schur_direct", "symmetric", "clever_symmetric")):
        run(d, kind, res, f"{name}/{kind}", mode == "full")
np.savez(out, **res)
print("CASE_OK", json.dumps(len(res)))
