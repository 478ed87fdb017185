"""What the Lanczos bound of the delta loop costs and saves, on the S-metric KKT instance of synth with the
diagonal of H shifted so that lambda_min(H + J' Sigma J) is about -1.  The shift comes from a bisection on the inertia flag of
okkt_kkt_factor (Q(0) - t I is positive definite exactly for t < lambda_min), to a relative 1e-4: no eigenvalue estimate is involved.

Per kind (symmetric, schur), in one process: okkt_kkt_ipopt_strategy, okkt_kkt_ipopt_strategy_eig and okkt_kkt_ipopt_strategy_eig with
scaled = 1 on three handles, alternating, the order rotated from round to round, --pairs rounds after one untimed round.  Every timed
loop starts from a fresh form_system.
One JSON line per record: the strategy, wall milliseconds of the loop, #fac, skipped, the Lanczos steps and its seconds_device.  The
yardstick from the same run: the device time of one okkt_kkt_factor_trial at delta = 0 (a failed, early-exited attempt) and of one
complete factorisation at the delta the loop returned.

Last, on the same pattern with sigma spread log-uniformly over 1e-8 .. 1e8: the steps the unscaled and the scaled mode take at the
default tolerance (what a later change of hip_delta_eig_scaled's default would go by).

    python scripts/delta_eig_timing.py [--config S-metric] [--steps 32] [--pairs 5] [--out profiles/delta_eig_timing.jsonl]
"""
import argparse
import json
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, ".")
from onephase_jl_amd import synth
from onephase_jl_amd import kkt_system_solver as KS


def iterate(prob, H):
    n, m = prob["n"], prob["m"]
    rng = np.random.default_rng(1)
    return KS.Class_iterate(x=rng.normal(size=n), y=prob["y"], s=prob["s"], mu=float(prob["mu"]), J=prob["J"], H=H,
                            grad=rng.normal(size=n), cons=prob["s"] + 1e-3 * rng.normal(size=m))


def solver(kind, it, **opts):
    pars = KS.Class_parameters()
    pars.kkt.kkt_solver_type = kind
    k = KS.HIP_KKT_solver(kind, pars, **opts)
    k.initialize_b(it)
    k.form_system_b(it)
    return k


def shifted_to_minus_one(prob):
    """H with its diagonal moved so that lambda_min(Q(0)) lands on -1 (to 1e-4 of the shift); (H, lambda_min before the shift).
    Q(0) of the synth instances is positive definite with a positive diagonal: lambda_min lies in (0, min diag]."""
    k = solver("schur", iterate(prob, prob["H"]))
    lo, hi = 0.0, k.diag_min()
    assert k.factor_b(0.0) == 1 and hi > 0.0
    while hi - lo > 1e-4 * hi:
        mid = 0.5 * (lo + hi)
        if k.factor_b(-mid) == 1:
            lo = mid
        else:
            hi = mid
    k.finalize_b()
    lam = 0.5 * (lo + hi)
    H = (prob["H"] - sp.diags(np.full(prob["n"], lam + 1.0), format="csc")).tocsc()
    H.sort_indices()
    return H, lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="S-metric")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--kinds", default="symmetric,schur")
    ap.add_argument("--create-order", default="0,1,2", help="the order in which the three handles of a kind are created")
    ap.add_argument("--out", default="profiles/delta_eig_timing.jsonl")
    a = ap.parse_args()
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    prob = synth.make_config(a.config, seed=0)
    H, lam0 = shifted_to_minus_one(prob)
    sig = prob["y"] / prob["s"]
    emit({"record": "instance", "config": a.config, "n": prob["n"], "m": prob["m"], "nnzJ": int(prob["J"].nnz), "nnzH": int(H.nnz),
          "lambda_min_before_shift": lam0, "sigma_min": float(sig.min()), "sigma_max": float(sig.max())})
    it = iterate(prob, H)
    for kind in a.kinds.split(","):
        make = {"ipopt_strategy": {}, "ipopt_strategy_eig": dict(hip_delta_eig_steps=a.steps, hip_delta_eig_scaled=0),
                "ipopt_strategy_eig_scaled": dict(hip_delta_eig_steps=a.steps, hip_delta_eig_scaled=1)}
        made = {name: solver(kind, it, **make[name]) for name in [list(make)[int(i)] for i in a.create_order.split(",")]}
        ks = {name: made[name] for name in make}
        for pair in range(-1, a.pairs):                      # pair -1: untimed (analysis done, modules loaded, workspaces allocated)
            order = list(ks)[pair % 3:] + list(ks)[: pair % 3]
            for name in order:
                k = ks[name]
                k.form_system_b(it)
                t0 = time.perf_counter()
                status, nfac, delta = k.ipopt_strategy_b(it)
                wall = 1e3 * (time.perf_counter() - t0)
                if pair < 0:
                    continue
                e = k.delta_eig_info or {}
                emit({"record": "loop", "kind": kind, "strategy": name, "pair": pair, "wall_ms": wall, "status": status, "num_fac": nfac,
                      "skipped": k.skipped, "delta": delta, "lanczos_steps": e.get("steps"), "lanczos_status": e.get("status"),
                      "lanczos_device_ms": None if not e else 1e3 * e["seconds_device"], "rho": e.get("rho"), "rho_margin": e.get("rho_margin")})
        # the yardstick on the first handle: one failed trial at delta = 0, one complete factorisation at the returned delta
        k = ks["ipopt_strategy"]
        trial, full = [], []
        for _ in range(a.pairs):
            k.form_system_b(it)
            flag = k.factor_b(0.0, trial=True)
            trial.append(k.timers()["factor_ms"])
            k.factor_b(delta)
            full.append(k.timers()["factor_ms"])
        emit({"record": "yardstick", "kind": kind, "trial_flag_at_0": flag, "failed_trial_device_ms": trial, "complete_factor_device_ms": full})
        # the estimate alone, repeated: its device time when it runs to the step limit (a tolerance it cannot meet) and at the default one
        k.form_system_b(it)
        for scaled in (0, 1):
            for tol in (1e-300, 0.0):
                alone = [k.min_eig(a.steps, tol, scaled, with_vector=False)[0] for _ in range(a.pairs + 1)][1:]
                emit({"record": "min_eig", "kind": kind, "max_steps": a.steps, "scaled": scaled, "tol": tol, "steps": [e["steps"] for e in alone],
                      "status": [e["status"] for e in alone], "device_ms": [1e3 * e["seconds_device"] for e in alone], "rho": alone[-1]["rho"],
                      "rho_margin": alone[-1]["rho_margin"], "theta_min": alone[-1]["theta_min"], "bound": alone[-1]["bound"]})
        for k in ks.values():
            k.finalize_b()
    # sigma over sixteen decades: steps of the two modes at the default tolerance
    rng = np.random.default_rng(2)
    wide = dict(prob)
    wide["s"] = np.ones(prob["m"])
    wide["y"] = 10.0 ** rng.uniform(-8.0, 8.0, size=prob["m"])
    Hw, lamw = shifted_to_minus_one(wide)
    k = solver("symmetric", iterate(wide, Hw))
    for scaled in (0, 1):
        for steps in (32, 64):
            e, _ = k.min_eig(steps, 0.0, scaled, with_vector=False)
            emit({"record": "sigma_spread", "scaled": scaled, "max_steps": steps, "steps": e["steps"], "status": e["status"], "theta_min": e["theta_min"],
                  "bound": e["bound"], "rho": e["rho"], "rho_margin": e["rho_margin"], "resid": e["resid"], "device_ms": 1e3 * e["seconds_device"],
                  "lambda_min_before_shift": lamw})
    k.finalize_b()
    with open(a.out, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
