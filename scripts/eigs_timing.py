"""okkt_eigs on the symmetric KKT factor of S-metric (or --config), the system bench.py factors: nev = 6,
block = 4, the default basis, with nlead = 0 (the eigenvalues of K nearest zero) and nlead = n (those of H + delta I + J' Sigma J),
everything resident on the device (okkt_eigs_dev).  Medians of --reps after --warmup (host clock around calls that end in a device
synchronisation), the sweeps and restarts, the time per sweep next to okkt_solve_dev with four right-hand sides timed in the same
process, and what of a sweep is not the solve: the vector kernels, the host's eigen-solver and the small reads.  Writes one JSON object
to --out.

With --stats CSV (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this script) it instead sums the device time of
the k_eig_* kernels against everything else."""
import argparse
import csv
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def run(config, reps, warmup, nev, block, max_basis, tol):
    prob = synth.make_config(config, seed=0)
    n, m = prob["n"], prob["m"]
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    d_k = h.dev_upload(np.asarray(K.data, dtype=np.float64))
    d_b = h.dev_upload(np.random.default_rng(9).normal(size=4 * (n + m)))
    d_x = h.dev_alloc(8 * 4 * (n + m))
    d_v = h.dev_alloc(8 * nev * (n + m))
    h.ls_factor_dev(d_k, n, m)
    res = {"config": config, "dim": n + m, "n": n, "nev": nev, "block": block, "tol": tol}
    res["solve4_ms"] = timed(lambda: h.ls_solve_dev(d_b, d_x, 4), reps, warmup)
    res["solve1_ms"] = timed(lambda: h.ls_solve_dev(d_b, d_x, 1), reps, warmup)
    for name, nlead in (("standard", 0), ("pencil", n)):
        out = {}

        def call():
            out["lam"], out["resid"], out["info"] = h.eigs_dev(nev, d_k, d_v, block=block, max_basis=max_basis, tol=tol, nlead=nlead)
        t = timed(call, reps, warmup)
        info = out["info"]
        per_sweep = t[0] / max(info["sweeps"], 1)
        res[name] = {"ms": t, "info": info, "lambda": out["lam"].tolist(), "resid": out["resid"].tolist(), "ms_per_sweep": per_sweep,
                     "not_solve_share_of_sweep": 1.0 - res["solve4_ms"][0] / per_sweep}
    for p in (d_k, d_b, d_x, d_v):
        h.dev_free(p)
    finalize_b(h)
    return res


def stats(path):
    eig, rest, per = 0.0, 0.0, {}
    with open(path) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            if "k_eig_" in r["Name"]:
                eig += ns
                short = r["Name"].split("::")[-1].split("(")[0]
                per[short] = per.get(short, 0.0) + ns * 1e-6
            else:
                rest += ns
    return {"k_eig_ms": eig * 1e-6, "other_kernels_ms": rest * 1e-6, "k_eig_share": eig / (eig + rest), "k_eig_ms_by_kernel": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="S-metric")
    ap.add_argument("--nev", type=int, default=6)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--max-basis", type=int, default=0)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--out", default="eigs_timing.json")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    res = stats(a.stats) if a.stats else run(a.config, a.reps, a.warmup, a.nev, a.block, a.max_basis, a.tol)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
