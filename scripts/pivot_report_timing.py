"""Device time of the threshold pivot report next to a one-right-hand-side solve on the same handle, on S-C3 and
S-metric, the systems bench.py factors.  Per configuration: --warmup untimed rounds, then --reps rounds of one factorisation (so that
the report scans again), one okkt_pivot_report (seconds_device: HIP events around the scan) and one okkt_solve_dev (last_solve_ms: HIP
events around the sweeps); medians, minima and maxima of both, the report's counts at u = 1e-8, and the entries of L the scan reads
with the bandwidth that follows from them.  Writes one JSON object to --out (profiles/<tag>_pivot_report_timing.json).

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/pivot_report_timing.py ...` in a run
of its own (the scan's kernels are k_pv_small, k_pv_big, k_pv_merge, k_pv_fill, k_pv_count)."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def one(config, reps, warmup):
    prob = synth.make_config(config, seed=0)
    n, m = prob["n"], prob["m"]
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    d_k = h.dev_upload(np.asarray(K.data, dtype=np.float64))
    d_b = h.dev_upload(np.random.default_rng(9).normal(size=n + m))
    d_x = h.dev_alloc(8 * (n + m))
    rep_ms, solve_ms, factor_ms = [], [], []
    rep = None
    for it in range(warmup + reps):
        flag = h.ls_factor_dev(d_k, n, m)
        rep = h.pivot_report(1e-8)
        h.ls_solve_dev(d_b, d_x, 1)
        st = h.stats()
        if it >= warmup:
            rep_ms.append(rep["seconds_device"] * 1e3)
            solve_ms.append(st["last_solve_ms"])
            factor_ms.append(st["last_factor_ms"])
    st = h.stats()
    entries = int(st["nnzL_stored"] - st["n"])
    res = {"config": config, "dim": n + m, "flag": flag, "reps": reps, "warmup": warmup, "entries_of_L": entries,
           "n_small_fronts": int(st["n_small_fronts"]), "n_big_fronts": int(st["n_big_fronts"]), "max_front": int(st["max_front"]),
           "report_device_ms": stats(rep_ms), "solve_device_ms": stats(solve_ms), "factor_device_ms": stats(factor_ms),
           "report_over_solve": float(np.median(rep_ms) / np.median(solve_ms)),
           "scan_GB_per_s": float(8.0 * entries / (np.median(rep_ms) * 1e-3) / 1e9),
           "rejected": int(rep["rejected"]), "nonfinite_cols": int(rep["nonfinite_cols"]), "max_multiplier": float(rep["max_multiplier"])}
    for p in (d_k, d_b, d_x):
        h.dev_free(p)
    finalize_b(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="S-C3,S-metric")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/r10_pivot_report_timing.json")
    a = ap.parse_args()
    out = {"what": "okkt_pivot_report seconds_device next to last_solve_ms of a one-right-hand-side solve, HIP events, medians of reps",
           "results": [one(c, a.reps, a.warmup) for c in a.configs.split(",")]}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
