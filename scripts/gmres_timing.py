"""GMRES-based refinement on S-C3 and S-metric, the systems bench.py factors: A = K(1e-8) solved with the
factor of K(1e-8 + delta) for each --deltas value, everything resident on the device (okkt_solve_gmres_dev).  Medians of --reps
after --warmup (host clock around calls that end in a device synchronisation), the outcome (iterations, cycles, solves, omega) and the
plain solve's device time.  Writes one JSON object to --out.

With --trace TRACE (rocprofv3 --kernel-trace output of a run of this script: its kernel_trace.csv or its rocpd .db), it instead
splits the device time of the GMRES calls -- every dispatch from the first residual gather on -- into the solve passes, the double-double residual kernels
(refine.hip) and the new vector kernels (krylov.hip, k_kry_*), per iteration (--iterations: the operator applications the traced
calls made together)."""
import argparse
import csv
import json
import re
import sqlite3
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
    return float(np.median(ts)), float(np.min(ts))


def one(config, delta, reps, warmup, restart):
    prob = synth.make_config(config, seed=0)
    n, m = prob["n"], prob["m"]
    A = synth.augmented_matrix(prob, delta=1e-8)
    F = synth.augmented_matrix(prob, delta=1e-8 + delta)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(F)
    d_f = h.dev_upload(np.asarray(F.data, dtype=np.float64))
    d_a = h.dev_upload(np.asarray(A.data, dtype=np.float64))
    b = np.random.default_rng(9).normal(size=n + m)
    d_b = h.dev_upload(b)
    d_x = h.dev_alloc(8 * (n + m))
    h.ls_factor_dev(d_f, n, m)
    res = {"config": config, "delta": delta, "dim": n + m, "restart": restart}
    res["solve_ms"] = timed(lambda: h.ls_solve_dev(d_b, d_x, 1), reps, warmup)
    res["solve_device_ms"] = h.stats()["last_solve_ms"]
    out = {}

    def run():
        out["info"], out["om"] = h.ls_solve_gmres_dev(d_a, d_b, d_x, 1, restart=restart, max_iters=400)
    res["gmres_ms"] = timed(run, reps, warmup)
    info = out["info"]
    res.update({k: info[k] for k in ("iterations", "cycles", "solves", "status", "omega0", "omega", "work_bytes")})
    res["ms_per_solve_pass"] = res["gmres_ms"][0] / max(info["solves"], 1)
    x = h.dev_download(d_x, (n + m,))
    _, om = h.residual(A, b, x)
    res["omega_check"] = float(om)
    for p in (d_f, d_a, d_b, d_x):
        h.dev_free(p)
    finalize_b(h)
    return res


def split_trace(path, iterations):
    rows = []
    if path.endswith(".db"):          # rocprofv3's default rocpd (SQLite) output
        con = sqlite3.connect(path)
        rows = [(int(s), int(e), str(n)) for s, e, n in con.execute("select start, end, name from kernels")]
        con.close()
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    first = next(i for i, r in enumerate(rows) if "k_gather_vals" in r[2])
    cat = {"solve": 0.0, "residual": 0.0, "krylov": 0.0}
    per = {}
    for s, e, name in rows[first:]:
        k = "krylov" if "k_kry_" in name else ("residual" if ("k_resid" in name or "k_gather" in name or "k_refine_update" in name) else "solve")
        cat[k] += (e - s) * 1e-3
        if k == "krylov":
            mt = re.search(r"k_kry_\w+(<[^>]*>)?", name)
            short = mt.group(0) if mt else name
            per[short] = per.get(short, 0.0) + (e - s) * 1e-3
    total = sum(cat.values())
    return {"iterations": iterations, "dispatches": len(rows) - first, "device_us_total": total,
            "device_us_per_iteration": {k: v / iterations for k, v in cat.items()}, "krylov_share": cat["krylov"] / total,
            "krylov_us_per_iteration_by_kernel": {k: v / iterations for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="S-C3,S-metric")
    ap.add_argument("--deltas", default="1e-12,1e-2,1")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--out", default="gmres_timing.json")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--iterations", type=int, default=0)
    a = ap.parse_args()
    if a.trace:
        r = split_trace(a.trace, a.iterations)
        print(json.dumps(r), flush=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
        return
    out = {"results": []}
    for c in a.configs.split(","):
        for d in a.deltas.split(","):
            r = one(c, float(d), a.reps, a.warmup, a.restart)
            print(json.dumps(r), flush=True)
            out["results"].append(r)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
