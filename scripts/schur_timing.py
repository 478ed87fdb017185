"""Schur mode on S-C5: the system bench.py factors for BASELINE config 5 with its 200 linking x-columns as the
Schur set.  Times okkt_factor_schur, the export of S, condense + expand of one right-hand side (device pointers throughout), next to
okkt_factor + okkt_solve of the whole matrix on a second handle; medians of --reps after --warmup, host clock around calls that end in
a device synchronisation.  Writes one JSON object to --out."""
import argparse
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
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="schur_timing.json")
    a = ap.parse_args()
    prob = synth.make_config("S-C5", seed=0)
    K = synth.augmented_matrix(prob, delta=1e-8)
    n, m = prob["n"], prob["m"]
    dim, ns = n + m, 200
    idx = np.arange(n - ns, n)
    vals = np.asarray(K.data, dtype=np.float64)
    b = np.random.default_rng(0).normal(size=dim)

    w = linear_solver_HIP("symmetric")
    initialize_b(w)
    w.analyze(K)
    d_vals = w.dev_upload(vals)
    d_b = w.dev_upload(b)
    d_x = w.dev_alloc(8 * dim)
    assert w.ls_factor_dev(d_vals, n, m) == 1
    res = {"config": "S-C5", "dim": dim, "ns": ns}
    res["whole_factor_ms"] = timed(lambda: w.ls_factor_dev(d_vals, n, m), a.reps, a.warmup)
    res["whole_solve_ms"] = timed(lambda: w.ls_solve_dev(d_b, d_x, 1), a.reps, a.warmup)
    res["whole_stats"] = {k: w.stats()[k] for k in ("nsuper", "nlevels", "max_front", "critical_pivots")}

    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.set_schur(idx)
    h.analyze(K)
    hv = h.dev_upload(vals)
    hb = h.dev_upload(b)
    hx = h.dev_alloc(8 * dim)
    hS = h.dev_alloc(8 * ns * ns)
    hr2 = h.dev_alloc(8 * ns)
    assert h.ls_factor_schur_dev(hv, n - ns, m) == 1
    res["schur_factor_ms"] = timed(lambda: h.ls_factor_schur_dev(hv, n - ns, m), a.reps, a.warmup)
    res["schur_export_ms"] = timed(lambda: h.schur_dev(hS, ns), a.reps, a.warmup)
    S = h.dev_download(hS, (ns, ns))
    r2 = None

    def cond_expand():
        h.schur_condense_dev(hb, hr2, 1)
        h.schur_expand_dev(hb, hr2, hx, 1)      # (x2 = r2 here: the timing does not depend on the values)
    res["schur_condense_expand_ms"] = timed(cond_expand, a.reps, a.warmup)
    h.schur_condense_dev(hb, hr2, 1)
    r2 = h.dev_download(hr2, (ns,))
    x2 = np.linalg.solve(S, r2)
    hx2 = h.dev_upload(x2)
    h.schur_expand_dev(hb, hx2, hx, 1)
    x = h.dev_download(hx, (dim,))
    w.ls_solve_dev(d_b, d_x, 1)
    xw = w.dev_download(d_x, (dim,))
    res["x_rel_diff_vs_whole"] = float(np.max(np.abs(x - xw)) / np.max(np.abs(xw)))
    res["schur_stats"] = {k: h.stats()[k] for k in ("nsuper", "nlevels", "max_front", "critical_pivots")}
    finalize_b(h)
    finalize_b(w)
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
