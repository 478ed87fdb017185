"""Device time of the sparse right-hand-side solves next to a one-column okkt_solve_dev on the same factor, on
S-C3 and S-metric, the systems bench.py factors.  Per configuration and case: --warmup untimed calls, then --reps calls; medians, minima
and maxima of the device time (HIP events around the enqueued work: last_solve_ms / okkt_sparse_info.seconds_device) and of the host's
wall clock around the whole call (it holds the reach, the list copy and the wait), with the info's counts and panel bytes beside them.

Cases: one non-zero in a leaf (the first column of the factor order), one in the root's pivot block (the last column), both with every
entry of x and with that one entry wanted; 16 random non-zeros with 16 random wanted rows; inverse_block of 64 random indices (16 groups
of four unit columns).  Writes one JSON object to --out (profiles/sparse_solve_timing.json)."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

KEYS = ["nsuper", "fwd_reach", "bwd_reach", "fwd_run", "bwd_run", "fringe", "fringe_entries", "fwd_panel_bytes", "bwd_panel_bytes",
        "factor_panel_bytes", "batches", "pruned"]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(call, reps, warmup):
    dev, wall, info = [], [], None
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        ms, info = call()
        t1 = time.perf_counter()
        if it >= warmup:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    out = {"device_ms": stats(dev), "wall_ms": stats(wall)}
    if info is not None:
        out["info"] = {k: int(info[k]) for k in KEYS}
    return out


def one(config, reps, warmup):
    prob = synth.make_config(config, seed=0)
    n, m = prob["n"], prob["m"]
    dim = n + m
    K = synth.augmented_matrix(prob, delta=1e-8)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    d_k = h.dev_upload(np.asarray(K.data, dtype=np.float64))
    flag = h.ls_factor_dev(d_k, n, m)
    perm = h.perm()
    rng = np.random.default_rng(11)
    d_b = h.dev_upload(rng.normal(size=dim))
    d_x = h.dev_alloc(8 * dim)
    d_v = h.dev_upload(rng.normal(size=64))
    d_o = h.dev_alloc(8 * 64 * 64)
    res = {"config": config, "dim": dim, "flag": flag, "reps": reps, "warmup": warmup, "cases": {}}

    def dense():
        h.ls_solve_dev(d_b, d_x, 1)
        return h.stats()["last_solve_ms"], None

    def sparse(rows, want):
        def call():
            info = h.ls_solve_sparse_dev([0, len(rows)], rows, d_v, d_x if want is None else d_o, want)
            return info["seconds_device"] * 1e3, info
        return call

    def block(idx):
        def call():
            info = h.inverse_columns_dev(idx, d_o, idx)
            return info["seconds_device"] * 1e3, info
        return call

    leaf, root = np.array([perm[0]], dtype=np.int64), np.array([perm[dim - 1]], dtype=np.int64)
    r16, x16 = rng.choice(dim, 16, replace=False).astype(np.int64), rng.choice(dim, 16, replace=False).astype(np.int64)
    i64 = rng.choice(dim, 64, replace=False).astype(np.int64)
    cases = {
        "okkt_solve_dev, 1 column": dense,
        "leaf non-zero, all of x": sparse(leaf, None),
        "leaf non-zero, that entry of x": sparse(leaf, leaf),
        "root non-zero, all of x": sparse(root, None),
        "root non-zero, that entry of x": sparse(root, root),
        "16 non-zeros, 16 wanted rows": sparse(r16, x16),
        "inverse_block of 64 indices": block(i64),
    }
    for name, call in cases.items():
        res["cases"][name] = timed(call, reps, warmup)
    st = h.stats()
    res.update(nsuper=int(st["nsuper"]), nlevels=int(st["nlevels"]), max_front=int(st["max_front"]))
    for p in (d_k, d_b, d_x, d_v, d_o):
        h.dev_free(p)
    finalize_b(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="S-C3,S-metric")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/sparse_solve_timing.json")
    a = ap.parse_args()
    out = {"what": "okkt_solve_sparse_dev / okkt_get_inverse_columns_dev next to okkt_solve_dev: device ms (HIP events) and host wall ms, medians of reps",
           "results": [one(c, a.reps, a.warmup) for c in a.configs.split(",")]}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
