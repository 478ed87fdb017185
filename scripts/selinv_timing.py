"""Selected inversion on S-C3, S-C5 and S-metric, the systems bench.py factors: okkt_factor on device values,
then okkt_selinv, next to each other on one handle; medians of --reps after --warmup (host clock around calls that end in a device
synchronisation, and the device time okkt_selinv reports), the bytes it holds and the rate of its block products.  Writes one JSON
object to --out."""
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


def one(config, reps, warmup):
    prob = synth.make_config(config, seed=0)
    K = synth.augmented_matrix(prob, delta=1e-8)
    n, m = prob["n"], prob["m"]
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(K)
    d_vals = h.dev_upload(np.asarray(K.data, dtype=np.float64))
    assert h.ls_factor_dev(d_vals, n, m) in (0, 1)
    res = {"config": config, "dim": n + m}
    res["factor_ms"] = timed(lambda: h.ls_factor_dev(d_vals, n, m), reps, warmup)
    h.ls_factor_dev(d_vals, n, m)
    info = h.selinv()
    dev = []

    def run():
        dev.append(h.selinv()["seconds_device"] * 1e3)
    res["selinv_ms"] = timed(run, reps, warmup)
    res["selinv_device_ms_median"] = float(np.median(dev[warmup:]))
    res["selinv_over_factor"] = res["selinv_ms"][0] / res["factor_ms"][0]
    res["selinv_flops"] = info["flops"]
    res["selinv_tflops"] = info["flops"] / (res["selinv_device_ms_median"] * 1e-3) / 1e12
    res["arena_bytes"] = info["arena_bytes"]
    res["nonfinite"] = info["nonfinite"]
    st = h.stats()
    res["factor_flops_stored"] = st["flops_stored"]
    res["stats"] = {k: st[k] for k in ("nsuper", "nlevels", "max_front", "n_big_fronts", "arena_bytes")}
    finalize_b(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="S-C3,S-C5,S-metric")
    ap.add_argument("--out", default="selinv_timing.json")
    a = ap.parse_args()
    out = {"results": []}
    for c in a.configs.split(","):
        r = one(c, a.reps, a.warmup)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
