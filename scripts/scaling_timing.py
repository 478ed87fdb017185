"""Cost and effect of the symmetric equilibration on the augmented system K of S-small and S-metric, the system
bench.py factors, everything resident on the device.  Per configuration, for a plain handle, a handle with a caller's vector (the value
pass and the row-maximum pass without sweeps) and a handle with OKKT_SCALE_RUIZ at --sweeps: the device time of okkt_factor_dev and of
okkt_solve_dev (HIP events of the handle, medians of --reps after --warmup), and omega0, ferr and okkt_condest of the plain solve.  The
scaling phase alone is the difference of the factor times: it runs inside the timed span.  Prints SCALING {json} lines and writes
--out."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP


def median_ms(fn, key, h, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        fn()
        ts.append(h.stats()[key])
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def one(config, delta, sweeps, reps, warmup):
    prob = synth.make_config(config, seed=1 if config == "S-small" else 0)
    n, m = prob["n"], prob["m"]
    K = synth.augmented_matrix(prob, delta=delta)
    vals = np.asarray(K.data, dtype=np.float64)
    b = np.random.default_rng(9).normal(size=n + m)
    res = {"config": config, "dim": n + m, "nnz": int(K.nnz), "delta": delta, "sweeps": sweeps}
    s_ruiz = None
    for tag in ("plain", "ruiz", "user"):
        h = linear_solver_HIP("symmetric")
        initialize_b(h)
        h.analyze(K)
        if tag == "ruiz":
            h.set_scaling("ruiz", sweeps)
        elif tag == "user":
            h.set_scaling("user", s=s_ruiz)
        d_v = h.dev_upload(vals)
        d_b = h.dev_upload(b)
        d_x = h.dev_alloc(8 * (n + m))
        flag = h.ls_factor_dev(d_v, n, m)
        r = {"flag": flag, "factor_ms": median_ms(lambda: h.ls_factor_dev(d_v, n, m), "last_factor_ms", h, reps, warmup),
             "solve_ms": median_ms(lambda: h.ls_solve_dev(d_b, d_x, 1), "last_solve_ms", h, reps, warmup)}
        x, info = h.ls_solve_refine(vals, b, max_steps=0)
        ferr, berr = h.forward_error(vals, b, x)
        ce = h.condest(vals)
        r.update(omega0=info["omega0"], ferr=float(ferr), cond1=ce["cond1"], norm1=ce["norm1"], inv_norm1=ce["inv_norm1"])
        if tag != "plain":
            si = h.scaling_info()
            r.update(rowmax_min=si["rowmax_min"], rowmax_max=si["rowmax_max"], zero_rows=si["zero_rows"])
            s = h.scaling()
            r.update(s_min=float(s.min()), s_max=float(s.max()))
            if tag == "ruiz":
                s_ruiz = s
        res[tag] = r
        for p in (d_v, d_b, d_x):
            h.dev_free(p)
        finalize_b(h)
    res["scaling_phase_ms"] = res["ruiz"]["factor_ms"][0] - res["plain"]["factor_ms"][0]
    res["value_and_rowmax_pass_ms"] = res["user"]["factor_ms"][0] - res["plain"]["factor_ms"][0]
    res["added_solve_ms"] = res["ruiz"]["solve_ms"][0] - res["plain"]["solve_ms"][0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="S-small,S-metric")
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--out", default="scaling_timing.json")
    a = ap.parse_args()
    out = {"results": []}
    for c in a.configs.split(","):
        r = one(c, 1e-4 if c == "S-small" else 1e-8, a.sweeps, a.reps, a.warmup)
        print("SCALING " + json.dumps(r), flush=True)
        out["results"].append(r)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
