"""The dense factor of the Schur complement and the fused solve on S-C5 with its 200 linking x-columns as the
Schur set, plus one synthetic dense S of order 2048 through the caller-supplied path.  Times okkt_schur_factor_dev,
okkt_schur_dense_solve_dev and okkt_schur_solve_dev for one right-hand side next to okkt_schur_condense_dev + okkt_schur_expand_dev (the
route without a device factor of S) and the whole-matrix okkt_solve_dev on a second handle, all in one run; medians of --reps after
--warmup, host clock around calls that end in a device synchronisation.  Writes one JSON object to --out and prints the table of
section 8.7."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "scripts")
from schur_timing import timed
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP


def spectrum(n, seed=0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = 10.0 ** rng.uniform(-3.0, 0.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    S = (Q * lam) @ Q.T
    return (S + S.T) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=2048)
    ap.add_argument("--only-factor", action="store_true", help="a few factorisations and nothing else (for a kernel trace)")
    ap.add_argument("--out", default="schur_solve_timing.json")
    a = ap.parse_args()
    prob = synth.make_config("S-C5", seed=0)
    K = synth.augmented_matrix(prob, delta=1e-8)
    n, m = prob["n"], prob["m"]
    dim, ns = n + m, 200
    vals = np.asarray(K.data, dtype=np.float64)
    b = np.random.default_rng(0).normal(size=dim)
    res = {"config": "S-C5", "dim": dim, "ns": ns, "reps": a.reps}

    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.set_schur(np.arange(n - ns, n))
    h.analyze(K)
    hv, hb, hx = h.dev_upload(vals), h.dev_upload(b), h.dev_alloc(8 * dim)
    hr2 = h.dev_alloc(8 * ns)
    assert h.ls_factor_schur_dev(hv, n - ns, m) == 1
    assert h.schur_factor_dev() == 1
    if a.only_factor:
        for _ in range(5):
            h.schur_factor_dev()
    else:
        res["schur_factor_ms"] = timed(h.schur_factor_dev, a.reps, a.warmup)
        res["schur_inertia"], res["total_inertia"] = h.schur_inertia, h.total_inertia
        res["dense_solve_ms"] = timed(lambda: h.schur_dense_solve_dev(hr2, hr2, 1), a.reps, a.warmup)
        res["fused_solve_ms"] = timed(lambda: h.schur_solve_dev(hb, hx, 1), a.reps, a.warmup)

        def cond_expand():
            h.schur_condense_dev(hb, hr2, 1)
            h.schur_expand_dev(hb, hr2, hx, 1)      # (x2 = r2 here: the timing does not depend on the values)
        res["condense_expand_ms"] = timed(cond_expand, a.reps, a.warmup)
        res["condense_ms"] = timed(lambda: h.schur_condense_dev(hb, hr2, 1), a.reps, a.warmup)
        w = linear_solver_HIP("symmetric")
        initialize_b(w)
        w.analyze(K)
        wv, wb, wx = w.dev_upload(vals), w.dev_upload(b), w.dev_alloc(8 * dim)
        assert w.ls_factor_dev(wv, n, m) == 1
        res["whole_solve_ms"] = timed(lambda: w.ls_solve_dev(wb, wx, 1), a.reps, a.warmup)
        h.schur_solve_dev(hb, hx, 1)
        x, xw = h.dev_download(hx, (dim,)), w.dev_download(wx, (dim,))
        res["x_rel_diff_vs_whole"] = float(np.max(np.abs(x - xw)) / np.max(np.abs(xw)))
        finalize_b(w)
    finalize_b(h)

    # a synthetic S of order --big: any Schur-mode handle of that order takes it
    nb = a.big
    prob2 = synth.make_problem(nb + 500, 500, seed=1, well_scaled=True)
    K2 = synth.augmented_matrix(prob2, delta=1e-8)
    g = linear_solver_HIP("symmetric")
    initialize_b(g)
    g.set_schur(np.arange(nb))
    g.analyze(K2)
    S = spectrum(nb)
    gS = g.dev_upload(S)
    gr = g.dev_upload(np.random.default_rng(1).normal(size=nb))
    assert g.schur_factor_dev(gS, nb) == 1
    if a.only_factor:
        for _ in range(3):
            g.schur_factor_dev(gS, nb)
    else:
        res["big_ns"] = nb
        res["big_factor_ms"] = timed(lambda: g.schur_factor_dev(gS, nb), a.reps, a.warmup)
        res["big_dense_solve_ms"] = timed(lambda: g.schur_dense_solve_dev(gr, gr, 1), a.reps, a.warmup)
        res["big_inertia"] = g.schur_inertia
    finalize_b(g)
    print(json.dumps(res))
    if not a.only_factor:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("| call (median of %d, ms) | S-C5, ns = 200 | ns = %d |" % (a.reps, nb))
        print("|---|---|---|")
        print("| okkt_schur_factor_dev | %.3f | %.3f |" % (res["schur_factor_ms"][0], res["big_factor_ms"][0]))
        print("| okkt_schur_dense_solve_dev, 1 rhs | %.3f | %.3f |" % (res["dense_solve_ms"][0], res["big_dense_solve_ms"][0]))
        print("| okkt_schur_solve_dev, 1 rhs | %.3f | |" % res["fused_solve_ms"][0])
        print("| okkt_schur_condense_dev + okkt_schur_expand_dev | %.3f | |" % res["condense_expand_ms"][0])
        print("| okkt_solve_dev, whole matrix | %.3f | |" % res["whole_solve_ms"][0])


if __name__ == "__main__":
    main()
