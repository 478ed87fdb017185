"""Throughput of the line-search batches: one line-search round per item -- max step, s-bound test, dual range,
predicted reduction, dual step -- for B iterates on the hanging-chain structure (n + m = 1608, symmetric kind) whose directions are
resident in the slots of a KKT batch, through okkt_kkt_items_max_step_primal ... okkt_kkt_items_dual_step and as the loop
items_select(b) + the single-iterate calls over the same items, in the same process.

    python scripts/ls_items_throughput.py [--out profiles/ls_items_throughput.json] [--reps 5] [--sizes 1,16,64,512]

The step before the round (form, delta loop, rhs, direction) is run once per shape and not timed.  Both ways go through the Python mirror
(line_search.py), so both pay its packing of the arguments; the fraction vectors are one vector for every item (stride 0), the candidates'
Jacobian is one array for every item.

Every figure is a window between two device events on the handle's stream around whole rounds (host round trips included: they are part of
what a caller pays), repeated inside the window until it lasts about 20 ms; every shape is warmed up; the two ways alternate `reps` times
and the median and the range are reported.  Above 64 items the loop is timed on 64 items and scaled (it costs the same per item)."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from onephase_jl_amd import _lib as L  # noqa: E402
from onephase_jl_amd import kkt_system_solver as KS  # noqa: E402
from onephase_jl_amd import line_search as LS  # noqa: E402
from onephase_jl_amd import synth  # noqa: E402
from onephase_jl_amd.linear_system_solvers import linear_solver_HIP  # noqa: E402

WINDOW_MS = 20.0
NSEQ_MAX = 64
KIND = "symmetric"
CALLS = ("max_step", "s_bound", "dual_range", "predicted_reduction", "dual_step")


def iterates(prob, B, seed=0):
    rng = np.random.default_rng(seed)
    n, m = prob["n"], prob["m"]
    return [KS.Class_iterate(x=np.zeros(n), y=prob["y"] * rng.uniform(0.5, 2.0, size=m), s=prob["s"] * rng.uniform(0.5, 2.0, size=m), mu=prob["mu"] * (1.0 + 0.01 * b),
                             J=prob["J"], H=prob["H"], grad=rng.normal(size=n), cons=prob["s"] + 0.1 * rng.normal(size=m)) for b in range(B)]


def window(stream, work, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(count):
        work()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,64,512")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lib = L.load()
    prob = synth.hanging_chain(N_h=400)
    m = prob["m"]
    eta = KS.Reduct_affine()
    pars = LS.Class_ls_parameters()
    rng = np.random.default_rng(1)
    fp, fb = rng.uniform(0.05, 0.3, size=m), rng.uniform(0.05, 0.3, size=m)
    rows = []
    info = None
    for B in sizes:
        its = iterates(prob, B)
        k = KS.HIP_KKT_solver(KIND)
        k.initialize_b(its[0])
        k._set_structure(its[0])
        info = LS.items_ls_query(k)
        assert info["eligible"] == 1, info
        k.items_reserve(B)
        k.form_system_items(its)
        k.ipopt_strategy_items(its)
        k.kkt_associate_rhs_items(its, eta)
        dirs, _ = k.compute_direction_items(check_nan=False)      # on the host for the candidates; they stay resident as well
        alpha = [0.5 / (1 + b % 7) for b in range(B)]
        cands = [dataclasses.replace(it, s=np.abs(it.s + al * d.s) + 1e-3, mu=it.mu + al * d.mu) for it, d, al in zip(its, dirs, alpha)]
        Jc = its[0].J * 1.01
        new_its = [dataclasses.replace(c, grad=c.grad + 0.1 * al, J=Jc) for c, al in zip(cands, alpha)]
        s_new = np.stack([c.s for c in cands])
        stream = torch.cuda.ExternalStream(int(lib.okkt_get_stream(linear_solver_HIP.of_kkt(k)._h)))
        nseq = min(B, NSEQ_MAX)
        state = {}

        def batch():
            t = [time.perf_counter()]
            step_P, _ = LS.max_step_primal_items(k, fp, pars); t.append(time.perf_counter())
            ok = LS.s_bound_ok_items(k, s_new, fb, pars); t.append(time.perf_counter())
            lb, ub = LS.dual_step_range_items(k, cands, fb, pars); t.append(time.perf_counter())
            pred = LS.predicted_reduction_terms_items(k, alpha); t.append(time.perf_counter())
            sd = LS.move_dual_step_items(k, new_its, alpha, lb, ub, 1.0, 1.0, pars); t.append(time.perf_counter())
            state["items"] = (step_P[:nseq].copy(), ok[:nseq].copy(), lb[:nseq].copy(), ub[:nseq].copy(), pred[:nseq].copy(), sd[:nseq].copy())
            state["host_ms"] = {c: 1e3 * (t[i + 1] - t[i]) for i, c in enumerate(CALLS)}

        def loop():
            out = []
            for b in range(nseq):
                k.items_select(b)
                step_P, _ = LS.max_step_primal(k, fp, pars)
                ok = LS.s_bound_ok(k, cands[b].s, fb, pars)
                lb, ub = LS.dual_step_range(k, cands[b], fb, pars)
                pred = LS.predicted_reduction_terms(k, alpha[b])
                sd = LS.move_dual_step(k, new_its[b], alpha[b], lb, ub, 1.0, 1.0, pars)
                out.append((step_P, int(ok), lb, ub, pred, sd))
            state["loop"] = out

        ways = {"loop": loop, "items": batch}
        ms = {w: [] for w in ways}
        counts = {}
        for rep in range(a.reps + 1):      # rep 0 warms every shape up and sizes the windows
            for w, work in ways.items():
                if rep == 0:
                    work()
                    counts[w] = max(1, int(WINDOW_MS / max(window(stream, work, 1), 1e-3)))
                    continue
                ms[w].append(window(stream, work, counts[w]))
        # the two ways computed the same numbers (bytes)
        cols = list(zip(*state["loop"]))
        same = all(np.array(col, dtype=got.dtype).tobytes() == got.tobytes() for col, got in zip(cols, state["items"]))
        t_loop = np.array(ms["loop"]) * (B / nseq)
        t_items = np.array(ms["items"])
        row = dict(B=B, items_timed_in_the_loop=nseq, calls_per_window=counts, same_bytes_both_ways=bool(same))
        for w, per in (("loop", t_loop), ("items", t_items)):
            row[w] = dict(ms_per_round_of_B=dict(min=float(per.min()), median=float(np.median(per)), max=float(per.max())),
                          items_per_s=dict(min=1e3 * B / per.max(), median=1e3 * B / float(np.median(per)), max=1e3 * B / per.min()))
        row["items_over_loop"] = float(np.median(t_loop) / np.median(t_items))
        row["host_ms_of_the_batched_calls"] = state["host_ms"]
        rows.append(row)
        print("B=%4d   loop %9.0f items/s   items %9.0f items/s   x %.2f   same bytes %s" % (
            B, row["loop"]["items_per_s"]["median"], row["items"]["items_per_s"]["median"], row["items_over_loop"], same), flush=True)
        k.finalize_b()
    out = dict(what="line-search batches: max step + s-bound + dual range + predicted reduction + dual step per item, B iterates on hanging_chain(N_h=400), symmetric "
                    "kind, directions resident; windows between device events on the handle's stream; the comparison base is the loop items_select(b) + the "
                    "single-iterate calls on the same solver",
               version=lib.okkt_version().decode(), device=torch.cuda.get_device_name(0), reps=a.reps, window_ms=WINDOW_MS, n=int(prob["n"]), m=int(prob["m"]),
               ls_info=info, rows=rows)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
