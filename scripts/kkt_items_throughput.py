"""Throughput of the KKT batches: one full interior-point step per item -- form_system!, the delta loop of
ipopt_strategy!, System_rhs, compute_direction! with its N err -- for B iterates on the hanging-chain structure (n + m = 1608, symmetric
kind), through okkt_kkt_items_* and as the loop over ONE HIP_KKT_solver calling the single-iterate entry points, in the same process.

    python scripts/kkt_items_throughput.py [--out profiles/kkt_items_throughput.json] [--reps 5] [--sizes 1,16,64,512]

The iterates share the structure and differ in (s, y, grad, cons); every fourth one carries -H / 2 instead of H, so that the items leave
the delta loop in different rounds (the chain's Hessian is indefinite at this point: three quarters of the items take six attempts, the
others one or two; the output records the histogram).  Both ways go through the Python mirror (kkt_system_solver.py), so both pay its
packing of the arguments.

Every figure is a window between two device events on the handle's stream around the whole step (host round trips included: they are
part of what a caller pays), repeated inside the window until it lasts about 20 ms; every shape is warmed up; the two ways alternate
`reps` times and the median and the range are reported.  Above 64 items the loop is timed on 64 items and scaled (it costs the same per
item).  The form / factor / rhs / direction split of the batched step is okkt_kkt_get_timers' (HIP events inside the calls)."""
import argparse
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
from onephase_jl_amd import synth  # noqa: E402
from onephase_jl_amd.linear_system_solvers import linear_solver_HIP  # noqa: E402

WINDOW_MS = 20.0
NSEQ_MAX = 64
KIND = "symmetric"


def iterates(prob, B, seed=0):
    rng = np.random.default_rng(seed)
    n, m = prob["n"], prob["m"]
    Hneg = prob["H"] * -0.5
    out = []
    for b in range(B):
        out.append(KS.Class_iterate(x=np.zeros(n), y=prob["y"] * rng.uniform(0.5, 2.0, size=m), s=prob["s"] * rng.uniform(0.5, 2.0, size=m), mu=prob["mu"],
                                    J=prob["J"], H=Hneg if b % 4 == 3 else prob["H"], grad=rng.normal(size=n), cons=prob["s"] + 0.1 * rng.normal(size=m)))
    return out


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
    eta = KS.Reduct_affine()
    rows = []
    info = None
    for B in sizes:
        its = iterates(prob, B)
        kb = KS.HIP_KKT_solver(KIND)
        kb.initialize_b(its[0])
        kb._set_structure(its[0])
        info = kb.items_query()
        assert info["eligible"] == 1, info
        kb.items_reserve(B)
        ks = KS.HIP_KKT_solver(KIND)
        ks.initialize_b(its[0])
        ks._set_structure(its[0])
        stream_b = torch.cuda.ExternalStream(int(lib.okkt_get_stream(linear_solver_HIP.of_kkt(kb)._h)))
        nseq = min(B, NSEQ_MAX)
        state = {}

        def batch():
            for it in its:
                it.delta = 0.0
            t0 = time.perf_counter()
            kb.form_system_items(its)
            t1 = time.perf_counter()
            state["form"] = kb.timers()
            t2 = time.perf_counter()
            res, state["launches"] = kb.ipopt_strategy_items(its)
            t3 = time.perf_counter()
            state["factor"] = kb.timers()
            t4 = time.perf_counter()
            kb.kkt_associate_rhs_items(its, eta)
            t5 = time.perf_counter()
            kb.compute_direction_items()
            t6 = time.perf_counter()
            state["dir"] = kb.timers()
            state["num_fac"] = [r[1] for r in res]
            # wall clock of the four calls (the Python mirror's packing and the host side of the copies included), last run
            state["host_ms"] = dict(form=1e3 * (t1 - t0), delta_loop=1e3 * (t3 - t2), rhs=1e3 * (t5 - t4), direction=1e3 * (t6 - t5))

        def loop():
            for it in its[:nseq]:
                it.delta = 0.0
                ks.form_system_b(it)
                ks.ipopt_strategy_b(it)
                ks.kkt_associate_rhs_b(it, eta)
                ks.compute_direction_b()

        stream_s = torch.cuda.ExternalStream(int(lib.okkt_get_stream(linear_solver_HIP.of_kkt(ks)._h)))
        ways = {"loop": (loop, stream_s), "items": (batch, stream_b)}
        ms = {w: [] for w in ways}
        counts = {}
        for rep in range(a.reps + 1):      # rep 0 warms every shape up and sizes the windows
            for w, (work, stream) in ways.items():
                if rep == 0:
                    work()
                    counts[w] = max(1, int(WINDOW_MS / max(window(stream, work, 1), 1e-3)))
                    continue
                ms[w].append(window(stream, work, counts[w]))
        t_loop = np.array(ms["loop"]) * (B / nseq)
        t_items = np.array(ms["items"])
        row = dict(B=B, items_timed_in_the_loop=nseq, calls_per_window=counts)
        for w, per in (("loop", t_loop), ("items", t_items)):
            row[w] = dict(ms_per_step_of_B=dict(min=float(per.min()), median=float(np.median(per)), max=float(per.max())),
                          items_per_s=dict(min=1e3 * B / per.max(), median=1e3 * B / float(np.median(per)), max=1e3 * B / per.min()))
        row["items_over_loop"] = float(np.median(t_loop) / np.median(t_items))
        row["delta_loop_rounds"] = state["launches"]
        row["num_fac_histogram"] = {str(v): int(c) for v, c in zip(*np.unique(state["num_fac"], return_counts=True))}
        row["device_ms_of_the_batched_step"] = dict(form=state["form"]["assemble_ms"], upload=state["form"]["upload_ms"], factor_all_rounds=state["factor"]["factor_ms"],
                                                    rhs=state["dir"]["rhs_ms"], direction=state["dir"]["direction_ms"], kkt_err=state["dir"]["kkt_err_ms"])
        row["host_ms_of_the_batched_calls"] = state["host_ms"]
        rows.append(row)
        print("B=%4d   loop %9.0f items/s   items %9.0f items/s   x %.2f   rounds %d" % (
            B, row["loop"]["items_per_s"]["median"], row["items"]["items_per_s"]["median"], row["items_over_loop"], row["delta_loop_rounds"]), flush=True)
        kb.finalize_b()
        ks.finalize_b()
    out = dict(what="KKT batches: form_system + delta loop + System_rhs + compute_direction per item, B iterates on hanging_chain(N_h=400), symmetric kind; windows "
                    "between device events on the handle's stream; the comparison base is the loop over one HIP_KKT_solver calling the single-iterate entry points",
               version=lib.okkt_version().decode(), device=torch.cuda.get_device_name(0), reps=a.reps, window_ms=WINDOW_MS, n=int(prob["n"]), m=int(prob["m"]),
               launches_form=info["launches_form"], launches_direction=info["launches_direction"], bytes_per_item=info["bytes_per_item"], rows=rows)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
