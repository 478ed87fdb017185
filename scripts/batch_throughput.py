"""Throughput of the uniform batches: systems factored and solved per second by okkt_factor_batch_dev +
okkt_solve_batch_dev in level mode and in item mode, against the sequential loop of okkt_factor_dev + okkt_solve_dev on one handle --
the only way to do this work without a batch -- in the same process.

    python scripts/batch_throughput.py [--out profiles/batch_throughput.json] [--reps 5] [--sizes 1,8,64,512,4096]

Every figure is a window between two device events on the handle's stream around the whole piece of work (host round trips of the
calls included: they are part of what a caller pays), repeated inside the window until it lasts about 20 ms; every shape is warmed up;
the three ways alternate `reps` times and the range is reported.  device_ms_* are the library's own event spans of the calls
(okkt_stats.last_factor_ms / last_solve_ms) summed: the device time without the host gaps."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onephase_jl_amd import _lib as L  # noqa: E402
from onephase_jl_amd import synth  # noqa: E402
from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP  # noqa: E402

WINDOW_MS = 20.0


def inputs():
    for name, prob, delta in (("hanging_chain(N_h=400), augmented", synth.hanging_chain(N_h=400), 1.0),
                              ("S-tiny, augmented", synth.make_config("S-tiny", seed=3), 1e-4)):
        K = sp.tril(synth.augmented_matrix(prob, delta=delta), format="csc")
        K.sort_indices()
        yield name, K, prob["n"], prob["m"]


class Timer:
    def __init__(self, h):
        self.stream = torch.cuda.ExternalStream(int(h._lib.okkt_get_stream(h._h)))

    def window(self, work, count):
        """ms per call of work(), from one window of `count` calls between two events on the handle's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        for _ in range(count):
            work()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / count


def measure(name, K, n, m, sizes, reps):
    h = linear_solver_HIP("symmetric", False, False)
    initialize_b(h)
    h.analyze(K)
    q = h.batch_query(nrhs_max=1)
    st = h.stats()
    assert q["eligible"] == 1, q
    nnz, dim = K.nnz, K.shape[0]
    free, _ = torch.cuda.mem_get_info()
    rng = np.random.default_rng(0)
    timer = Timer(h)
    rows = []
    for B in sizes:
        need = B * (q["bytes_per_item"] + 8 * nnz + 16 * dim)
        if need > 0.6 * free:
            rows.append(dict(B=B, skipped="%.1f GB of slots, values and vectors do not fit" % (need / 1e9)))
            continue
        vals = K.data[None, :] * rng.uniform(0.9, 1.1, size=(B, nnz))
        d_vals = h.dev_upload(vals)
        d_rhs = h.dev_upload(rng.normal(size=(B, dim)))
        d_sol = h.dev_alloc(8 * B * dim)
        nseq = min(B, 256)      # the sequential loop costs the same per system: a part of a large batch is enough to time it

        def seq():
            dev = 0.0
            for b in range(nseq):
                h.ls_factor_dev(d_vals + 8 * nnz * b, n, m)
                dev += h.stats()["last_factor_ms"]
                h.ls_solve_dev(d_rhs + 8 * dim * b, d_sol + 8 * dim * b, 1)
                dev += h.stats()["last_solve_ms"]
            return dev

        def batch():
            h.ls_factor_batch_dev(d_vals, B, nnz, n, m)
            dev = h.stats()["last_factor_ms"]
            h.ls_solve_batch_dev(d_rhs, d_sol, B, 1)
            return dev + h.stats()["last_solve_ms"]

        ways = {"sequential": (seq, nseq, None), "level": (batch, B, "level"), "item": (batch, B, "item")}
        ms = {w: [] for w in ways}
        dev_ms, counts = {}, {}
        for rep in range(reps + 1):      # rep 0 warms every shape up and sizes the windows
            for w, (work, systems, mode) in ways.items():
                if mode:
                    h.batch_reserve(B, nrhs_max=1, mode=mode)
                if rep == 0:
                    work()
                    once = timer.window(work, 1)
                    counts[w] = max(1, int(WINDOW_MS / max(once, 1e-3)))
                    dev_ms[w] = work() / systems
                    continue
                ms[w].append(timer.window(work, counts[w]) / systems)
        row = dict(B=B)
        for w in ways:
            per = np.array(ms[w])
            row[w] = dict(systems_per_s=dict(min=1e3 / per.max(), median=1e3 / np.median(per), max=1e3 / per.min()),
                          us_per_system=dict(min=1e3 * per.min(), median=1e3 * float(np.median(per)), max=1e3 * per.max()),
                          device_us_per_system=1e3 * dev_ms[w], calls_per_window=counts[w])
        rows.append(row)
        print("%-36s B=%5d   sequential %9.0f /s   level %9.0f /s   item %9.0f /s" % (
            name, B, row["sequential"]["systems_per_s"]["median"], row["level"]["systems_per_s"]["median"],
            row["item"]["systems_per_s"]["median"]), flush=True)
        h.batch_release()
        for p in (d_vals, d_rhs, d_sol):
            h.dev_free(p)
    return dict(input=name, dim=dim, nnz=nnz, nsuper=st["nsuper"], max_front=st["max_front"], levels=q["levels"], tasks=q["tasks_per_item"],
                bytes_per_item=q["bytes_per_item"], rows=rows)


def delta_loop(reps):
    """ipopt_strategy! on the indefinite design of order 37 (lambda_min = -3.7, symmetric kind): the serial loop against the batched one,
    ms per loop from windows of 20 loops between device events on the linear solver's stream."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import lanczos_ref as R
    from onephase_jl_amd import kkt_system_solver as KS
    it = R.indefinite_design(KS.Class_iterate, 37, -3.7)
    ways = {"serial": 0, "width 4": 4, "width 16": 16}
    solvers, timers, ms, facts = {}, {}, {w: [] for w in ways}, {}
    for w, width in ways.items():
        k = KS.HIP_KKT_solver("symmetric", hip_delta_batch=width)
        it.delta = 0.0
        k.initialize_b(it)
        k.form_system_b(it)
        solvers[w] = k
        timers[w] = Timer(linear_solver_HIP.of_kkt(k))
        status, nfac, delta = k.ipopt_strategy_b(it)      # warm-up (and the reservation of the slots)
        facts[w] = dict(status=status, num_fac=nfac, delta=delta, loop=k.delta_loop, launches=k.delta_launches)
        it.delta = 0.0
    for _ in range(reps):
        for w, k in solvers.items():
            ms[w].append(timers[w].window(lambda: k.ipopt_strategy_b(it), 20))
    out = {w: dict(facts[w], ms_per_loop=dict(min=min(ms[w]), median=float(np.median(ms[w])), max=max(ms[w]))) for w in ways}
    print("delta loop, n = 37: " + "   ".join("%s %.3f ms" % (w, out[w]["ms_per_loop"]["median"]) for w in ways), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,8,64,512,4096")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lib = L.load()
    out = dict(what="uniform batches: factor + solve (one right-hand side) per system, windows between device events on the handle's stream",
               version=lib.okkt_version().decode(), device=torch.cuda.get_device_name(0), reps=a.reps, window_ms=WINDOW_MS,
               results=[measure(name, K, n, m, sizes, a.reps) for name, K, n, m in inputs()])
    out["delta_loop_n37"] = delta_loop(a.reps)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
