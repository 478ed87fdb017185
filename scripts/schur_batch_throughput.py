"""Throughput of the scenario batches: arrowhead systems of B blocks factored and solved per second by
okkt_factor_schur_batch_dev + okkt_schur_batch_factor_dev + okkt_schur_batch_solve_dev, against the loop over ONE handle in Schur mode
-- okkt_factor_schur_dev, okkt_get_schur_dev and a device sum per block, one okkt_schur_factor_dev of the sum, okkt_schur_solve_dev per
block -- the only way to do this work without the batch, in the same process.

    python scripts/schur_batch_throughput.py [--out profiles/schur_batch_throughput.json] [--reps 5] [--sizes 1,8,64,512]

The loop is favoured: one handle holds one factor of A11, so a real caller would have to factor every block a second time before its
back-substitution (or keep B handles); the loop here solves every block with the factor that happens to be there.  Its figure is a
lower bound of what the work costs without the batch.

Every figure is a window between two device events on the handle's stream around the whole piece of work (host round trips of the
calls included: they are part of what a caller pays), repeated inside the window until it lasts about 20 ms; every shape is warmed up;
the two ways alternate `reps` times and the median and the range are reported.  Above 64 blocks the per-block part of the loop is timed
on 64 blocks and scaled (it costs the same per block); its dense part is timed whole."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from onephase_jl_amd import _lib as L  # noqa: E402
from onephase_jl_amd import synth  # noqa: E402
from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP  # noqa: E402

WINDOW_MS = 20.0
NSEQ_MAX = 64


def inputs():
    """(name, handle analysed in Schur mode, base values, n1, m1)"""
    import schur_batch_designs as sbd
    sc = sbd.scenario("set-65-small-only")
    yield "set-65-small-only (designed tree, ns = 65)", sc.handle(), sc.vals(1)[0], sc.n1pos, sc.n1neg
    prob = synth.hanging_chain(N_h=400)
    K = sp.tril(synth.augmented_matrix(prob, delta=1.0), format="csc")
    K.sort_indices()
    n, m = prob["n"], prob["m"]
    idx = (np.arange(16) * n) // 16 + n // 32      # 16 linking variables spread over the primal block
    h = linear_solver_HIP("symmetric", False, False)
    initialize_b(h)
    h.set_schur(idx)
    h.analyze(K)
    yield "hanging_chain(N_h=400), augmented, 16 linking variables", h, K.data.copy(), n - 16, m


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


def measure(name, h, base, n1, m1, sizes, reps):
    q = h.schur_batch_query(nrhs_max=1)
    st = h.stats()
    assert q["eligible"] == 1, q
    nnz, dim, ns = len(base), st["n"], q["ns"]
    rng = np.random.default_rng(0)
    timer = Timer(h)
    dev = torch.device("cuda:0")
    rows = []
    for B in sizes:
        vals = torch.from_numpy(base[None, :] * rng.uniform(0.9, 1.1, size=(B, nnz))).to(dev)
        rhs = torch.from_numpy(rng.normal(size=(B, dim))).to(dev)
        sol = torch.empty_like(rhs)
        Sb = torch.empty(ns * ns, dtype=torch.float64, device=dev)
        acc = torch.zeros(ns * ns, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nseq = min(B, NSEQ_MAX)
        h.schur_batch_reserve(B, nrhs_max=1)

        def seq_blocks():
            with torch.cuda.stream(timer.stream):
                acc.zero_()
                for b in range(nseq):
                    h.ls_factor_schur_dev(vals[b].data_ptr(), n1, m1)
                    h.schur_dev(Sb.data_ptr(), ns)
                    acc.add_(Sb)

        def seq_dense_and_solves():
            h.schur_factor_dev(acc.data_ptr(), ns)
            for b in range(nseq):
                h.schur_solve_dev(rhs[b].data_ptr(), sol[b].data_ptr(), 1)

        def seq_dense():
            h.schur_factor_dev(acc.data_ptr(), ns)

        def batch():
            h.ls_factor_schur_batch_dev(vals.data_ptr(), B, nnz, n1, m1)
            h.schur_batch_factor_dev()
            h.schur_batch_solve_dev(rhs.data_ptr(), sol.data_ptr(), B, 1)

        ways = {"loop_blocks": seq_blocks, "loop_dense_and_solves": seq_dense_and_solves, "loop_dense": seq_dense, "batch": batch}
        ms = {w: [] for w in ways}
        counts = {}
        for rep in range(reps + 1):      # rep 0 warms every shape up and sizes the windows
            for w, work in ways.items():
                if rep == 0:
                    work()
                    counts[w] = max(1, int(WINDOW_MS / max(timer.window(work, 1), 1e-3)))
                    continue
                ms[w].append(timer.window(work, counts[w]))
        t = {w: np.array(v) for w, v in ms.items()}
        scale = B / nseq
        # the loop: its per-block parts scaled to B blocks, its one dense factorisation counted once
        loop = (t["loop_blocks"] + t["loop_dense_and_solves"] - t["loop_dense"]) * scale + t["loop_dense"]
        row = dict(B=B, blocks_timed_in_the_loop=nseq)
        for w, per in (("loop", loop), ("batch", t["batch"])):
            row[w] = dict(ms_per_arrowhead_system=dict(min=float(per.min()), median=float(np.median(per)), max=float(per.max())),
                          blocks_per_s=dict(min=1e3 * B / per.max(), median=1e3 * B / float(np.median(per)), max=1e3 * B / per.min()))
        row["loop_parts_ms"] = {w: float(np.median(t[w])) for w in ("loop_blocks", "loop_dense_and_solves", "loop_dense")}
        row["calls_per_window"] = counts
        row["batch_over_loop"] = float(np.median(loop) / np.median(t["batch"]))
        rows.append(row)
        print("%-58s B=%4d   loop %9.0f blocks/s   batch %9.0f blocks/s   x %.2f" % (
            name, B, row["loop"]["blocks_per_s"]["median"], row["batch"]["blocks_per_s"]["median"], row["batch_over_loop"]), flush=True)
        h.schur_batch_release()
    return dict(input=name, dim=dim, ns=ns, nnz=nnz, nsuper=st["nsuper"], interior_max_front=q["max_front"], levels=q["levels"], tasks=q["tasks_per_item"],
                bytes_per_item=q["bytes_per_item"], bytes_shared=q["bytes_shared"], rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,8,64,512")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lib = L.load()
    out = dict(what="scenario batches: factor of every block + sum of the S_b + dense factor + one fused solve (one right-hand side) per arrowhead "
                    "system of B blocks, windows between device events on the handle's stream; the loop over one handle does not refactor a block "
                    "before its back-substitution (a lower bound of its real cost)",
               version=lib.okkt_version().decode(), device=torch.cuda.get_device_name(0), reps=a.reps, window_ms=WINDOW_MS,
               results=[measure(name, h, base, n1, m1, sizes, a.reps) for name, h, base, n1, m1 in inputs()])
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
