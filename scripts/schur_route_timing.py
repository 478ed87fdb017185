"""Times for DESIGN.md 8.10: S^-1 by okkt_schur_get_inverse_dev against ns right-hand sides through okkt_schur_dense_solve_dev, and
okkt_schur_selinv against okkt_selinv of the same design factored whole.  Medians after warm-up; device events where the handle has them.  Run from the repository root on an MI355X; writes
profiles/schur_route_timing.json."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import dense_ldlt_ref as ref
import front_trees as ft
import schur_case as sc
import schur_trees as sct
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

out = {}
K, n, m = sc.kkt()
for ns in (257, 2049):
    h = sc.schur_handle("symmetric", K, np.random.default_rng(ns).permutation(n + m)[:ns])
    S = ref.heavy_tail(ns)
    assert h.schur_factor(S) == 1
    d_Z = h.dev_alloc(8 * ns * ns)
    ev, wall = [], []
    for it in range(23):
        t0 = time.perf_counter()
        h.schur_inverse_dev(d_Z)
        t1 = time.perf_counter()
        if it >= 3:
            ev.append(h.stats()["last_solve_ms"])
            wall.append((t1 - t0) * 1e3)
    Z = h.dev_download(d_Z, (ns, ns))
    d_I = h.dev_upload(np.eye(ns))
    d_X = h.dev_alloc(8 * ns * ns)
    sw = []
    for it in range(7):
        t0 = time.perf_counter()
        h.schur_dense_solve_dev(d_I, d_X, nrhs=ns)
        t1 = time.perf_counter()
        if it >= 2:
            sw.append((t1 - t0) * 1e3)
    X = h.dev_download(d_X, (ns, ns))
    out[f"inverse_{ns}"] = dict(event_ms_median=float(np.median(ev)), event_ms_min=float(np.min(ev)), event_ms_max=float(np.max(ev)),
                                wall_ms_median=float(np.median(wall)), solves_wall_ms_median=float(np.median(sw)), solves_wall_ms_min=float(np.min(sw)),
                                solves_wall_ms_max=float(np.max(sw)), max_diff=float(np.max(np.abs(Z - X)) / np.max(np.abs(X))),
                                gflops=float(ns) ** 3 / (np.median(ev) * 1e-3) / 1e9)
    print(json.dumps({f"inverse_{ns}": out[f"inverse_{ns}"]}), flush=True)
    for p in (d_Z, d_I, d_X):
        h.dev_free(p)
    finalize_b(h)

for name in ("set-257", "set-2049-thin"):
    d = sct.build(name, values="plain")
    ns = sct.set_size(d)
    n1 = d.n - ns
    n1pos = sct.interior_positive(d)
    h = sct.schur_handle(d)
    assert h.ls_factor_schur(d.A, n1pos, n1 - n1pos) == 1 and h.schur_factor() == 1
    a = [h.schur_selinv()["seconds_device"] * 1e3 for _ in range(13)][3:]
    w = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(w)
    w.set_perm(d.perm)
    assert w.ls_factor_b(d.A, d.npos, d.nneg) == 1
    b = [w.selinv()["seconds_device"] * 1e3 for _ in range(13)][3:]
    out[f"selinv_{name}"] = dict(schur_ms_median=float(np.median(a)), schur_ms_min=float(np.min(a)), schur_ms_max=float(np.max(a)),
                                 plain_ms_median=float(np.median(b)), plain_ms_min=float(np.min(b)), plain_ms_max=float(np.max(b)))
    print(json.dumps({f"selinv_{name}": out[f"selinv_{name}"]}), flush=True)
    finalize_b(h)
    finalize_b(w)

os.makedirs("profiles", exist_ok=True)
json.dump(out, open("profiles/schur_route_timing.json", "w"), indent=1)
