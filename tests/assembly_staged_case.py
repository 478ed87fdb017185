"""Helper of test_gpu_assembly_staged.py (run as a subprocess: the OKKT_ASM_* switches are read once per process).
argv: output .npz, then case names of CASES.  A case is a designed tree of tests/front_trees.py ("plain" values, the design's
permutation, no amalgamation) and a mode:

  plain    factor, read D and L (CSC), solve one right-hand side
  dup      the same from a raw CSC in which 300 entries are split into two (0.75 v + 0.25 v): the serial has_dup scatter
  schur    the last root held back as the Schur set: S (the assembled Schur front) and one fused solve
  parted   a 2-part partitioned plan on one device: the composed D and L and one solve

The designs put the big-front assembly kernels at their edges (the staged kernel cuts a column into chunks of 512 rows, the chunked
kernel it replaces into chunks of 1024; one wave per (column, chunk)); a child (k, c) under a root of f rows gives the items of c,
c - 1, ... 1 rows, cut at the chunk boundaries:

  p2100    a root of 2100 rows (five chunks of 512 rows, the last of 52; three of 1024) under thirteen children: contiguous CBs of
           1025, 1087, 1088, 1089, 1151, 1152, 1153 rows (pieces of 1, 63, 64, 65, 127, 128 and 129 rows in the chunk that starts at row
           1024, every length from 1 to 512 in the first), of 513 and 1537 rows (one row past a 512-row boundary), of 2048 rows (whole
           chunks: pieces of 512 and 1024 rows), of 1024 rows (empty in the chunks behind it), two scattered ones whose rows straddle every
           boundary; column 0 takes up to thirteen pieces per chunk, columns past 2048 take none or one; the pivot counts 2 .. 7 make
           the source columns start at even and odd entries of the arena
  p2049    a root just above 2048 rows (the threshold of the chunked kernel, and of the staged one under OKKT_ASM_CHUNK_MIN=2048),
           f = 4 * 512 + 1: three idle waves in the last workgroup
  p2048    a root just below it (the LDS-column kernel under OKKT_ASM_CHUNK_MIN=2048)
  p1025    a root one row past a chunk boundary
  mid2150  a front of 2150 rows that is itself a child: its columns past the pivots live in the shared contribution-block region"""
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import front_trees as ft  # noqa: E402
from front_trees import N  # noqa: E402

DESIGNS = {
    "p2100": [N(2100, 0, N(3, 1025), N(2, 1087), N(4, 1088), N(3, 1089), N(2, 1151), N(5, 1152), N(3, 1153), N(2, 2048),
                N(6, 700, scatter=True), N(3, 1024), N(7, 1500, scatter=True), N(2, 513), N(3, 1537))],
    "p2049": [N(2049, 0, N(5, 1025), N(130, 1100, scatter=True), N(2, 1))],
    "p2048": [N(2048, 0, N(5, 1025), N(130, 1100, scatter=True), N(2, 1))],
    "p1025": [N(1025, 0, N(4, 1024), N(3, 700, scatter=True))],
    "mid2150": [N(2200, 0, N(150, 2000, N(4, 1500, scatter=True), N(3, 1025), N(2, 2100)))],
}
CASES = {"p2100": ("p2100", "plain"), "p2049": ("p2049", "plain"), "p2048": ("p2048", "plain"), "p1025": ("p1025", "plain"),
         "mid2150": ("mid2150", "plain"), "p2100-dup": ("p2100", "dup"), "p2100-schur": ("p2100", "schur"), "p2100-parted": ("p2100", "parted")}


def with_duplicates(A):
    """The lower triangle as a raw CSC (n, colptr, rowval, nzval, 0) in which 300 entries appear twice, as 0.75 v and 0.25 v."""
    A = A.tocsc()
    A.sort_indices()
    n = A.shape[0]
    rng = np.random.default_rng(11)
    cols = np.repeat(np.arange(n), np.diff(A.indptr))
    pick = np.unique(np.concatenate([rng.choice(len(A.data), size=298, replace=False), [0, len(A.data) - 1]]))
    v = A.data.copy()
    v[pick] *= 0.75
    rr = np.concatenate([A.indices, A.indices[pick]]).astype(np.int64)
    cc = np.concatenate([cols, cols[pick]])
    vv = np.concatenate([v, 0.25 * A.data[pick]])
    order = np.lexsort((rr, cc))
    cp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(cp, cc + 1, 1)
    return (n, np.cumsum(cp), rr[order], vv[order], 0)


def run_case(design, mode):
    from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP
    d = ft.build(DESIGNS[design])
    b = ft.rhs(d.n, 1)
    if mode == "parted":
        import parted_trees as pt
        sh = pt.sharded(d, 2)
        r = pt.device_results(sh, d, b)
        return {"d": r["D"], "Lp": r["Lp"], "Li": r["Li"], "Lx": r["Lx"], "x": r["X"][0], "inertia": r["inertia"], "n": np.array(d.n)}
    h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(h)
    if mode == "schur":
        ns = d.nodes[-1]["k"]
        n1pos = int((d.A.diagonal()[d.perm][:d.n - ns] > 0).sum())
        h.set_schur(d.perm[d.n - ns:])
        h.set_perm(d.perm)
        h.analyze(d.A)
        flag = h.ls_factor_schur(d.A, n1pos, d.n - ns - n1pos)
        res = {"flag": np.array(flag), "S": h.schur(), "d": h.diag().copy(), "inertia": np.array(h.inertia)}
        res["sflag"] = np.array(h.schur_factor())
        res["x"] = h.schur_solve(b).reshape(-1)
    else:
        h.set_perm(d.perm)
        flag = h.ls_factor_b(with_duplicates(d.A) if mode == "dup" else d.A, d.npos, d.nneg)
        Lh = h.factor_csc()
        res = {"flag": np.array(flag), "d": h.diag().copy(), "Lp": Lh.indptr, "Li": Lh.indices, "Lx": Lh.data, "x": h.ls_solve(b[0]),
               "inertia": np.array(h.inertia)}
    res["n"] = np.array(d.n)
    finalize_b(h)
    return res


if __name__ == "__main__":
    out, res = sys.argv[1], {}
    for name in sys.argv[2:]:
        print(f"okkt-case: {name}", file=sys.stderr, flush=True)
        res.update({f"{name}/{k}": v for k, v in run_case(*CASES[name]).items()})
    np.savez(out, **res)
    print("CASE_OK")
