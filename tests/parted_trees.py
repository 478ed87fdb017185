"""The partitioned (subtree-sharded) factor and solve on designed cuts of the tree: the catalogue and the helpers shared by
test_parted_trees.py, test_gpu_parted_trees.py and parted_trees_case.py.

A design is a forest of front_trees.py; the handle gets `ordering = 2`, `set_perm(d.perm)` and `NO_RELAX`, so the fronts are the
designed ones, and the flops of the designed fronts decide where `partition_tree` cuts.  For every design and number of parts the
catalogue holds the cut it was designed for: the owner of every front in postorder (-1: the top, factored by part 0 behind the
exchange), the number of boundary fronts (owned fronts whose parent is in the top) and the doubles of their contribution blocks.
test_parted_trees.py holds the partitioner to this table on a host_symbolic_only handle, so that no GPU time goes into a cut that
is not the designed one and a later change of `partition_tree` cannot move one unnoticed.

What a partitioned plan does that no other plan does, and which design makes it happen:
  * tasks of small fronts must not cross the cut, flow launches stop at it        small-subtrees-under-big-top, small-top-over-small-parts
  * the top: absent / one wide front / two levels / small fronts only             forest-no-top, deep-chain-6 / wide-top-1100 / two-level-top-4 / small-top-*
  * boundary fronts of every class (k = 1, small of each LDS class, thin, mid, wide, scattered)    thin-boundary-*, small-classes-under-top, cut-mid-wide, fan-in-8
  * a wide front in part 0 (one inverse event) and in a part > 0 (events per level)                 two-wide-subtrees
  * empty parts                                                                   every design with more parts than subtrees
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import front_trees as ft
import oracle
from front_trees import N, _chain_small as chain
from onephase_jl_amd import _lib as L
from onephase_jl_amd.distributed import LocalComm, ShardedLinearSolver
from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP

SMALL_MAX = 128        # the default small_front_max
NRHS = 2


def _D(forest, cuts, n_boundary, cb_doubles, what):
    return dict(forest=forest, cuts=cuts, n_boundary=n_boundary, cb_doubles=cb_doubles, what=what)


# name -> forest, {nparts: owners in postorder}, n_boundary, cb_doubles (the same at every nparts of a design), what it is for
DESIGNS = {
    "cut-mid-wide": _D(
        [N(260, 0, N(300, 150, N(140, 300)), N(500, 250, N(129, 400)))],
        {2: [1, 1, 0, 0, -1], 3: [1, 1, 0, 0, -1]}, 2, 85000,
        "a mid and a wide boundary front, two-front subtrees, an empty part at 3"),
    "wide-top-1100": _D(
        [N(1100, 0, N(200, 700), N(129, 1000, scatter=True))],
        {2: [1, 0, -1]}, 2, 1490000,
        "top = one wide front (1024-column inverse + padded block on the auxiliary stream), 62 % of the flops in the top"),
    "two-wide-subtrees": _D(
        [N(300, 0, N(1100, 200), N(1025, 150, scatter=True))],
        {2: [1, 0, -1]}, 2, 62500,
        "a wide front in part 0 (single inverse event) and one in part 1 (per-level events)"),
    "two-level-top-4": _D(
        [N(200, 0, N(150, 190, N(300, 330, N(200, 400)), N(280, 339, N(220, 380), scatter=True)),
           N(160, 180, N(250, 300), N(240, 320)))],
        {2: [1, 1, 1, 0, 0, 1, 1, -1, -1], 3: [2, 2, 2, 0, 0, 1, 1, -1, -1], 4: [2, 2, 2, 0, 0, 1, 1, -1, -1]}, 3, 256221,
        "two top levels, boundary fronts that feed different top fronts at different levels, part 3 empty at 4"),
    "small-subtrees-under-big-top": _D(
        [N(300, 0, chain(8), chain(6), N(24, 8), N(40, 60), N(150, 120))],
        {2: [1] * 16 + [0, -1], 4: [3] + [2] * 8 + [3] * 6 + [1, 0, -1], 8: [4] + [2] * 8 + [3] * 6 + [1, 0, -1]}, 5, 18576,
        "boundary fronts that are roots of small-front tasks and flow launches; parts made of tasks only; parts 5-7 empty at 8"),
    "small-classes-under-top": _D(
        [N(200, 0, *[N(f - 16, 16) for f in (32, 33, 64, 65, 128, 129)], N(150, 120))],
        {2: [1] * 6 + [0, -1], 8: [6, 5, 4, 3, 2, 1, 0, -1]}, 7, 15936,
        "a part that is one small front of each LDS class; fold rule under the owner filter; part 7 empty at 8"),
    "small-top-2-levels": _D(
        [N(20, 0, N(30, 19, N(200, 40), N(180, 45, scatter=True)))],
        {2: [0, 1, -1, -1]}, 2, 3625,
        "a top of small fronts only, two levels"),
    "forest-no-top": _D(
        [N(500), N(1100), N(300, 0, N(200, 150))],
        {2: [1, 0, 1, 1], 3: [1, 0, 2, 2], 4: [1, 0, 2, 2]}, 0, 0,
        "no top, no boundary, zero-length exchanges, part 3 empty at 4"),
    "deep-chain-6": _D(
        ft.DESIGNS["deep-chain-6"][0],
        {2: [0] * 6}, 0, 0,
        "nothing to cut: everything in part 0, part 1 empty"),
    "fan-in-8": _D(
        ft.DESIGNS["fan-in-8"][0],
        {3: [0, 1, 1, 2, 1, 2, 0, 2, -1], 8: [6, 7, 1, 2, 4, 5, 0, 3, -1]}, 8, 681226,
        "eight boundary CBs, half of them scattered, one per part at 8"),
    "mixed-level-scatter": _D(
        ft.DESIGNS["mixed-level-scatter"][0],
        {2: [1, 1, 1, 0, -1, 1], 4: [3, 2, 3, 0, -1, 1]}, 4, 125064,
        "thin, mid, wide and small boundary fronts, plus a separate root owned by a part"),
    "thin-boundary-k1-2-127-128": _D(
        [N(701, 0, N(1, 700), N(2, 700), N(127, 700), N(128, 700))],
        {2: [0, 1, 1, 0, -1], 4: [3, 2, 1, 0, -1]}, 4, 1960000,
        "k = 1, 2, 127, 128 boundary fronts with 700-row CBs"),
    # the one cut at which the owner test of the task rule decides: the top front is small and so are the boundary fronts below it,
    # so without the test the whole tree is one task that part 0 runs in its top schedule and nobody runs for part 1
    "small-top-over-small-parts": _D(
        [N(16, 0, N(8, 12, N(8, 10)), N(10, 14, N(6, 9)))],
        {2: [1, 1, 0, 0, -1]}, 2, 340,
        "a small top front over small boundary fronts: a task of small fronts would cross the cut"),
}

CASES = [(name, nparts) for name, v in DESIGNS.items() for nparts in v["cuts"]]
# the cases the subprocess runs under the other routes
VARIANT_CASES = [("cut-mid-wide", 2), ("two-level-top-4", 3), ("small-subtrees-under-big-top", 4), ("wide-top-1100", 2),
                 ("small-top-over-small-parts", 2)]


def case_id(case):
    return f"{case[0]}/{case[1]}"


def build(name, values="plain", seed=0):
    return ft.build(DESIGNS[name]["forest"], values=values, seed=seed)


# ---- what a cut looks like (host only: from the design and the owners) ---------------------------------------------------------------
def boundary_of(d, owners):
    """the boundary fronts (postorder indices): owned, with a parent in the top"""
    return [i for i, nd in enumerate(d.nodes) if owners[i] >= 0 and nd["parent"] is not None and owners[nd["parent"]] == -1]


def cb_rows(nd):
    return nd["f"] - nd["k"]


def slots(d, owners):
    """(front, r, offset in the cb buffer, offset in the cv buffer) of every boundary front, in postorder"""
    out, ocb, ocv = [], 0, 0
    for i in boundary_of(d, owners):
        r = cb_rows(d.nodes[i])
        out.append((i, r, ocb, ocv))
        ocb += r * r
        ocv += r
    return out, ocb, ocv


def subtree_cols(d, i):
    """the pivot columns of front i and of everything below it: one range (the fronts are numbered in postorder)"""
    lo = [nd["col0"] for nd in d.nodes]
    for j, nd in enumerate(d.nodes):
        if nd["parent"] is not None:
            lo[nd["parent"]] = min(lo[nd["parent"]], lo[j])
    return lo[i], d.nodes[i]["col0"] + d.nodes[i]["k"]


def col_owner(d, owners):
    co = np.zeros(d.n, dtype=np.int64)
    for nd, o in zip(d.nodes, owners):
        co[nd["col0"]:nd["col0"] + nd["k"]] = o
    return co


def top_levels(d, owners):
    """number of levels of the top (0: no top)"""
    h = [0] * len(d.nodes)
    for i, nd in enumerate(d.nodes):
        if owners[i] != -1:
            continue
        h[i] = max(h[i], 1)
        if nd["parent"] is not None:
            h[nd["parent"]] = max(h[nd["parent"]], h[i] + 1)
    return max(h)


def front_class(nd):
    k, f = nd["k"], nd["f"]
    if f <= 32:
        return "f<=32"
    if f <= 64:
        return "f<=64"
    if f <= SMALL_MAX:
        return "f<=128"
    return "thin" if k <= 128 else "mid" if k <= 384 else "wide"


def is_scattered(nd):
    cb = nd["rows"][nd["k"]:]
    return len(cb) > 1 and bool(np.any(np.diff(cb) > 1))


# ---- handles ------------------------------------------------------------------------------------------------------------------------
def host_cut(d, nparts, part_id=0):
    """The cut of a host_symbolic_only handle: (handle, owners per supernode, column owners, parents, info)."""
    s = linear_solver_HIP("symmetric", host_symbolic_only=1, ordering=2, **ft.NO_RELAX)
    initialize_b(s)
    s.set_perm(d.perm)
    s.analyze(d.A)
    s._check(s._lib.okkt_dist_set_partition(s._h, nparts, part_id), "okkt_dist_set_partition")
    ns = s.stats()["nsuper"]
    sn, col, par = np.zeros(ns, dtype=np.int64), np.zeros(d.n, dtype=np.int64), np.zeros(ns, dtype=np.int64)
    s._check(s._lib.okkt_dist_get_owner(s._h, L.p_i64(sn), L.p_i64(col), L.p_i64(par)), "okkt_dist_get_owner")
    cb, cv, nb, tf = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
    pf = np.zeros(nparts)
    s._check(s._lib.okkt_dist_info(s._h, C.byref(cb), C.byref(cv), C.byref(nb), L.p_f64(pf), C.byref(tf)), "okkt_dist_info")
    return s, sn, col, par, dict(cb_doubles=cb.value, cv_doubles=cv.value, n_boundary=nb.value, part_flops=pf.tolist(), top_flops=tf.value)


class RecordingComm(LocalComm):
    """LocalComm that keeps a copy of every rank's buffer at each reduce_sum and broadcast, before doing it:
    log = [(kind, root, [rank 0's buffer, rank 1's, ...]), ...] in the order of the calls."""

    def __init__(self, nparts):
        super().__init__(nparts)
        self.log = []

    def reduce_sum(self, bufs, dst=0):
        self.log.append(("reduce", dst, [b.download().copy() for b in bufs]))
        super().reduce_sum(bufs, dst)

    def broadcast(self, bufs, src=0):
        self.log.append(("broadcast", src, [b.download().copy() for b in bufs]))
        super().broadcast(bufs, src)


def sharded(d, nparts, **opts):
    """An analysed ShardedLinearSolver of the design: nparts virtual ranks on one device, every exchange recorded."""
    sh = ShardedLinearSolver(RecordingComm(nparts), "symmetric", ordering=2, **dict(ft.NO_RELAX, **opts))
    for s in sh.solvers:
        s.set_perm(d.perm)
    sh.analyze(d.A)
    return sh


def composed_factor(sh):
    """D and L of the whole factor (permuted numbering): column j from the solver of col_owner[j], the top from solver 0.  Read
    through diag() and factor_csc() behind okkt_dist_finish; what a solver holds for fronts it does not own is never used."""
    _, col, _ = sh.owners()
    src = np.where(col < 0, 0, col)
    n = sh.dim
    D = np.zeros(n)
    indptr = data = indices = None
    for p, s in enumerate(sh.solvers):
        mine = src == p
        if not mine.any():
            continue
        D[mine] = s.diag()[mine]
        Lp = s.factor_csc()
        if data is None:
            indptr, indices, data = Lp.indptr.copy(), Lp.indices.copy(), np.zeros_like(Lp.data)
        assert np.array_equal(Lp.indptr, indptr) and np.array_equal(Lp.indices, indices)
        entry = np.repeat(mine, np.diff(indptr))
        data[entry] = Lp.data[entry]
    return D, sp.csc_matrix((data, indices, indptr), shape=(n, n))


def device_results(sh, d, B):
    """One partitioned factorisation and the solves of the rows of B one at a time, each twice: the flag, the summed pivot counts,
    the composed D and L, the solutions, the repeated solutions and every rank's buffer in front of each exchange
    (cb: the factor's reduce; cv/i, x/i, sol/i: the reduce, broadcast and reduce of the first solve of right-hand side i)."""
    log = sh.comm.log
    vals = [s.dev_upload(d.A.data) for s in sh.solvers]
    del log[:]
    flag = sh.factor(vals, d.npos, d.nneg)
    assert [e[:2] for e in log] == [("reduce", 0)], [e[:2] for e in log]
    res = {"flag": np.array(flag), "inertia": np.array(sh.inertia), "cb": np.array(log[0][2])}
    D, Lh = composed_factor(sh)
    res.update(D=D, Lp=Lh.indptr, Li=Lh.indices, Lx=Lh.data)
    X, again = [], []
    for i, b in enumerate(B):
        rhs = [s.dev_upload(b) for s in sh.solvers]
        del log[:]
        X.append(sh.solve(rhs))
        assert [e[:2] for e in log] == [("reduce", 0), ("broadcast", 0), ("reduce", 0)], [e[:2] for e in log]
        res[f"cv/{i}"], res[f"x/{i}"], res[f"sol/{i}"] = (np.array(e[2]) for e in log)
        again.append(sh.solve(rhs))
        for s, p in zip(sh.solvers, rhs):
            s.dev_free(p)
    for s, p in zip(sh.solvers, vals):
        s.dev_free(p)
    res.update(X=np.array(X), X_again=np.array(again))
    return res


def wrong_then_right(sh, d, B):
    """A factorisation that is asked for the wrong inertia and, right behind it with no solve in between, the right one:
    (flag and counts of the wrong one, D, L values and solutions of the right one)."""
    vals = [s.dev_upload(d.A.data) for s in sh.solvers]
    flag = sh.factor(vals, d.npos + 1, d.nneg - 1)
    counts = sh.inertia
    flag2 = sh.factor(vals, d.npos, d.nneg)
    D, Lh = composed_factor(sh)
    X = []
    for b in B:
        rhs = [s.dev_upload(b) for s in sh.solvers]
        X.append(sh.solve(rhs))
        for s, p in zip(sh.solvers, rhs):
            s.dev_free(p)
    for s, p in zip(sh.solvers, vals):
        s.dev_free(p)
    return dict(wrong_flag=np.array(flag), wrong_inertia=np.array(counts), right_flag=np.array(flag2), right_inertia=np.array(sh.inertia),
                right_D=D, right_Lx=Lh.data, right_X=np.array(X))


# ---- the reference --------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, **kw):
        self.__dict__.update(kw)


_REF = {}


def reference(name):
    """The design ("plain" values), the oracle's factor on the design's permutation, the right-hand sides, the true solutions
    (the oracle's, refined with long-double residuals) and the oracle's own forward error; cached, nobody changes it."""
    if name not in _REF:
        d = build(name)
        o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
        assert o.ls_factor_b(d.A, d.npos, d.nneg) == 1
        M = ft.full_csr(d.A)
        B = ft.rhs(d.n, NRHS)
        XT = np.array([ft.true_solution(M, o.ls_solve, b) for b in B])
        e_oracle = max(ft.fwd_err(o.ls_solve(b), xt) for b, xt in zip(B, XT))
        _REF[name] = Ref(name=name, d=d, o=o, M=M, B=B, XT=XT, e_oracle=e_oracle, D=o.diag(), L=o.L().tocsr())
    return _REF[name]
