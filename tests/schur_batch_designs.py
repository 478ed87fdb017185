"""Scenario batches: the designs, the items and the references shared by test_schur_batch_host.py,
test_gpu_schur_batch.py and schur_batch_case.py.

A design is a forest of front_trees.py whose LAST ROOT is the Schur set (schur_trees.py), every interior front a small front.  One
pattern with the value seeds 0 .. B-1 gives the items of a batch: the pattern and the labelling of front_trees.build do not depend on
the seed.  The sums over the items are evaluated here in NumPy with explicit loops, in the order okkt.h states: groups of
OKKT_SBATCH_GROUP items summed one after the other from 0.0, the groups' partials added left to right, the caller's addend last."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import schur_trees as sct  # noqa: E402
from front_trees import N  # noqa: E402

GROUP = 32
NRHS = (1, 2, 3, 4, 5)          # column groups of 1, 2, 4 and 4 + 1


def _chain(depth):
    nd = N(8, 5)
    for _ in range(depth - 1):
        nd = N(8, 5, nd)
    return nd


def _eight(ns):
    """eight scattered children of small fronts under a set of ns: every column of the Schur front gets several records"""
    return [N(ns, 0, *[N(k, c, scatter=True) for k, c in ((10, 100), (12, 116), (8, 64), (20, 90), (6, 33), (16, 17), (9, 118), (14, 1))])]


# name -> (forest, handle options, batch sizes)
DESIGNS = {
    "set-2-leaf": ([N(2, 0, N(5, 1))], {}, (1, 3, 7, 33, 65)),
    "childless-set": ([N(30, 0, N(20, 10)), N(40), N(17)], {}, (1, 3, 7, 33, 65)),
    "set-65-small-only": (sct.NEW_DESIGNS["set-65-small-only"][0], {}, (1, 3, 7)),
    "set-64-child-136": ([N(64, 0, N(73, 63))], {"small_front_max": 136}, (1, 3, 7)),
    "set-256-eight": (_eight(256), {}, (1, 3, 7)),
    "set-257-eight": (_eight(257), {}, (1, 3, 7)),
    "set-2048-two": ([N(2048, 0, N(20, 100, scatter=True), N(10, 118))], {}, (2,)),
    "three-levels-chain": ([N(9, 0, N(40, 8, *[N(17, 16, *[N(16 + (i % 2), 16) for i in range(20)]) for _ in range(3)]), _chain(5))], {}, (1, 3, 7)),
    "duplicates": ([N(6, 0, N(10, 5, scatter=True), N(7, 3))], {}, (1, 3, 7)),
}


class Scenario:
    """One design as the C ABI takes it: the pattern (lower triangle, raw CSC), the permutation, the set, the value sets of the items."""

    def __init__(self, name):
        self.name = name
        roots, self.opts, self.sizes = DESIGNS[name]
        self.roots = roots
        d = ft.build(roots)
        self.d = d
        A = sp.csc_matrix(d.A)
        self.colptr0, self.rowval0 = A.indptr.astype(np.int64), A.indices.astype(np.int64)
        self.ns = sct.set_size(d)
        self.n1 = d.n - self.ns
        self.dim = d.n
        self.idx = sct.set_index(d)
        self.n1pos = sct.interior_positive(d)
        self.n1neg = self.n1 - self.n1pos
        self.reached = sct.reached(d)
        self.src = np.arange(A.nnz)
        self.frac = np.ones(A.nnz)
        self.colptr, self.rowval = self.colptr0, self.rowval0
        if name == "duplicates":
            self._duplicate()
        self._vals = {}

    def _duplicate(self):
        """every second entry of A21 and A22 split into two halves, one diagonal entry of A22 into three parts: the raw CSC holds
        duplicated entries, which the assembly sums serially in input order (the parts are powers of two: the sums are exact)"""
        inset = np.zeros(self.dim, dtype=bool)
        inset[self.idx] = True
        colptr, rowval, src, frac = [0], [], [], []
        cnt, diag_done = 0, False
        for j in range(self.dim):
            for e in range(self.colptr0[j], self.colptr0[j + 1]):
                i = self.rowval0[e]
                parts = (1.0,)
                if inset[i] or inset[j]:
                    cnt += 1
                    if i == j and inset[i] and not diag_done:
                        parts, diag_done = (0.25, 0.5, 0.25), True
                    elif cnt % 2 == 0:
                        parts = (0.5, 0.5)
                for p in parts:
                    rowval.append(i)
                    src.append(e)
                    frac.append(p)
            colptr.append(len(rowval))
        assert diag_done and len(rowval) > len(self.rowval0)
        self.colptr, self.rowval = np.array(colptr, np.int64), np.array(rowval, np.int64)
        self.src, self.frac = np.array(src), np.array(frac)

    def item_matrix(self, seed):
        """the lower triangle of item `seed` (canonical CSC, the design's labels)"""
        A = sp.csc_matrix(ft.build(self.roots, seed=seed).A)
        assert np.array_equal(A.indptr, self.colptr0) and np.array_equal(A.indices, self.rowval0)
        return A

    def vals(self, B):
        """[B, nnz]: the values of items 0 .. B-1 in the order of the pattern handed to okkt_analyze"""
        for b in range(B):
            if b not in self._vals:
                self._vals[b] = self.item_matrix(b).data[self.src] * self.frac
        return np.ascontiguousarray(np.stack([self._vals[b] for b in range(B)]))

    def matrix(self, vals):
        return (self.dim, self.colptr, self.rowval, np.ascontiguousarray(vals), 0)

    def handle(self, host=False, **more):
        from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP
        opts = dict(ft.NO_RELAX, **self.opts)
        opts.update(more)
        if host:
            opts["host_symbolic_only"] = 1
        h = linear_solver_HIP("symmetric", ordering=2, **opts)
        initialize_b(h)
        h.set_schur(self.idx)
        h.set_perm(self.d.perm)
        h.analyze(self.matrix(np.zeros(len(self.rowval))))
        return h

    def a22(self, seed):
        """A22 of item `seed`, dense, rows and columns in the order of the set"""
        M = ft.full_csr(self.item_matrix(seed))
        return M[self.idx][:, self.idx].toarray()

    def dense_item(self, seed):
        """the whole symmetric matrix of item `seed`, dense, interior (permuted order) then the set"""
        M = ft.full_csr(self.item_matrix(seed))
        return M[self.d.perm][:, self.d.perm].toarray()

    def rhs(self, B, nrhs, seed=0):
        return np.random.default_rng(5000 + seed).normal(size=(B, nrhs, self.dim))


_SC = {}


def scenario(name):
    if name not in _SC:
        _SC[name] = Scenario(name)
    return _SC[name]


def group_sum(items, add=None):
    """((P_0 + P_1) + ... + P_{G-1}) (+ add): P_g the sequential sum from 0.0 over the items of group g, in item order"""
    items = [np.asarray(x, dtype=np.float64) for x in items]
    parts = []
    for g0 in range(0, len(items), GROUP):
        p = np.zeros_like(items[0])
        for x in items[g0:g0 + GROUP]:
            p = p + x
        parts.append(p)
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    if add is not None:
        tot = tot + np.asarray(add, dtype=np.float64)
    return tot


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Equal as bits (NaNs included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def x2_given(sc, nrhs):
    """an x2 for the expansions (any values do: the expansion is compared as bits)"""
    return np.random.default_rng(77).normal(size=(nrhs, sc.ns))


def single_item(sc, vals_b, rhs_b):
    """A fresh single handle in Schur mode on item values vals_b: flag, inertia, D, the stored factor, S, and per block of right-hand
    sides (rhs_b[k]: nrhs x dim) r2 and the expansion of x2_given."""
    from onephase_jl_amd.linear_system_solvers import finalize_b
    h = sc.handle()
    flag = h.ls_factor_schur(np.ascontiguousarray(vals_b), sc.n1pos, sc.n1neg)
    out = dict(flag=int(flag), inertia=h.inertia, D=h.diag(), L=h.factor_csc(), S=h.schur(), r2=[], xe=[])
    for Bk in rhs_b:
        out["r2"].append(h.schur_condense(Bk).reshape(len(Bk), -1))
        out["xe"].append(h.schur_expand(Bk, x2_given(sc, len(Bk))).reshape(len(Bk), -1))
    finalize_b(h)
    return out


def rhs_blocks(sc, item):
    rng = np.random.default_rng(1000 + item)
    return [rng.normal(size=(k, sc.dim)) for k in NRHS]


_REF = {}


def reference(name, B):
    """what fresh single handles make of items 0 .. B-1 (cached, shared, never changed); right-hand sides of every column group for
    the first seven items, one column beyond"""
    sc = scenario(name)
    vals = sc.vals(B)
    for b in range(B):
        if (name, b) not in _REF:
            blocks = rhs_blocks(sc, b)
            _REF[(name, b)] = single_item(sc, vals[b], blocks if b < 7 else blocks[:1])
    return sc, vals, [_REF[(name, b)] for b in range(B)]


def check_items(name, sizes=None):
    """Case 1 of the device tests: every item of every batch size, as bits, against a fresh single handle in Schur mode -- flag, inertia
    and D; S_b; after the select S, r2, the expansion and the stored factor; r2_items; and S_b = A22_b wherever no child reaches."""
    from onephase_jl_amd.linear_system_solvers import finalize_b
    sc = scenario(name)
    sizes = sizes or sc.sizes
    sc, vals, ref = reference(name, max(sizes))
    h = sc.handle()
    q = h.schur_batch_query(nrhs_max=max(NRHS))
    assert q["eligible"] == 1 and q["ns"] == sc.ns, q
    h.schur_batch_reserve(max(sizes), nrhs_max=max(NRHS))
    away = ~sc.reached
    for B in sizes:
        flags = h.ls_factor_schur_batch(vals[:B], sc.n1pos, sc.n1neg)
        assert [int(f) for f in flags] == [ref[b]["flag"] for b in range(B)]
        assert h.schur_batch_inertia == [ref[b]["inertia"] for b in range(B)]
        for k, nrhs in enumerate(NRHS if B <= 7 else NRHS[:1]):
            rhs = np.stack([rhs_blocks(sc, b)[k] for b in range(B)])
            _, items = h.schur_batch_condense(rhs, items=True)
            for b in range(B):
                assert same(items[b], ref[b]["r2"][k]), f"B = {B}, nrhs = {nrhs}: r2 of item {b}"
        picks = range(B) if B <= 7 else (0, 31, 32, B - 1)
        for b in picks:
            Sb = h.schur_batch(b)
            assert same(Sb, ref[b]["S"]), f"B = {B}: S of item {b}"
            assert same(Sb[away], sc.a22(b)[away]), f"B = {B}: an entry of S_{b} that no child reaches is not A22"
        for b in picks:
            h.schur_batch_select(b)
            assert h.inertia == ref[b]["inertia"]
            assert same(h.diag(), ref[b]["D"]), f"D of item {b}"
            Lb = h.factor_csc()
            assert np.array_equal(Lb.indptr, ref[b]["L"].indptr) and np.array_equal(Lb.indices, ref[b]["L"].indices)
            assert same(Lb.data, ref[b]["L"].data), f"the stored factor of item {b}"
            assert same(h.schur(), ref[b]["S"])
            blocks = rhs_blocks(sc, b)
            for k in range(len(ref[b]["r2"])):
                assert same(h.schur_condense(blocks[k]).reshape(len(blocks[k]), -1), ref[b]["r2"][k]), (b, k)
                assert same(h.schur_expand(blocks[k], x2_given(sc, len(blocks[k]))).reshape(len(blocks[k]), -1), ref[b]["xe"][k]), (b, k)
    h.schur_batch_release()
    finalize_b(h)
