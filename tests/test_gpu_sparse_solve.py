"""GPU tests of the sparse right-hand sides: okkt_solve_sparse returns, at the requested entries, the numbers
okkt_solve returns for the densified b -- np.array_equal, no tolerance -- on designed trees (front_trees.py) that put a front on every
route of the sweeps:
  small-classes-f32-33-64-65-128-129   the small-front classes at their edges and the first big (thin) front
  task-chains-under-big                chains of small fronts that run as whole tasks under a big root
  edge-k129-c700                       a mid front (block substitution) under a wide root
  thin-k128-f2049                      the last thin pivot block under a wide root of two 1024-column blocks
  mixed-level-scatter                  thin, mid, wide and small children under one parent, a second root; also with a Ruiz scaling
  fan-in-8                             one child of eight active: seven contribution vectors in the fringe
  deep-chain-6                         six big fronts on one path
Before every sparse call the work vectors are poisoned by an okkt_solve of a dense vector with entries around 1e30: a missing zero (the
fringe, zwork, xwork) then shows as 1e30, not as a rounding difference.  One factored handle per design is shared by the module."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402

pytestmark = pytest.mark.gpu

DESIGNS = ["small-classes-f32-33-64-65-128-129", "task-chains-under-big", "edge-k129-c700", "thin-k128-f2049", "mixed-level-scatter", "fan-in-8",
           "deep-chain-6"]
CASES = [(name, False) for name in DESIGNS] + [("mixed-level-scatter", True)]
IDS = [name + ("+ruiz" if sc else "") for name, sc in CASES]
SUPPORTS = ["leaf", "root", "child", "five", "dense"]


def record(**kw):
    print("SPARSE_SOLVE " + json.dumps(kw))


class Case:
    def __init__(self, name, scaled):
        self.name, self.scaled = name, scaled
        self.d = d = ft.build(ft.DESIGNS[name][0])
        self.h = h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
        initialize_b(h)
        h.set_perm(d.perm)
        if scaled:
            h.set_scaling("ruiz")
        assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
        self.n = d.n
        self.ns = len(d.nodes)
        assert h.stats()["nsuper"] == self.ns
        nodes = d.nodes
        self.kids = {i: [j for j, nd in enumerate(nodes) if nd["parent"] == i] for i in range(self.ns)}
        self.depth = [len(self.closure([i])) for i in range(self.ns)]
        self.poison = np.random.default_rng(99).normal(size=self.n) * 1e30
        self._ref = {}

    def closure(self, starts):
        out = set()
        for i in starts:
            while i is not None and i not in out:
                out.add(i)
                i = self.d.nodes[i]["parent"]
        return out

    def orig(self, i, j=0):
        nd = self.d.nodes[i]
        return int(self.d.perm[nd["col0"] + (j % nd["k"])])

    def support(self, kind, shift=0):
        """(rows, values, nodes that hold them): original indices of the non-zeros of one column"""
        rng = np.random.default_rng(1000 + shift)
        leaves = [i for i in range(self.ns) if not self.kids[i]]
        deepest = max(leaves, key=lambda i: (self.depth[i], -i))
        roots = [i for i in range(self.ns) if self.d.nodes[i]["parent"] is None]
        many = max(range(self.ns), key=lambda i: (len(self.kids[i]), i))
        if kind == "leaf":
            hold = [deepest]
            rows = [self.orig(deepest, 1 + shift)]
        elif kind == "root":
            hold = [roots[-1]]
            rows = [self.orig(roots[-1], 3 + shift)]
        elif kind == "child":
            ch = self.kids[many][(len(self.kids[many]) // 2 + shift) % len(self.kids[many])]
            hold = [ch]
            rows = [self.orig(ch, shift)]
        elif kind == "five":
            # two subtrees: two different children of the node with the most children where it has two, else a leaf and its root
            ks = self.kids[many]
            a, b = (ks[shift % len(ks)], ks[(shift + 1) % len(ks)]) if len(ks) >= 2 else (deepest, roots[-1])
            hold = [a, b]
            rows = list(dict.fromkeys([self.orig(a, 0), self.orig(a, 1), self.orig(a, 2), self.orig(b, 0), self.orig(b, 1)]))
        else:
            hold = list(range(self.ns))
            rows = list(range(self.n))
        vals = rng.normal(size=len(rows)) * 10.0 ** rng.integers(-2, 3, size=len(rows))
        return np.array(rows, dtype=np.int64), vals, hold

    def requests(self, rows, hold):
        """None (all), the support itself, three rows of a subtree disjoint from the support's paths where the tree has one (else of a
        front that holds no non-zero), a list with a duplicate"""
        on_paths = self.closure(hold)
        free = [i for i in range(self.ns) if i not in on_paths] or [i for i in range(self.ns) if i not in hold] or [0]
        f = free[0]
        three = np.array([self.orig(f, 0), self.orig(f, 1), self.orig(f, 2)], dtype=np.int64)
        dup = np.array([rows[0], three[0], rows[0]], dtype=np.int64)
        return {"all": None, "support": rows[:64], "disjoint": three, "duplicate": dup}

    def dense(self, rows, vals):
        b = np.zeros(self.n)
        b[rows] = vals
        return b

    def solve(self, B):
        B = np.ascontiguousarray(np.atleast_2d(B))
        X = np.zeros_like(B)
        self.h._check(self.h._lib.okkt_solve(self.h._h, L.p_f64(B), L.p_f64(X), B.shape[0]), "okkt_solve")
        return X

    def reference(self, key, rows, vals):
        if key not in self._ref:
            self._ref[key] = self.solve(self.dense(rows, vals))[0]
        return self._ref[key]

    def do_poison(self):
        x = self.solve(self.poison)
        assert np.max(np.abs(x)) > 1e25


_CASES = {}


def case(name, scaled=False):
    if (name, scaled) not in _CASES:
        _CASES[(name, scaled)] = Case(name, scaled)
    return _CASES[(name, scaled)]


def matrix_of(c, columns):
    """scipy CSC with one right-hand side per column from [(rows, vals), ...]"""
    r = np.concatenate([rows for rows, _ in columns])
    v = np.concatenate([vals for _, vals in columns])
    ptr = np.concatenate([[0], np.cumsum([len(rows) for rows, _ in columns])])
    M = sp.csc_matrix((v, r, ptr), shape=(c.n, len(columns)))
    M.sort_indices()
    return M


@pytest.mark.parametrize("kind", SUPPORTS)
@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_sparse_solve_is_the_dense_solve_at_the_requested_entries(name, scaled, kind):
    c = case(name, scaled)
    rows, vals, hold = c.support(kind)
    ref = c.reference(kind, rows, vals)
    assert np.all(np.isfinite(ref)) and np.any(ref != 0.0)
    for what, want in c.requests(rows, hold).items():
        c.do_poison()
        x, info = c.h.ls_solve_sparse((rows, vals), want)
        expect = ref if want is None else ref[want]
        assert x.shape == expect.shape
        assert np.array_equal(x, expect), (name, kind, what, float(np.max(np.abs(x - expect))))
        assert info["batches"] == 1 and info["nsuper"] == c.ns
        # the sets are those of the host call
        hinfo, _ = c.h.sparse_reach(rows, want)
        for k in ("fwd_reach", "bwd_reach", "fwd_run", "bwd_run", "fringe", "fringe_entries", "fwd_panel_bytes", "bwd_panel_bytes", "pruned"):
            assert info[k] == hinfo[k], (k, what)
        if kind == "dense" and want is None:
            assert info["pruned"] == 0
        if kind == "root":
            assert info["pruned"] == 1 and info["fwd_run"] == 1 < c.ns and info["fwd_panel_bytes"] < info["factor_panel_bytes"]


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_batches_of_columns_with_different_supports(name, scaled):
    c = case(name, scaled)
    kinds = ["leaf", "root", "child", "five", "leaf", "child", "five"]
    cols = [c.support(k, shift=q)[:2] for q, k in enumerate(kinds)]
    want = np.array([c.orig(0, 0), c.orig(c.ns - 1, 0), c.orig(c.ns // 2, 1), c.orig(0, 0)], dtype=np.int64)
    singles, dense = [], []
    for rows, vals in cols:
        c.do_poison()
        singles.append(c.h.ls_solve_sparse((rows, vals), None)[0])
        dense.append(c.solve(c.dense(rows, vals))[0])
        assert np.array_equal(singles[-1], dense[-1])
    for nrhs in (1, 2, 3, 4, 5, 7):
        B = matrix_of(c, cols[:nrhs])
        for w in (None, want):
            c.do_poison()
            X, info = c.h.ls_solve_sparse(B, w)
            assert X.shape == (nrhs, c.n if w is None else len(w)) and info["batches"] == (nrhs + 3) // 4
            for q in range(nrhs):
                assert np.array_equal(X[q], singles[q] if w is None else singles[q][w]), (nrhs, q)
    # an empty column between two others is a zero column
    B = matrix_of(c, [cols[0], (np.zeros(0, dtype=np.int64), np.zeros(0)), cols[1]])
    c.do_poison()
    X, _ = c.h.ls_solve_sparse(B, want)
    assert np.array_equal(X[0], singles[0][want]) and np.array_equal(X[2], singles[1][want]) and not X[1].any()
    # all columns empty, all rows
    c.do_poison()
    X, info = c.h.ls_solve_sparse(sp.csc_matrix((c.n, 2)), None)
    assert X.shape == (2, c.n) and not X.any() and info["fwd_reach"] == 0


@pytest.mark.parametrize("name,scaled", [("mixed-level-scatter", False), ("mixed-level-scatter", True), ("task-chains-under-big", False)],
                         ids=["mixed", "mixed+ruiz", "tasks"])
def test_device_form_determinism_and_the_ordinary_solve_unchanged(name, scaled):
    c = case(name, scaled)
    h = c.h
    kinds = ["five", "leaf", "root", "child", "five"]
    cols = [c.support(k, shift=3 + q)[:2] for q, k in enumerate(kinds)]
    B = matrix_of(c, cols)
    want = np.array([c.orig(1, 0), c.orig(c.ns - 1, 2), c.orig(1, 0)], dtype=np.int64)
    probe = ft.rhs(c.n, 3, seed=31)
    before = c.solve(probe)
    c.do_poison()
    X1, _ = h.ls_solve_sparse(B, want)
    after = c.solve(probe)
    assert after.tobytes() == before.tobytes()
    c.do_poison()
    X2, _ = h.ls_solve_sparse(B, want)
    assert X1.tobytes() == X2.tobytes()
    # values and result in device memory
    d_val = h.dev_upload(np.ascontiguousarray(B.data))
    for w in (want, None):
        nx = c.n if w is None else len(w)
        d_out = h.dev_alloc(8 * len(cols) * nx)
        c.do_poison()
        info = h.ls_solve_sparse_dev(B.indptr, B.indices, d_val, d_out, w)
        got = h.dev_download(d_out, (len(cols), nx))
        h.dev_free(d_out)
        host, _ = h.ls_solve_sparse(B, w)
        assert np.array_equal(got, host) and info["batches"] == 2 and info["seconds_device"] > 0
        if w is not None:
            assert got.tobytes() == X1.tobytes()
    h.dev_free(d_val)
    # nothing to do
    lib = h._lib
    cp = np.zeros(1, dtype=np.int64)
    assert lib.okkt_solve_sparse(h._h, 0, L.p_i64(cp), None, None, 0, None, None, None) == L.OKKT_OK
    out = np.full(4, 7.0)
    xi = np.zeros(1, dtype=np.int64)
    b = matrix_of(c, cols[:1])
    assert lib.okkt_solve_sparse(h._h, 1, L.p_i64(L.i64(b.indptr)), L.p_i64(L.i64(b.indices)), L.p_f64(L.f64(b.data)), 0, L.p_i64(xi), L.p_f64(out),
                                 None) == L.OKKT_OK
    assert np.all(out == 7.0)
    assert c.solve(probe).tobytes() == before.tobytes()


@pytest.mark.parametrize("name,scaled", CASES, ids=IDS)
def test_inverse_columns_and_block(name, scaled):
    c = case(name, scaled)
    h = c.h
    idx = np.array([c.orig(i, j) for i in (0, c.ns // 2, c.ns - 1) for j in (0, 1)], dtype=np.int64)
    E = np.zeros((len(idx), c.n))
    E[np.arange(len(idx)), idx] = 1.0
    ref = c.solve(E)                       # row j: F^-1 e_idx[j]
    rows = np.array([c.orig(c.ns - 1, 5), c.orig(0, 0), c.orig(0, 0), c.orig(c.ns // 2, 2)], dtype=np.int64)
    c.do_poison()
    Z, info = h.inverse_columns(idx, rows, with_info=True)
    assert Z.shape == (len(rows), len(idx)) and info["batches"] == 2
    assert np.array_equal(Z, ref[:, rows].T)
    c.do_poison()
    Zall = h.inverse_columns(idx[:2])
    assert np.array_equal(Zall, ref[:2].T)
    d_out = h.dev_alloc(8 * len(idx) * len(rows))
    c.do_poison()
    h.inverse_columns_dev(idx, d_out, rows)
    assert np.array_equal(h.dev_download(d_out, (len(idx), len(rows))).T, Z)
    h.dev_free(d_out)
    # the block: symmetric up to the forward error of the two unit solves
    c.do_poison()
    Zb = h.inverse_block(idx)
    assert np.array_equal(Zb, ref[:, idx].T)
    ferr, _ = h.forward_error(c.d.A, E, ref)
    defect = np.abs(Zb - Zb.T)
    bound = np.abs(Zb) * (ferr[None, :] + ferr[:, None])
    frac = float(np.max(np.where(defect > 0, defect / np.where(bound > 0, bound, 1.0), 0.0)))
    record(test="inverse_block", case=name, scaled=scaled, max_defect=float(defect.max()), max_ferr=float(ferr.max()), worst_fraction_of_bound=frac)
    assert np.all(defect <= bound), frac


def test_of_kkt_on_a_synthetic_system():
    """The level-1 handle of a KKT solver: the sparse solve is the dense solve of the matrix okkt_kkt_factor last factored."""
    prob = synth.make_config("S-small", seed=5, well_scaled=True)
    rng = np.random.default_rng(2)
    it = KS.Class_iterate(x=rng.normal(size=prob["n"]), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                          grad=rng.normal(size=prob["n"]), cons=prob["s"] + 0.1 * rng.normal(size=prob["m"]), a_norm_penalty_par=1e-4)
    k = KS.HIP_KKT_solver("symmetric", KS.Class_parameters())
    k.initialize_b(it)
    k.form_system_b(it)
    assert k.factor_b(1e-2) == 1
    ls = linear_solver_HIP.of_kkt(k)
    n = k.matrix().shape[0]
    assert 200 <= n <= 1000
    poison = rng.normal(size=n) * 1e30
    for trial in range(4):
        rows = rng.choice(n, size=1 + 2 * trial, replace=False).astype(np.int64)
        vals = rng.normal(size=len(rows))
        want = rng.choice(n, size=5, replace=True).astype(np.int64)
        b = np.zeros(n)
        b[rows] = vals
        ref = ls.ls_solve(b)
        ls.ls_solve(poison)
        x, info = ls.ls_solve_sparse((rows, vals), want)
        assert np.array_equal(x, ref[want]), trial
        ls.ls_solve(poison)
        xa, _ = ls.ls_solve_sparse((rows, vals))
        assert np.array_equal(xa, ref)
        hinfo, act = ls.sparse_reach(rows, want)
        assert hinfo["fwd_run"] == info["fwd_run"] and hinfo["bwd_run"] == info["bwd_run"]
    ls.ls_solve(poison)
    Z = ls.inverse_block(want)
    E = np.zeros((len(want), n))
    E[np.arange(len(want)), want] = 1.0
    assert np.array_equal(Z, np.array([ls.ls_solve(e) for e in E])[:, want].T)
    ls._finalize()


def test_refusals_that_need_a_device():
    d = ft.build(ft.DESIGNS["mixed-level-scatter"][0])
    h = linear_solver_HIP("symmetric", ordering=2, **ft.NO_RELAX)
    initialize_b(h)
    h.set_perm(d.perm)
    h.analyze(d.A)
    rows, vals = np.array([3, 9], dtype=np.int64), np.array([1.0, -2.0])

    def refused(hh, word):
        with pytest.raises(OkktError, match=word):
            hh.ls_solve_sparse((rows, vals), [0, 1])
        with pytest.raises(OkktError, match=word):
            hh.inverse_columns([0, 1], [2])
        d_v = hh.dev_upload(vals)
        d_o = hh.dev_alloc(64)
        try:
            with pytest.raises(OkktError, match=word):
                hh.ls_solve_sparse_dev([0, 2], rows, d_v, d_o, [0, 1])
            with pytest.raises(OkktError, match=word):
                hh.inverse_columns_dev([0, 1], d_o, [2])
        finally:
            hh.dev_free(d_v)
            hh.dev_free(d_o)

    # before a factorisation (the reach needs none)
    refused(h, "complete factorisation")
    assert h.sparse_reach(rows)[0]["fwd_reach"] >= 1
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
    b = np.zeros(d.n)
    b[rows] = vals
    x = h.ls_solve(b)
    assert np.array_equal(h.ls_solve_sparse((rows, vals))[0], x)
    # bad arguments on a factored handle leave it usable
    with pytest.raises(OkktError, match="twice"):
        h.ls_solve_sparse((np.array([3, 3]), vals))
    with pytest.raises(OkktError, match="out of range"):
        h.ls_solve_sparse((rows, vals), [d.n])
    assert np.array_equal(h.ls_solve_sparse((rows, vals), [5, 5])[0], x[[5, 5]])
    # after an early exit that stopped short
    h._check(h._lib.okkt_set_early_exit(h._h, 1), "okkt_set_early_exit")
    if h.ls_factor_b(d.A, d.nneg, d.npos) == 0 and h._lib.okkt_solve(h._h, L.p_f64(b), L.p_f64(np.zeros(d.n)), 1) == L.OKKT_ERR_INVALID:
        refused(h, "complete factorisation")
    h._check(h._lib.okkt_set_early_exit(h._h, 0), "okkt_set_early_exit")
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == 1
    assert np.array_equal(h.ls_solve_sparse((rows, vals))[0], x)
    assert h.ls_solve(b).tobytes() == x.tobytes()
    finalize_b(h)
    # Schur mode
    h = linear_solver_HIP("symmetric", **ft.NO_RELAX)
    initialize_b(h)
    h.set_schur([0, 1])
    h.analyze(d.A)
    sg = np.sign(d.A.diagonal()[[0, 1]])
    assert h.ls_factor_schur(d.A, d.npos - int(np.sum(sg > 0)), d.nneg - int(np.sum(sg < 0))) in (0, 1)
    refused(h, "Schur mode")
    with pytest.raises(OkktError, match="Schur mode"):
        h.sparse_reach(rows)
    finalize_b(h)
