"""Host-side tests of the sparse right-hand sides: the symbols and the struct, every refusal on a handle
without a device, and okkt_sparse_reach -- the sets a pruned solve would use -- on designed trees (front_trees.py, built without
amalgamation, so that the designed nodes are the supernodes) and on a synthetic KKT pattern with the default amalgamation.

The expected sets are computed here from the designs' own parent links (Built.nodes), not typed in: the forward set is the closure of
the node that holds the non-zero, the fringe is every child of a node of the set that is not in it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["okkt_solve_sparse", "okkt_solve_sparse_dev", "okkt_get_inverse_columns", "okkt_get_inverse_columns_dev", "okkt_sparse_reach"]


def host_handle(A=None, perm=None, **opts):
    h = linear_solver_HIP("symmetric", host_symbolic_only=1, **opts)
    initialize_b(h)
    if perm is not None:
        h.set_perm(perm)
    if A is not None:
        h.analyze(A)
    return h


def designed(name):
    d = ft.build(ft.DESIGNS[name][0])
    h = host_handle(d.A, d.perm, ordering=2, **ft.NO_RELAX)
    assert h.stats()["nsuper"] == len(d.nodes)
    return d, h


def closure(d, starts):
    out = set()
    for i in starts:
        while i is not None and i not in out:
            out.add(i)
            i = d.nodes[i]["parent"]
    return out


def fringe_of(d, active):
    return [i for i, nd in enumerate(d.nodes) if nd["parent"] in active and i not in active]


def node(d, k, c):
    """The index of the designed node with k pivots and c contribution rows (the first in postorder)."""
    return next(i for i, nd in enumerate(d.nodes) if nd["k"] == k and nd["f"] - nd["k"] == c)


def orig(d, i, j=0):
    """Original index of pivot column j of node i."""
    return int(d.perm[d.nodes[i]["col0"] + j])


def columns(d, nodes_):
    m = np.zeros(d.n, dtype=bool)
    for i in nodes_:
        m[d.nodes[i]["col0"]:d.nodes[i]["col0"] + d.nodes[i]["k"]] = True
    return m


def test_symbols_signatures_and_struct():
    lib = L.load()
    txt = open(os.path.join(ROOT, "include", "okkt.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name + " is not declared in include/okkt.h"
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # ten int64, two int32, one double, no padding
    assert C.sizeof(L.OkktSparseInfo) == 10 * 8 + 2 * 4 + 8
    m = re.search(r"typedef struct \{([^}]*)\} okkt_sparse_info;", txt)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == [f for f, _ in L.OkktSparseInfo._fields_]


def _sparse(lib, h, nrhs, colptr, rowidx, val, nx, xidx, out, info=True, fn="okkt_solve_sparse"):
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dtype=dt)
    cp, ri, xi = arr(colptr, np.int64), arr(rowidx, np.int64), arr(xidx, np.int64)
    va = arr(val, np.float64)
    inf = L.OkktSparseInfo()
    rc = getattr(lib, fn)(h, nrhs, None if cp is None else L.p_i64(cp), None if ri is None else L.p_i64(ri),
                          None if va is None else (L.p_f64(va) if fn == "okkt_solve_sparse" else C.c_void_p(va.ctypes.data)), nx,
                          None if xi is None else L.p_i64(xi),
                          None if out is None else (L.p_f64(out) if fn == "okkt_solve_sparse" else C.c_void_p(out.ctypes.data)),
                          C.byref(inf) if info else None)
    return rc, lib.okkt_last_error(h).decode()


@pytest.mark.parametrize("fn", ["okkt_solve_sparse", "okkt_solve_sparse_dev"])
def test_refusals_without_a_device(fn):
    lib = L.load()
    d, h = designed("deep-chain-6")
    n = d.n
    out = np.zeros(4 * n)
    ok = dict(nrhs=2, colptr=[0, 2, 3], rowidx=[0, 5, 7], val=[1.0, 2.0, 3.0], nx=2, xidx=[1, 1], out=out)

    def call(**over):
        a = dict(ok, **over)
        return _sparse(lib, h._h, a["nrhs"], a["colptr"], a["rowidx"], a["val"], a["nx"], a["xidx"], a["out"], fn=fn)

    assert getattr(lib, fn)(None, 0, None, None, None, 0, None, None, None) == L.OKKT_ERR_INVALID
    # valid arguments (a duplicate in x_idx is allowed) reach the device gate
    rc, msg = call()
    assert rc == L.OKKT_ERR_NO_DEVICE and "host_symbolic_only" in msg
    rc, msg = call(xidx=None)
    assert rc == L.OKKT_ERR_NO_DEVICE
    bad = {
        "nrhs < 0": dict(nrhs=-1),
        "nx < 0": dict(nx=-1),
        "colptr NULL": dict(colptr=None),
        "rowidx NULL": dict(rowidx=None),
        "val NULL": dict(val=None),
        "x_out NULL": dict(out=None),
        "colptr decreases": dict(colptr=[0, 3, 2]),
        "colptr[0] < 0": dict(colptr=[-1, 2, 3]),
        "row out of range (high)": dict(rowidx=[0, 5, n]),
        "row out of range (low)": dict(rowidx=[0, -1, 7]),
        "requested row out of range": dict(xidx=[1, n]),
        "requested row negative": dict(xidx=[-1, 1]),
        "duplicate row in one column": dict(rowidx=[5, 5, 7]),
    }
    for what, over in bad.items():
        rc, msg = call(**over)
        assert rc == L.OKKT_ERR_INVALID, (what, rc, msg)
        assert msg, what
    # the same row in two columns is no duplicate
    rc, _ = call(rowidx=[0, 5, 5])
    assert rc == L.OKKT_ERR_NO_DEVICE
    # the handle stays usable
    info, _ = h.sparse_reach([0])
    assert info["fwd_reach"] >= 1
    finalize_b(h)


def test_refusals_of_the_other_entries_and_modes():
    lib = L.load()
    d, h = designed("deep-chain-6")
    n = d.n
    out = np.zeros(2 * n)
    cols = np.array([0, 3], dtype=np.int64)
    rows = np.array([1, 2, 2], dtype=np.int64)
    inf = L.OkktSparseInfo()

    def inv(fn, ncols, c, nrows, r, o):
        po = None if o is None else (L.p_f64(o) if fn.endswith("columns") else C.c_void_p(o.ctypes.data))
        rc = getattr(lib, fn)(h._h, ncols, None if c is None else L.p_i64(c), nrows, None if r is None else L.p_i64(r), po, C.byref(inf))
        return rc, lib.okkt_last_error(h._h).decode()

    for fn in ("okkt_get_inverse_columns", "okkt_get_inverse_columns_dev"):
        assert getattr(lib, fn)(None, 0, None, 0, None, None, None) == L.OKKT_ERR_INVALID
        assert inv(fn, 2, cols, 3, rows, out)[0] == L.OKKT_ERR_NO_DEVICE
        assert inv(fn, 2, cols, 0, None, out)[0] == L.OKKT_ERR_NO_DEVICE
        for what, args in {"ncols < 0": (-1, cols, 3, rows, out), "nrows < 0": (2, cols, -1, rows, out), "cols NULL": (2, None, 3, rows, out),
                           "out NULL": (2, cols, 3, rows, None), "column out of range": (2, np.array([0, n], dtype=np.int64), 3, rows, out),
                           "row out of range": (2, cols, 3, np.array([0, 1, -1], dtype=np.int64), out)}.items():
            rc, msg = inv(fn, *args)
            assert rc == L.OKKT_ERR_INVALID and msg, (fn, what, rc, msg)
    # okkt_sparse_reach: its own arguments
    b = np.array([0, 1], dtype=np.int64)
    act = np.zeros(n, dtype=np.uint8)
    pa = act.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.okkt_sparse_reach(None, 0, None, 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 0, None, C.byref(inf), pa) == L.OKKT_OK
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 0, None, C.byref(inf), None) == L.OKKT_OK
    assert lib.okkt_sparse_reach(h._h, 0, None, 0, None, C.byref(inf), None) == L.OKKT_OK and inf.fwd_reach == 0
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 0, None, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_sparse_reach(h._h, -1, L.p_i64(b), 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_sparse_reach(h._h, 2, None, 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), -1, L.p_i64(b), C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(np.array([0, n], dtype=np.int64)), 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 1, L.p_i64(np.array([-1], dtype=np.int64)), C.byref(inf), None) == L.OKKT_ERR_INVALID
    # a partitioned handle
    assert lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    for rc, msg in (_sparse(lib, h._h, 1, [0, 1], [0], [1.0], 0, None, out), inv("okkt_get_inverse_columns", 2, cols, 3, rows, out)):
        assert rc == L.OKKT_ERR_INVALID and "partitioned" in msg
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_dist_set_partition(h._h, 1, 0) == L.OKKT_OK
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 0, None, C.byref(inf), None) == L.OKKT_OK
    finalize_b(h)
    # no analysis
    h = host_handle()
    for rc, msg in (_sparse(lib, h._h, 1, [0, 1], [0], [1.0], 0, None, out), _sparse(lib, h._h, 1, [0, 1], [0], [1.0], 0, None, out, fn="okkt_solve_sparse_dev")):
        assert rc == L.OKKT_ERR_INVALID and "okkt_analyze" in msg
    assert lib.okkt_sparse_reach(h._h, 2, L.p_i64(b), 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_columns(h._h, 2, L.p_i64(cols), 0, None, L.p_f64(out), None) == L.OKKT_ERR_INVALID
    # Schur mode
    hs = host_handle()
    hs.set_schur([2, 3])
    hs.analyze(d.A)
    rc, msg = _sparse(lib, hs._h, 1, [0, 1], [0], [1.0], 0, None, out)
    assert rc == L.OKKT_ERR_INVALID and "Schur mode" in msg
    assert lib.okkt_sparse_reach(hs._h, 2, L.p_i64(b), 0, None, C.byref(inf), None) == L.OKKT_ERR_INVALID
    assert "Schur mode" in lib.okkt_last_error(hs._h).decode()
    assert lib.okkt_get_inverse_columns_dev(hs._h, 2, L.p_i64(cols), 0, None, C.c_void_p(out.ctypes.data), None) == L.OKKT_ERR_INVALID
    finalize_b(hs)
    finalize_b(h)


def reach(h, b_rows, x_rows=None):
    info, active = h.sparse_reach(b_rows, x_rows)
    assert info["nsuper"] == h.stats()["nsuper"] and info["batches"] == 1
    assert info["fwd_run"] >= info["fwd_reach"] and info["bwd_run"] >= info["bwd_reach"]
    assert info["fwd_panel_bytes"] <= info["factor_panel_bytes"] and info["bwd_panel_bytes"] <= info["factor_panel_bytes"]
    return info, active


def check_bits(d, active, bit, expected_nodes, exact):
    """The columns with `bit` are the pivot columns of the expected fronts -- or, where small fronts run as tasks, a superset of them
    made of whole fronts."""
    got = (active & bit) != 0
    want = columns(d, expected_nodes)
    assert np.all(got[want])
    if exact:
        assert np.array_equal(got, want)
    for nd in d.nodes:      # whole fronts
        seg = got[nd["col0"]:nd["col0"] + nd["k"]]
        assert seg.all() or not seg.any()


def test_reach_mixed_level_scatter():
    d, h = designed("mixed-level-scatter")
    ns = len(d.nodes)
    lone = node(d, 450, 0)
    assert d.nodes[lone]["parent"] is None
    info, act = reach(h, [orig(d, lone, 7)])
    assert info["fwd_reach"] == 1 and info["fwd_run"] == 1 and info["fringe"] == 0 and info["fringe_entries"] == 0
    assert info["bwd_reach"] == ns and info["bwd_run"] == ns and info["pruned"] == 1
    assert info["fwd_panel_bytes"] == 450 * 450 * 8
    check_bits(d, act, 1, [lone], True)
    assert np.all(act & 2) and not np.any(act & 4)
    small = node(d, 24, 8)
    info, act = reach(h, [orig(d, lone)], [orig(d, small, 3)])
    assert info["bwd_reach"] == 2 == len(closure(d, [small]))
    check_bits(d, act, 2, closure(d, [small]), info["bwd_run"] == 2)
    # a non-zero in the small child: its parent runs, the three other children are the fringe
    info, act = reach(h, [orig(d, small)], [orig(d, small)])
    A = closure(d, [small])
    fr = fringe_of(d, A)
    assert info["fwd_reach"] == 2 and info["fringe"] == len(fr) == 3
    assert info["fringe_entries"] == sum(d.nodes[i]["f"] - d.nodes[i]["k"] for i in fr) == 200 + 150 + 250
    check_bits(d, act, 4, fr, True)
    finalize_b(h)


def test_reach_deep_chain():
    d, h = designed("deep-chain-6")
    leaf, root = node(d, 130, 740), node(d, 300, 0)
    assert len(closure(d, [leaf])) == 6
    info, act = reach(h, [orig(d, leaf, 129)], [orig(d, leaf)])
    assert info["fwd_reach"] == info["fwd_run"] == 6 and info["bwd_reach"] == info["bwd_run"] == 6 and info["fringe"] == 0
    assert info["pruned"] == 0 and info["fwd_panel_bytes"] == info["factor_panel_bytes"]      # every supernode, both ways: the ordinary sweeps
    info, act = reach(h, [orig(d, root)], [orig(d, leaf)])
    assert info["fwd_reach"] == info["fwd_run"] == 1 and info["bwd_reach"] == 6 and info["pruned"] == 1
    assert info["fringe"] == 1 and info["fringe_entries"] == 290      # the root's one child does not run forward
    check_bits(d, act, 1, [root], True)
    check_bits(d, act, 2, closure(d, [leaf]), True)
    mid = node(d, 160, 440)
    info, act = reach(h, [orig(d, mid)], [orig(d, mid)])
    assert info["fwd_reach"] == 3 == len(closure(d, [mid])) and info["bwd_reach"] == 3 and info["fringe"] == 1 and info["fringe_entries"] == 560
    finalize_b(h)


def test_reach_fan_in_8():
    d, h = designed("fan-in-8")
    child = node(d, 260, 250)
    A = closure(d, [child])
    fr = fringe_of(d, A)
    info, act = reach(h, [orig(d, child, 5)], [orig(d, child, 5)])
    assert info["fwd_reach"] == 2 == len(A) and info["fwd_run"] == 2
    assert info["fringe"] == 7 == len(fr)
    assert info["fringe_entries"] == sum(d.nodes[i]["f"] - d.nodes[i]["k"] for i in fr) == 399 + 300 + 380 + 200 + 390 + 129 + 128
    check_bits(d, act, 1, A, True)
    check_bits(d, act, 4, fr, True)
    # two children: the fringe is the other six
    other = node(d, 385, 200)
    info, _ = reach(h, [orig(d, child), orig(d, other), orig(d, other, 1)])
    assert info["fwd_reach"] == 3 and info["fringe"] == 6
    finalize_b(h)


def test_reach_task_chains_under_big():
    d, h = designed("task-chains-under-big")
    # the 8-chain comes first in postorder?  find the two chains by walking down from the root's children
    root = node(d, 300, 0)
    kids = [i for i, nd in enumerate(d.nodes) if nd["parent"] == root]
    depth = {}
    for kd in kids:
        below = [i for i in range(len(d.nodes)) if kd in closure(d, [i]) and i != root]
        depth[kd] = len(below)
    top8 = next(kd for kd, n_ in depth.items() if n_ == 8)
    top6 = next(kd for kd, n_ in depth.items() if n_ == 6)
    big = node(d, 150, 120)
    leaf8 = next(i for i in range(len(d.nodes)) if top8 in closure(d, [i]) and not any(nd["parent"] == i for nd in d.nodes))
    A = closure(d, [leaf8])
    assert len(A) == 9
    info, act = reach(h, [orig(d, leaf8)], [orig(d, leaf8)])
    assert info["fwd_reach"] == 9 and info["fwd_run"] >= 9 and info["fwd_run"] < len(d.nodes)
    fr = fringe_of(d, A)
    assert sorted(fr) == sorted([top6, big])
    assert info["fringe"] == 2 and info["fringe_entries"] == 16 + 120 == 136
    check_bits(d, act, 1, A, info["fwd_run"] == 9)
    check_bits(d, act, 4, fr, True)
    assert info["bwd_reach"] == 9
    finalize_b(h)


def test_reach_on_a_kkt_pattern_with_default_relaxation():
    prob = synth.make_config("S-small", seed=3, well_scaled=True)
    K = sp.csc_matrix(synth.augmented_matrix(prob, delta=1e-8))
    h = host_handle(K)
    n = K.shape[0]
    perm = h.perm()
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    parent, _ = h.etree()
    ns = h.stats()["nsuper"]

    def col_closure(rows):
        m = np.zeros(n, dtype=bool)
        for j in iperm[np.asarray(rows, dtype=np.int64)]:
            while j >= 0 and not m[j]:
                m[j] = True
                j = parent[j]
        return m

    rng = np.random.default_rng(5)
    for trial in range(6):
        b = rng.choice(n, size=int(rng.integers(1, 6)), replace=False)
        x = rng.choice(n, size=int(rng.integers(1, 6)), replace=True)
        info, act = reach(h, b, x)
        fw, bw = col_closure(b), col_closure(x)
        assert np.all((act & 1)[fw] == 1), trial
        assert np.all((act & 2)[bw] == 2), trial
        assert info["fwd_run"] <= ns and info["fwd_reach"] >= 1
        # the fringe never runs forward
        assert not np.any((act & 4) & ((act & 1) << 2))
        if info["fwd_run"] < ns:
            assert info["pruned"] == 1 and info["fwd_panel_bytes"] < info["factor_panel_bytes"]
    # b on every leaf of the column tree: every supernode, the ordinary sweeps
    is_parent = np.zeros(n, dtype=bool)
    is_parent[parent[parent >= 0]] = True
    leaves = perm[~is_parent]
    info, act = reach(h, leaves)
    assert info["fwd_reach"] == ns == info["fwd_run"] and info["bwd_run"] == ns and info["pruned"] == 0 and info["fringe"] == 0
    assert np.all(act == 3)
    # and nothing at all
    info, act = reach(h, [], [])
    assert info["fwd_reach"] == info["bwd_reach"] == info["fringe"] == 0 and not act.any()
    finalize_b(h)
