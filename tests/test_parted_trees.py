"""The designed cuts of parted_trees.py on a host_symbolic_only handle: for every design and number of parts the analysis gives the
design's own fronts and `partition_tree` the cut of the catalogue -- the owners, the boundary fronts, the sizes of the exchange
buffers and the flops of the parts and of the top.  So that no GPU time goes into a cut that is not the designed one, and a later
change of the partitioner cannot move one unnoticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parted_trees as pt  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402

_BUILT = {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = pt.build(name)
    return _BUILT[name]


@pytest.mark.parametrize("case", pt.CASES, ids=pt.case_id)
def test_the_partitioner_makes_the_designed_cut(case):
    name, nparts = case
    d = built(name)
    want = pt.DESIGNS[name]
    owners = np.array(want["cuts"][nparts])
    s, sn, col, par, info = pt.host_cut(d, nparts)
    assert np.array_equal(s.perm(), d.perm)
    st = s.stats()
    assert {k: st[k] for k in d.fingerprint()} == d.fingerprint()
    assert np.array_equal(par, [-1 if nd["parent"] is None else nd["parent"] for nd in d.nodes])
    assert sn.tolist() == owners.tolist(), (name, nparts, sn.tolist())
    assert np.array_equal(col, pt.col_owner(d, owners))
    assert set(sn.tolist()) <= set(range(-1, nparts))
    for c, p in enumerate(par):
        if sn[c] == -1:
            assert (par == c).any()        # a top front is one that was split: it has children
        if p < 0:
            continue
        if sn[p] >= 0:
            assert sn[c] == sn[p]          # below an owned front everything has that owner
        if sn[c] == -1:
            assert sn[p] == -1             # the parent of a top front is a top front
    sl, cb, cv = pt.slots(d, owners)
    assert info["n_boundary"] == len(sl) == want["n_boundary"]
    assert info["cb_doubles"] == cb == want["cb_doubles"]
    assert info["cv_doubles"] == cv == sum(r for _, r, _, _ in sl)
    total = sum(info["part_flops"]) + info["top_flops"]
    assert abs(total - st["flops_stored"]) <= 1e-6 * st["flops_stored"]
    assert (info["top_flops"] > 0) == bool((owners == -1).any())
    for p in range(nparts):
        assert (info["part_flops"][p] > 0) == bool((owners == p).any()), (p, info["part_flops"])
    finalize_b(s)
    # every rank analyses for itself: the cut does not depend on which part asks
    for part_id in range(1, nparts):
        s2, sn2, col2, par2, info2 = pt.host_cut(d, nparts, part_id)
        assert np.array_equal(sn2, sn) and np.array_equal(col2, col) and info2 == info
        finalize_b(s2)


def test_the_catalogue_covers_the_cuts():
    """A cut without a top, tops of one and of two levels, a wide top and a top of small fronts only; boundary fronts with k = 1, of
    every small class, thin, mid and wide, one with a scattered CB; an empty part, a part of small fronts only, a wide front in
    part 0 and one in a part > 0, a small top front over small boundary fronts; no design above 2 600 unknowns."""
    tops, top_kinds, bclass, bk, scattered = set(), set(), set(), set(), False
    empty = small_part = wide0 = wide_other = small_over_small = False
    for name, nparts in pt.CASES:
        d = built(name)
        owners = pt.DESIGNS[name]["cuts"][nparts]
        assert len(owners) == len(d.nodes)
        tops.add(pt.top_levels(d, owners))
        top = [nd for nd, o in zip(d.nodes, owners) if o == -1]
        if top and all(nd["f"] <= pt.SMALL_MAX for nd in top):
            top_kinds.add("small")
        if any(pt.front_class(nd) == "wide" for nd in top):
            top_kinds.add("wide")
        for i in pt.boundary_of(d, owners):
            nd = d.nodes[i]
            bclass.add(pt.front_class(nd))
            bk.add(nd["k"])
            scattered |= pt.is_scattered(nd)
            small_over_small |= nd["f"] <= pt.SMALL_MAX and d.nodes[nd["parent"]]["f"] <= pt.SMALL_MAX
        for p in range(nparts):
            mine = [nd for nd, o in zip(d.nodes, owners) if o == p]
            empty |= not mine
            small_part |= bool(mine) and all(nd["f"] <= pt.SMALL_MAX for nd in mine)
            wide = any(pt.front_class(nd) == "wide" for nd in mine)
            wide0 |= wide and p == 0
            wide_other |= wide and p > 0
    assert {0, 1, 2} <= tops, tops
    assert top_kinds == {"small", "wide"}, top_kinds
    assert {"f<=32", "f<=64", "f<=128", "thin", "mid", "wide"} <= bclass, bclass
    assert 1 in bk
    assert scattered and empty and small_part and wide0 and wide_other and small_over_small
    assert max(built(name).n for name in pt.DESIGNS) <= 2600
    assert set(pt.VARIANT_CASES) <= set(pt.CASES)
    assert {("cut-mid-wide", 2), ("two-level-top-4", 3), ("small-subtrees-under-big-top", 4), ("wide-top-1100", 2)} <= set(pt.VARIANT_CASES)
