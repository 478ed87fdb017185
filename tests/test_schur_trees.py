"""The Schur designs of schur_trees.py on a host_symbolic_only handle: with the pivot columns of a design's last root held back as
the Schur set, the analysis has to give the design's own permutation, fingerprint and column counts -- the interior is the designed
fronts, the Schur front is the root (k = f = ns), and an interior root that does not touch the set stays a root.  So that no GPU time
goes into a set whose children are not the designed ones, and a later change of the Schur-mode analysis cannot move one unnoticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schur_trees as sct  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402


@pytest.mark.parametrize("name", list(sct.DESIGNS))
def test_analysis_reproduces_the_design_with_its_root_held_back(name):
    d = sct.build(name)
    ns = sct.set_size(d)
    root = d.nodes[-1]
    assert root["parent"] is None and root["f"] == root["k"] == ns and root["col0"] == d.n - ns
    s = sct.schur_handle(d, host_symbolic_only=1)
    perm = s.perm()
    assert np.array_equal(perm, d.perm)
    assert np.array_equal(perm[d.n - ns:], sct.set_index(d))          # the set is the tail of the permutation, in its own order
    st = s.stats()
    assert {k: st[k] for k in d.fingerprint()} == d.fingerprint()
    assert st["n_big_fronts"] == sum(f > 128 for _, f, _ in d.fronts)
    par, cnt = s.etree()
    assert np.array_equal(cnt, d.colcounts())
    # the elimination tree: the last pivot of a front points at the first CB row, a root's at nothing
    for nd in d.nodes:
        last = nd["col0"] + nd["k"] - 1
        assert par[last] == (-1 if nd["parent"] is None else nd["rows"][nd["k"]]), (name, nd["k"], nd["f"])
    for i in sct.lone_roots(d):
        nd = d.nodes[i]
        assert par[nd["col0"] + nd["k"] - 1] == -1
    finalize_b(s)


def test_the_catalogue_covers_the_set_edges():
    """Every set size of the list, a childless set, lone interior roots, an interior of small fronts only, and every child class
    under a set: small fronts of each LDS class, a chain of small fronts, thin / mid / wide big fronts, scattered CBs, a set of at
    most 128 rows above a big child, and CBs that end at the first 1024-row chunk boundary of a set > 2048, one row past it and at the second boundary."""
    built = {name: sct.build(name) for name in sct.DESIGNS}
    sizes = {sct.set_size(d) for d in built.values()}
    assert sct.SET_SIZES <= sizes, sct.SET_SIZES - sizes
    for name in sct.CHILDLESS:
        assert sct.children_of_set(built[name]) == [] and not sct.reached(built[name]).any()
    assert all(sct.children_of_set(d) for name, d in built.items() if name not in sct.CHILDLESS)
    lone = built["lone-roots-then-set"]
    assert sorted(lone.nodes[i]["f"] for i in sct.lone_roots(lone)) == [30, 140]
    assert max(f for _, f, _ in built["set-65-small-only"].fronts[:-1]) <= 128
    kids = [(nd["k"], nd["f"], sct.set_size(d)) for d in built.values() for nd in sct.children_of_set(d)]
    fs = {f for _, f, _ in kids}
    assert {32, 33, 64, 65, 128, 129} <= fs                                              # the small classes at their edges
    assert any(k <= 128 < f for k, f, _ in kids) and any(128 < k <= 384 for k, f, _ in kids) and any(k > 384 for k, f, _ in kids)
    assert any(f > 128 and ns <= 128 for _, f, ns in kids)                               # a small set above a big child
    chain = built["task-chains-under-big"]
    assert sum(nd["k"] == 8 and nd["f"] == 24 for nd in sct.children_of_set(chain)) == 2      # the tops of the two chains
    d = built["set-2049-thin"]
    ends = {int(nd["rows"][-1]) - (d.n - 2049) + 1 for nd in sct.children_of_set(d)}     # one past the last CB row, set numbering
    assert {1024, 1025, 2048} <= ends
    assert any(np.any(np.diff(nd["rows"][nd["k"]:]) > 1) and nd["f"] > 128 for nd in sct.children_of_set(d))      # a scattered big CB
    assert max(d.n for d in built.values()) <= 6000
    assert set(sct.IPM_DESIGNS) | set(sct.VARIANT_DESIGNS) <= set(sct.DESIGNS)
