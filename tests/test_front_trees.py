"""The designed elimination trees of front_trees.py (host only: a host_symbolic_only handle).  The analysis of every design of the
GPU catalogue has to produce exactly the designed fronts -- so that no GPU time goes into a design that does not take the route it
claims to, and so that a later change of the symbolic phase cannot move a design off its route unnoticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP  # noqa: E402


@pytest.mark.parametrize("values", ["plain", "ipm"])
@pytest.mark.parametrize("name", list(ft.DESIGNS))
def test_analysis_reproduces_the_design(name, values):
    roots, _ = ft.DESIGNS[name]
    d = ft.build(roots, values=values)
    assert d.A.nnz == d.l_pattern().nnz + d.n          # every designed entry is stored (the ipm zeros included)
    s = linear_solver_HIP("symmetric", host_symbolic_only=1, ordering=2, **ft.NO_RELAX)
    initialize_b(s)
    s.set_perm(d.perm)
    s.analyze(d.A)
    assert np.array_equal(s.perm(), d.perm)            # the design's numbering is the analysis' postorder
    st = s.stats()
    assert {k: st[k] for k in d.fingerprint()} == d.fingerprint()
    assert st["n_big_fronts"] == sum(f > 128 for _, f, _ in d.fronts)
    _, cnt = s.etree()
    assert np.array_equal(cnt, d.colcounts())
    finalize_b(s)


def test_the_catalogue_covers_the_edges():
    """Every pivot count and CB size of the issue's edge list, and the pairs that must be present."""
    ks = {k for k, _ in ft.EDGE_PAIRS}
    cs = {c for _, c in ft.EDGE_PAIRS}
    assert ks == {129, 255, 256, 257, 383, 384, 385, 1023, 1024, 1025, 2047, 2048, 2049}
    assert cs == {0, 1, 63, 127, 128, 129, 700}
    assert {(385, 1), (1025, 1), (2049, 129)} <= set(ft.EDGE_PAIRS)
    assert max(ft.build(r).n for r, _ in ft.DESIGNS.values()) <= 6000


def test_scatter_spreads_the_contribution_block():
    d = ft.build(ft.DESIGNS["mixed-level-scatter"][0])
    sep = [nd for nd in d.nodes if nd["k"] == 260][0]
    for nd in d.nodes:
        if nd["parent"] is not None:
            cb = nd["rows"][nd["k"]:]
            assert cb[0] == sep["col0"] and cb[-1] > sep["col0"] + len(cb)      # starts at the first pivot, not contiguous
