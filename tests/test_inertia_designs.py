"""The catalogue of inertia_designs.py (host only): the conditions under which the oracle's pivot counts are the expected counts
of the GPU file hold for every design -- so that no design needs an exemption on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import inertia_designs as idn  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP  # noqa: E402


def test_the_catalogue_is_the_issue_list():
    assert len(idn.NAMES) == 10 and set(idn.NAMES) <= set(ft.DESIGNS)
    assert max(idn.reference(n).design.n for n in idn.NAMES) == 2234
    assert [n for n in idn.NAMES if idn.reference(n).nlevels == 1] == ["edge-k256-c0"]
    assert idn.ALL[:10] == idn.NAMES and not set(idn.EXTRA) & set(ft.DESIGNS)


@pytest.mark.parametrize("name", list(idn.EXTRA))
def test_analysis_reproduces_the_extra_design(name):
    """as test_front_trees.py for the catalogue of front_trees: the analysis finds exactly the designed fronts, all of them small"""
    d = idn.reference(name).design
    assert max(f for _, f, _ in d.fronts) <= 128 and idn.reference(name).nlevels >= 3
    s = linear_solver_HIP("symmetric", host_symbolic_only=1, ordering=2, **ft.NO_RELAX)
    initialize_b(s)
    s.set_perm(d.perm)
    s.analyze(d.A)
    assert np.array_equal(s.perm(), d.perm)
    st = s.stats()
    assert {k: st[k] for k in d.fingerprint()} == d.fingerprint() and st["n_big_fronts"] == 0
    assert np.array_equal(s.etree()[1], d.colcounts())
    finalize_b(s)


@pytest.mark.parametrize("name", idn.ALL)
def test_quantile_tolerances_sit_in_wide_gaps(name):
    """Three tolerances inside the spectrum of |D|, each at least 1e-6 (relative) from the nearest pivot; the gap near the 25 %
    quantile is 1.0e-4 .. 3.0e-3 wide on every design; the oracle's counts there add up to n and really split the pivots."""
    r = idn.reference(name)
    tols = idn.quantile_tols(name)
    assert len(tols) == 3 and tols[0][0] < tols[1][0] < tols[2][0]
    for (tol, gap, cnt), q in zip(tols, idn.QUANTILES):
        print(f"INERTIA_HOST {name} q={q} tol={tol:.6e} gap={gap:.3e} nearest={idn.rel_dist(r.D, tol):.3e} counts={cnt}")
        assert idn.rel_dist(r.D, tol) >= idn.MIN_REL_DIST
        assert sum(cnt) == r.design.n and cnt[3] == 0
        assert abs(cnt[2] - q * r.design.n) <= idn.WINDOW // 2 + 1      # the zeros are the pivots below the quantile
        assert cnt[0] <= r.design.npos and cnt[1] <= r.design.nneg
    if name in idn.NAMES:
        assert 1.0e-4 <= tols[1][1] <= 3.0e-3, tols[1]
    assert r.oracle.inertia() == (r.design.npos, r.design.nneg, 0, 0)


@pytest.mark.parametrize("name", idn.ALL)
def test_boundary_matrices(name):
    """+-t and its outer neighbours on the first pivot of every leaf: the pattern is the design's, no other pivot is near t (the
    function asserts >= 1e-6; measured >= 0.41), the expected counts add up to n and move by the number of leaves between a value
    on the tolerance and its neighbour outside."""
    r = idn.reference(name)
    d = r.design
    bm = idn.boundary_matrices(name)
    nleaf = len(idn.leaf_first_pivots(d))
    assert nleaf >= 1 and set(bm) == set(idn.BOUNDARY_KINDS)
    for kind, (A, cnt) in bm.items():
        assert np.array_equal(A.indptr, d.A.indptr) and np.array_equal(A.indices, d.A.indices)
        assert sum(cnt) == d.n and cnt[3] == 0
    # the matrices of a pair differ by one ulp in nleaf entries: every other pivot keeps its class
    assert bm["+t_up"][1][0] - bm["+t"][1][0] == nleaf and bm["+t"][1][2] - bm["+t_up"][1][2] == nleaf
    assert bm["-t_down"][1][1] - bm["-t"][1][1] == nleaf and bm["-t"][1][2] - bm["-t_down"][1][2] == nleaf
    o = idn._factor(bm["+t"][0], d.perm, d.npos, d.nneg)
    P, Lo = d.l_pattern(), o.L()
    assert np.array_equal(Lo.indptr, P.indptr) and np.array_equal(Lo.indices, P.indices)
    leaves = idn.leaf_first_pivots(d)
    assert idn.rel_dist(o.diag(), idn.T_BOUNDARY, skip=leaves) >= 0.25


@pytest.mark.parametrize("name", idn.ALL)
def test_isolated_roots_keep_the_designed_pattern(name):
    r = idn.reference(name)
    A, perm, whole, cnt = idn.isolated(name)
    assert cnt == (r.design.npos, r.design.nneg, 1, 2) and whole.n == r.design.n + 3
    diag = A.diagonal()[-3:]
    assert diag[0] == 0.0 and np.isnan(diag[1]) and diag[2] == np.inf
    assert A[-3:, :].nnz == 3 and A[:, -3:].nnz == 3          # no off-diagonal entry: nothing propagates
    o = idn._factor(A, perm, cnt[0] + 3, cnt[1])
    P, Lo = whole.l_pattern(), o.L()
    assert np.array_equal(Lo.indptr, P.indptr) and np.array_equal(Lo.indices, P.indices)
    assert np.array_equal(o.diag()[:r.design.n], r.D)      # (the oracle stops at the zero pivot behind them: the counts are the design's)
    s = linear_solver_HIP("symmetric", host_symbolic_only=1, ordering=2, **ft.NO_RELAX)
    initialize_b(s)
    s.set_perm(perm)
    s.analyze(A)
    st = s.stats()
    assert {k: st[k] for k in whole.fingerprint()} == whole.fingerprint()
    finalize_b(s)


@pytest.mark.parametrize("name", idn.ALL)
def test_requests_and_level_counts(name):
    r = idn.reference(name)
    d = r.design
    pre = idn.level_prefix_counts(name)
    assert len(pre) == r.nlevels + 1 and pre[0] == (0, 0) and pre[-1] == (d.npos, d.nneg)
    assert all(a[0] <= b[0] and a[1] <= b[1] and sum(a) < sum(b) for a, b in zip(pre, pre[1:]))
    assert [sum(p) for p in pre] == [sum(k for k, _, lv in d.fronts if lv < l) for l in range(r.nlevels + 1)]
    n_req, m_req = idn.decided_low(name)
    assert m_req >= 0 and n_req + m_req == d.n and (n_req, m_req) != (d.npos, d.nneg)
    assert pre[1][1] == m_req + 1                                   # level 0 alone holds one negative pivot too many
    lv = idn.documented_early_level(name)
    assert lv is None or 1 <= lv < r.nlevels


def test_documented_early_levels():
    """The host's early check has a level to fire at on deep-chain-6 (and on two more designs), and none on others.  The root of
    fan-in-8 holds 7 % of the design's flops (its eight children the rest): by the documented rule it has no early level."""
    lv = {n: idn.documented_early_level(n) for n in idn.ALL}
    print("INERTIA_HOST early levels", lv)
    assert lv["deep-chain-6"] is not None and lv["deep-chain-6"] >= 1
    assert sum(v is not None for v in lv.values()) >= 3
    assert lv["edge-k256-c0"] is None and lv["fan-in-8"] is None
    # where the early check fires, the wrong request of decided_low is decided by then and something is left to skip
    for n, l in lv.items():
        if l is not None:
            pre = idn.level_prefix_counts(n)
            assert pre[l][1] > idn.decided_low(n)[1] and sum(pre[l]) < idn.reference(n).design.n
