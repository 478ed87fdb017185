"""Designed fronts for the pivot counters and the early exit of the delta loop: catalogue and reference, host only.

The designs are those of front_trees.py at the smallest shapes on which the counting routes differ (LDS-resident small fronts
of every class, task chains, lone fronts folded into the big fronts' launch, thin / mid / wide big fronts, deep and wide trees,
ragged last tiles).  Every design of front_trees is diagonally dominant with a designed sign, so on the plain matrices the
counted inertia always equals the request and no pivot comes near the tolerance.  What is added here makes the counters decide
something, and every expected number comes from the simplicial oracle or from the design itself:

  * quantile_tols: tolerances inside the spectrum of |D| (near its 10 %, 25 % and 60 % quantiles), each in the middle of a gap
    that is far wider than the error of any factorisation route -- the counts at such a tolerance are the oracle's;
  * boundary_matrices: the first pivot of every leaf front sits exactly on +-t or one ulp outside it (a leaf's first pivot takes
    no update: d is the stored entry bit for bit), t = 0.5 the handle's tolerance;
  * isolated: three extra 1 x 1 roots whose pivots are 0, NaN and +inf (no row below them: nothing propagates);
  * decided_low: a wrong request that the pivots of level 0 alone already refute; level_prefix_counts: what has been counted
    below every level boundary; documented_early_level: the boundary at which the host looks, from the rule in numeric.h.
"""
import numpy as np
import scipy.sparse as sp

import front_trees as ft
import oracle
from front_trees import N

NAMES = ["small-classes-f32-33-64-65-128-129", "task-chains-under-big", "fold-lone-3", "mixed-level", "deep-chain-6", "fan-in-8",
         "edge-k257-c127", "edge-k129-c700", "edge-k385-c1", "edge-k256-c0"]
# One design more, not in front_trees: small fronts only.  Its leading levels hold no big front, so they run as ONE launch of tasks
# that hand over through flags and an epoch (k_front_small<.., FLOW>): the only place where a stopped task has to release its waiting
# parent, and where an epoch survives a stop.  Four tasks of three fronts each (cost 1 + f^2 k / 8192 = 98 for the 108-row front: a
# task of its own each, the root's subtree is 2.5 x its critical path and is split) under a root task: two levels of tasks.
EXTRA = {"flow-small-only": ([N(60, 0, *[N(68, 40, N(8, 16), N(8, 16, scatter=True)) for _ in range(4)])],
                             "small fronts only: every level in one launch of tasks")}
ALL = NAMES + list(EXTRA)
# the designs whose scheduled units are not the designed levels (small fronts run as tasks that span several levels)
UNITS_DIFFER = ("small-classes-f32-33-64-65-128-129", "task-chains-under-big", "flow-small-only")
QUANTILES = (0.10, 0.25, 0.60)
WINDOW = 40            # neighbouring sorted values among which a tolerance looks for its gap
MIN_REL_DIST = 1e-6    # nearest |d| to a tolerance, relative: four decades above the 1e-10 the HIP D is held to against the oracle
T_BOUNDARY = 0.5
BOUNDARY_KINDS = ("+t", "+t_up", "-t", "-t_down")      # classes: zero, pos, zero, neg
ISOLATED_VALUES = (0.0, float("nan"), float("inf"))

_REF, _TOLS, _BOUNDARY = {}, {}, {}      # per design, computed once and never changed


class Reference:
    """design, oracle (factored on the design's permutation), D = the oracle's D, fronts = [(pivot columns, level)] in postorder"""

    def __init__(self, design, orc):
        self.design, self.oracle = design, orc
        self.D = orc.diag()
        self.fronts = [(np.arange(nd["col0"], nd["col0"] + nd["k"]), nd["level"]) for nd in design.nodes]
        self.level_of_col = np.zeros(design.n, dtype=np.int64)
        for cols, lv in self.fronts:
            self.level_of_col[cols] = lv
        self.nlevels = 1 + int(self.level_of_col.max())


def _factor(A, perm, npos, nneg):
    o = oracle.linear_solver_ORACLE("symmetric", perm=perm)
    o.ls_factor_b(A, npos, nneg)
    return o


def roots_of(name):
    return (EXTRA[name] if name in EXTRA else ft.DESIGNS[name])[0]


def reference(name):
    if name not in _REF:
        d = ft.build(roots_of(name))
        _REF[name] = Reference(d, _factor(d.A, d.perm, d.npos, d.nneg))
    return _REF[name]


def rel_dist(D, tol, skip=None):
    """smallest | |d| - tol | / tol over the finite pivots (those of `skip` left out)"""
    a = np.abs(D)
    keep = np.isfinite(a)
    if skip is not None:
        keep[skip] = False
    return float(np.min(np.abs(a[keep] - tol)) / tol)


def quantile_tols(name):
    """[(tol, relative width of its gap, oracle counts at tol)] for the three quantiles.  The tolerance is the geometric mean of the
    two neighbours of the widest (relative) gap among the WINDOW sorted values of |D| around the quantile."""
    if name in _TOLS:
        return _TOLS[name]
    r = reference(name)
    a = np.sort(np.abs(r.D))
    out = _TOLS[name] = []
    for q in QUANTILES:
        i0 = int(q * len(a))
        lo = max(0, i0 - WINDOW // 2)
        w = a[lo:lo + WINDOW + 1]
        gaps = w[1:] / w[:-1] - 1.0
        g = int(np.argmax(gaps))
        tol = float(np.sqrt(w[g] * w[g + 1]))
        assert rel_dist(r.D, tol) >= MIN_REL_DIST, (name, q, tol)
        out.append((tol, float(gaps[g]), r.oracle.inertia(tol)))
    return out


def leaf_first_pivots(d):
    """first pivot column (permuted numbering) of every leaf front"""
    has_child = {nd["parent"] for nd in d.nodes if nd["parent"] is not None}
    return np.array([nd["col0"] for i, nd in enumerate(d.nodes) if i not in has_child], dtype=np.int64)


def set_diagonal(A, idx, value):
    """a copy of the lower-triangular CSC matrix A with A[i, i] = value for i in idx (the entries are stored)"""
    A = sp.csc_matrix(A, copy=True)
    A.sort_indices()
    for i in idx:
        p = A.indptr[i]
        assert A.indices[p] == i, "the diagonal is the first stored entry of a lower-triangular column"
        A.data[p] = value
    return A


def boundary_matrices(name):
    """{kind: (matrix, expected (pos, neg, zero, nonfinite) at inertia_tol = T_BOUNDARY)}: the first pivot of every leaf front is +t,
    the next double above +t, -t, the next double below -t -- classify_pivot has to call them zero, pos, zero and neg.  Every other
    pivot is counted from the oracle's D of the same matrix, none of them within MIN_REL_DIST of t."""
    if name in _BOUNDARY:
        return _BOUNDARY[name]
    r = reference(name)
    d, t = r.design, T_BOUNDARY
    leaves = leaf_first_pivots(d)
    vals = {"+t": t, "+t_up": np.nextafter(t, np.inf), "-t": -t, "-t_down": np.nextafter(-t, -np.inf)}
    forced = {"+t": (0, 0, 1), "+t_up": (1, 0, 0), "-t": (0, 0, 1), "-t_down": (0, 1, 0)}
    out = _BOUNDARY[name] = {}
    for kind in BOUNDARY_KINDS:
        A = set_diagonal(d.A, d.perm[leaves], vals[kind])
        D = _factor(A, d.perm, d.npos, d.nneg).diag()
        assert np.all(np.isfinite(D))
        assert np.array_equal(D[leaves], np.full(len(leaves), vals[kind])), "a leaf's first pivot takes no update"
        assert rel_dist(D, t, skip=leaves) >= MIN_REL_DIST, (name, kind)
        rest = np.ones(d.n, dtype=bool)
        rest[leaves] = False
        fp, fn, fz = forced[kind]
        pos = int(np.sum(D[rest] > t)) + fp * len(leaves)
        neg = int(np.sum(D[rest] < -t)) + fn * len(leaves)
        zer = int(np.sum(np.abs(D[rest]) <= t)) + fz * len(leaves)
        out[kind] = (A, (pos, neg, zer, 0))
    return out


def isolated(name, value=ISOLATED_VALUES):
    """(matrix, perm, design of the whole, expected counts): the design plus one 1 x 1 root per entry of `value` (diagonals 0, NaN and
    +inf by default), no off-diagonal entry, numbered behind the design.  Default tolerance: the design's counts plus one zero and
    two non-finite pivots."""
    r = reference(name)
    d, e = r.design, len(value)
    B = sp.csc_matrix(d.A)
    B.sort_indices()
    # the extra columns appended by hand: the diagonal is stored whatever its value (an explicit zero included)
    A = sp.csc_matrix((np.concatenate([B.data, np.array(value, dtype=np.float64)]), np.concatenate([B.indices, d.n + np.arange(e)]),
                       np.concatenate([B.indptr, B.nnz + 1 + np.arange(e)])), shape=(d.n + e, d.n + e))
    assert A.nnz == d.A.nnz + e and A.has_sorted_indices
    perm = np.concatenate([d.perm, d.n + np.arange(e)]).astype(np.int64)
    nodes = list(d.nodes) + [dict(k=1, f=1, level=0, col0=d.n + i, rows=np.array([d.n + i]), parent=None) for i in range(e)]
    whole = ft.Built(n=d.n + e, A=A, perm=perm, nodes=nodes, npos=d.npos, nneg=d.nneg, values=d.values)
    nzero = sum(1 for v in value if v == 0.0)
    nbad = sum(1 for v in value if not np.isfinite(v))
    assert nzero + nbad == e, "the extra roots are zeros and non-finite values"
    return A, perm, whole, (d.npos, d.nneg, nzero, nbad)


def level_prefix_counts(name):
    """[(pos, neg) of every front below level l for l = 0 .. nlevels]: entry 0 is (0, 0), the last one the whole inertia"""
    r = reference(name)
    return [(int(np.sum((r.level_of_col < l) & (r.D > 0))), int(np.sum((r.level_of_col < l) & (r.D < 0)))) for l in range(r.nlevels + 1)]


def decided_low(name):
    """(n_req, m_req): one negative pivot fewer than level 0 alone holds -- wrong, and decided by level 0 (on a design of a single
    level that is the whole tree: the request is one off)"""
    r = reference(name)
    m_req = level_prefix_counts(name)[1][1] - 1
    return (r.design.n - m_req, m_req)


def documented_early_level(name):
    """The level before which the host reads the counters (numeric.h, DESIGN.md "Early exit in the delta loop"): the last level
    boundary l >= 1 with at least 30 % of sum k f^2 - k^2 f + k^3 / 3 at or above it; None when there is none.  From the design's
    own (k, f, level): it is the schedule's level wherever the scheduled units are the designed levels (not in UNITS_DIFFER)."""
    fronts = reference(name).design.fronts
    flops = lambda k, f: k * f * f - k * k * f + k ** 3 / 3.0      # noqa: E731
    tot = sum(flops(float(k), float(f)) for k, f, _ in fronts)
    nlev = 1 + max(lv for _, _, lv in fronts)
    for l in range(nlev - 1, 0, -1):
        if sum(flops(float(k), float(f)) for k, f, lv in fronts if lv >= l) >= 0.3 * tot:
            return l
    return None
