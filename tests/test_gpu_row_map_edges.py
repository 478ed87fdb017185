"""GPU tests of the row-map kernels at the edges of their partition: the double-double residual and omega
(csrc/refine.hip), the Ruiz row maxima (csrc/scaling.hip) and the ||F||_1 row sums (csrc/condest.hip) on the designs of
tests/row_map_designs.py, against exact arithmetic (fractions.Fraction), scaling_ref.py and the bounds that
test_row_map_designs_host.py proves for the reference.  okkt_debug_row_map shows that every design landed where it claims.
One REFINE / SCALING / CONDEST {json} line per design carries the worst measured err / bound."""
import ctypes as C
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_map_designs as rd  # noqa: E402
import scaling_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
U = rd.U
CAT = rd.catalogue()
NRHS = 7


def record(kind, **kw):
    print(kind + " " + json.dumps(kw))


def query(h):
    out = np.zeros(6, dtype=np.int64)
    h._check(h._lib.okkt_debug_row_map(h._h, L.p_i64(out)), "okkt_debug_row_map")
    return tuple(int(v) for v in out)


def handle(d, nz=None):
    """a handle on the design's pattern; factored with the values nz where they are given.  A row without a diagonal is ordered last"""
    opts = {}
    perm = None
    if d.last:
        g = linear_solver_HIP("symmetric")
        initialize_b(g)
        g.analyze(d.raw(np.zeros(len(d.rowval))))
        p = [int(v) for v in g.perm()]
        finalize_b(g)
        perm = np.array([v for v in p if v not in d.last] + list(d.last), dtype=np.int64)
        opts = dict(ordering=2)
    h = linear_solver_HIP("symmetric", **opts)
    initialize_b(h)
    if perm is not None:
        h.set_perm(perm)
    if nz is None:
        h.analyze(d.raw(np.zeros(len(d.rowval))))
    else:
        flag = h.ls_factor_b(d.raw(nz), d.n - len(d.last), len(d.last))
        assert flag == (0 if d.name == "zero-last" else 1), (d.name, flag, h.inertia)
    return h


# ---- placement ---------------------------------------------------------------------------------------------------------------------

def test_every_design_lands_where_it_claims():
    for name in rd.ALL_DESIGNS:
        d = CAT[name]
        h = handle(d)
        assert query(h) == d.query(), name                       # the query builds the map
        x = np.ones(d.n)
        h.residual(np.zeros(len(d.rowval)), x, x)
        assert query(h) == d.query(), name                       # and a residual pass leaves it
        finalize_b(h)


def test_query_refusals():
    d = CAT["avg5-on"]
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    out = np.zeros(6, dtype=np.int64)
    lib = h._lib
    assert lib.okkt_debug_row_map(h._h, L.p_i64(out)) == L.OKKT_ERR_INVALID and "okkt_analyze" in lib.okkt_last_error(h._h).decode()
    h.analyze(d.raw(np.zeros(len(d.rowval))))
    assert lib.okkt_debug_row_map(h._h, None) == L.OKKT_ERR_INVALID and "null pointer" in lib.okkt_last_error(h._h).decode()
    assert query(h) == d.query()
    assert lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        query(h)
    finalize_b(h)


# ---- residual ------------------------------------------------------------------------------------------------------------------------

def exact_rows(d, nz, b, x, r, rows):
    """worst err / bound over `rows` of |r_i - r_exact| <= u |r_exact| + 4 nnz_i u^2 (|A||x|)_i; asserts the bound"""
    rv = rd.row_values(d, nz, rows)
    worst = 0.0
    for i in rows:
        ex, ax = rd.exact_residual(rv[i], b[i], x)
        bound = rd.residual_bound(ex, ax, len(rv[i]))
        err = abs(Fraction(float(r[i])) - ex)
        assert err <= bound, (d.name, i, float(err), float(bound))
        if bound:
            worst = max(worst, float(err / bound))
    return worst


def nan_targets(d):
    """(label, row whose r must be NaN or None, column of x that holds the NaN)"""
    out = []
    for r in rd.resid_edges(d):
        ks = [k for k in range(len(d.rows[r])) if k % d.lpr == d.lpr - 1 and d.rows[r][k][0] != r]
        if ks and not d.is_long(r):
            out.append(("last lane of a short row", r, d.rows[r][ks[-1]][0]))
            break
    for r in d.long_rows[:1]:
        p = 255 if d.rows[r][255][0] != r else 254
        assert d.owner(r, p)[1] == 3
        out.append(("wave 3 of a long row", r, d.rows[r][p][0]))
    if d.nb_short > 256:
        out.append(("a row of workgroup 256", d.n - 1, d.n - 2))
    if "empty" in d.edge:
        out.append(("an empty row", None, d.edge["empty"]))
    return out


@pytest.mark.parametrize("name", rd.ALL_DESIGNS)
def test_residual(name):
    d = CAT[name]
    nz = rd.base_values(d)
    h = handle(d, nz if d.factorable else None)
    edges = rd.resid_edges(d)
    rows = rd.checked_rows(d)
    plants = [edges[q % len(edges)] for q in range(NRHS)]
    if name == "tridiag-16385":
        plants[0] = d.n - 1                                           # the row of workgroup 256
    XB = [rd.plain_rhs(d, nz, q, plants[q]) for q in range(NRHS)]
    X, B = np.array([x for x, _ in XB]), np.array([b for _, b in XB])
    R7, om7 = h.residual(nz, B, X)                                    # 4 + 3
    # exact arithmetic: every checked row of the first right-hand side, the edge rows of the others
    worst = exact_rows(d, nz, B[0], X[0], R7[0], rows)
    for q in range(1, NRHS):
        worst = max(worst, exact_rows(d, nz, B[q], X[q], R7[q], edges))
    # omega is the planted row's ratio, its denominator from exact arithmetic, to the roundings of the denominator and the division
    worst_om = 0.0
    for q in range(NRHS):
        i = plants[q]
        row = rd.row_values(d, nz, [i])[i]
        den = rd.exact_dot(row, X[q], absolute=True) + abs(Fraction(float(B[q][i])))
        want = abs(Fraction(float(R7[q][i]))) / den
        err = abs(Fraction(float(om7[q])) - want) / want
        assert err <= (len(row) + 3) * Fraction(U), (name, q, i, float(om7[q]), float(want))
        worst_om = max(worst_om, float(err / ((len(row) + 3) * Fraction(U))))
    # every count of right-hand sides gives the bits of the single ones: 1, 2, 3, 4 alone, 2 and 3 as the tails of 6 and 7
    for q in range(NRHS):
        r1, o1 = h.residual(nz, B[q], X[q])
        assert np.array_equal(r1, R7[q]) and o1 == om7[q], (name, q)
    for lo, hi in ((0, 6), (0, 2), (4, 7), (0, 4), (2, 5), (5, 7)):
        Rq, oq = h.residual(nz, B[lo:hi], X[lo:hi])
        assert np.array_equal(Rq, R7[lo:hi]) and np.array_equal(oq, om7[lo:hi]), (name, lo, hi)
    Rb, ob = h.residual(nz, B, X)
    assert np.array_equal(Rb, R7) and np.array_equal(ob, om7)         # two calls: identical bits
    dn, db, dx, dr = h.dev_upload(nz), h.dev_upload(B), h.dev_upload(X), h.dev_alloc(8 * max(B.size, 1))
    od = h.residual_dev(dn, db, dx, dr, NRHS)
    assert np.array_equal(h.dev_download(dr, B.shape), R7) and np.array_equal(od, om7)
    for p in (dn, db, dx, dr):
        h.dev_free(p)
    # the cancelling set: double-double or nothing
    nzc, xc, bc, done = rd.cancelling(d)
    rc, _ = h.residual(nzc, bc, xc)
    worst_c = exact_rows(d, nzc, bc, xc, rc, rows)
    # a NaN in x that one lane, one wave, one partial or nobody reads
    nans = []
    for label, row, col in nan_targets(d):
        Xn = X[:4].copy()
        Xn[1, col] = np.nan
        Rn, on = h.residual(nz, B[:4], Xn)
        assert np.isnan(on[1]), (name, label)
        if row is None:
            assert np.array_equal(Rn[1], R7[1])                       # nobody reads x there: r is untouched, omega is NaN all the same
        else:
            assert np.isnan(Rn[1][row]), (name, label, row)
            touched = {c for c, _ in d.rows[col]}
            keep = np.array([i not in touched for i in range(d.n)])
            assert np.array_equal(Rn[1][keep], R7[1][keep])
        for q in (0, 2, 3):
            assert np.array_equal(Rn[q], R7[q]) and on[q] == om7[q], (name, label, q)
        nans.append(label)
    if d.factorable and name != "zero-last":
        # the DEN instantiation: berr of okkt_forward_error is omega of the same pass
        for lo, hi in ((0, 7), (0, 6), (0, 1)):
            _, berr = h.forward_error(nz, B[lo:hi], X[lo:hi])
            assert np.array_equal(np.atleast_1d(berr), om7[lo:hi]), (name, lo, hi)
        # ||r||_inf of the refinement loop is max |r_i| of the residual of the x it returns
        xs, info = h.ls_solve_refine(nz, B[0], max_steps=0)
        rs, os_ = h.residual(nz, B[0], xs)
        assert info["resid_inf"] == np.max(np.abs(rs)) and info["omega"] == os_, (name, info)
    record("REFINE", test="row_map_edges", name=name, n=d.n, query=list(d.query()), worst_over_bound=worst, worst_cancelling=worst_c,
           worst_omega_over_bound=worst_om, cancelling_rows=len(done), nan=nans)
    finalize_b(h)


# ---- scaling -------------------------------------------------------------------------------------------------------------------------

def scaled(h, d, nz, sweeps):
    h.set_scaling("ruiz", sweeps)
    h.ls_factor_b(d.raw(nz), d.n - len(d.last), len(d.last))
    return h.scaling(), h.scaling_info()


def same_scaling(d, nz, sweeps, s, info, what):
    s_ref, _, iref = sr.ruiz(d.raw(nz), sweeps)
    assert np.array_equal(s, s_ref), (d.name, what, sweeps, np.flatnonzero(s != s_ref)[:5])
    assert info["rowmax_min"] == iref["rowmax_min"] and info["rowmax_max"] == iref["rowmax_max"], (d.name, what, sweeps, info, iref)
    assert info["zero_rows"] == iref["zero_rows"], (d.name, what, sweeps)
    return iref


@pytest.mark.parametrize("name", rd.FACTORED_DESIGNS)
def test_scaling(name):
    d = CAT[name]
    h = handle(d)
    sets = rd.planted_max_sets(d)
    if not sets:
        sets = [(rd.base_values(d), [])]
    extreme_ok = 0
    for nz, plants in sets:
        for sweeps in (1, 3):
            s, info = scaled(h, d, nz, sweeps)
            iref = same_scaling(d, nz, sweeps, s, info, plants)
            off = [r for r, p in plants if d.rows[r][p][0] != r]
            if sweeps == 1 and off and name != "lpr16-nodiag":
                rm = np.where(iref["rowmax"] > 0, iref["rowmax"], np.inf)
                assert int(np.argmin(rm)) in off and info["rowmax_min"] == rm[off].min()     # the extreme is an edge row's
                extreme_ok += 1
        s2, info2 = scaled(h, d, nz, 3)
        assert np.array_equal(s2, s) and info2 == info                                       # two calls: identical bits
    # an Inf at a deciding position is skipped
    nz, plants = sets[0]
    infs = 0
    for r, p in plants:
        bad = nz.copy()
        bad[d.pairs[d.rows[r][p][1]][2]] = np.inf
        for sweeps in (1, 3):
            s, info = scaled(h, d, bad, sweeps)
            same_scaling(d, bad, sweeps, s, info, ("inf", r, p))
        infs += 1
    if name == "zero-last":
        s, info = scaled(h, d, rd.base_values(d), 3)
        assert info["zero_rows"] == 1 and s[d.n - 1] == 1.0
    record("SCALING", test="row_map_edges", name=name, n=d.n, sets=len(sets), plants=sum(len(p) for _, p in sets),
           extreme_is_planted_row=extreme_ok, inf_positions=infs, worst_over_bound=0.0)
    finalize_b(h)


# ---- ||F||_1 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rd.FACTORED_DESIGNS)
def test_norm1(name):
    d = CAT[name]
    h = handle(d, rd.base_values(d))
    worst = 0.0
    cases = 0
    for r in sorted(set(d.edge.values())):
        if name == "zero-last" and r == d.n - 1:
            continue
        nz = rd.norm1_set(d, r)                                        # (r in d.last: no stored diagonal, the `hasd` branch with shift 0)
        row = rd.row_values(d, nz, [r])[r]
        exact = rd.exact_row_sum(row)
        bound = rd.norm1_bound(len(row), 256 if d.is_long(r) else d.lpr) * exact
        got = h.condest(nz)["norm1"]
        err = abs(Fraction(float(got)) - exact)
        assert err <= bound, (name, r, float(got), float(exact), float(err / bound))
        worst = max(worst, float(err / bound))
        assert h.condest(nz)["norm1"] == got                           # two calls: identical bits
        cases += 1
    record("CONDEST", test="row_map_edges", name=name, n=d.n, rows=cases, worst_over_bound=worst)
    finalize_b(h)
