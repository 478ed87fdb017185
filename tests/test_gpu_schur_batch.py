"""Scenario batches on the GPU: B items in Schur mode on one designed pattern (schur_batch_designs.py).

1. every item, as bits, against a fresh single handle in Schur mode (schur_batch_designs.check_items);
2. the sums of the S_b and of the r2_b, as bits, against the grouping rule of okkt.h evaluated in NumPy with explicit loops;
3. the fused solve, as bits, against its own parts and against the same decomposition done with B single handles, a NumPy sum and
   okkt_schur_factor(S) on one of them;
4. it solves the arrowhead system: forward error against numpy.linalg.solve on the dense matrix at most 1e-11, the bar
   test_gpu_schur_trees.py sets for the fused Schur solve of one handle on such designs;
5. inertia_total is the eigenvalue sign count of the dense arrowhead matrix;
6. isolation: an item with an exact zero pivot or a NaN changes nothing in the other items; a second, smaller batch in the same slots
   sums its own items only;
7. case 1 once more under OKKT_DEBUG_POISON=1 (schur_batch_case.py, a child process: the switch is read at allocation)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schur_batch_designs as sbd  # noqa: E402
from schur_batch_designs import NRHS, group_sum, same  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_X = 1e-11


def mid_size(sc):
    """the batch size of the tests that need one: 3 (2 where the design has no other)"""
    return 3 if 3 in sc.sizes else sc.sizes[0]


def sym(ns, seed):
    """a linking block: symmetric, of the size of the entries of the S_b"""
    M = np.random.default_rng(300 + seed).normal(size=(ns, ns))
    return (M + M.T) * 0.5 + np.diag(np.full(ns, 4.0 * np.sqrt(ns)))


@pytest.mark.parametrize("name", sorted(sbd.DESIGNS))
def test_every_item_equals_a_fresh_single_handle(name):
    sbd.check_items(name)


@pytest.mark.parametrize("name", sorted(sbd.DESIGNS))
def test_sums_follow_the_grouping_rule(name):
    sc = sbd.scenario(name)
    vals = sc.vals(max(sc.sizes))
    h = sc.handle()
    h.schur_batch_reserve(max(sc.sizes), nrhs_max=max(NRHS))
    for B in sc.sizes:
        h.ls_factor_schur_batch(vals[:B], sc.n1pos, sc.n1neg)
        items = [h.schur_batch(b) for b in range(B)]
        S = h.schur_batch(-1)
        assert same(S, group_sum(items)), f"B = {B}: the sum of the S_b"
        assert same(S, S.T), f"B = {B}: the sum is not bitwise symmetric"
        if B > 2 * sbd.GROUP:      # from the second full group on the rule is not the plain left-to-right sum (with 33 items it still is)
            plain = np.zeros_like(S)
            for x in items:
                plain = plain + x
            assert not same(S, plain) or sc.ns <= 2
        for nrhs in (NRHS if B <= 7 else (1, 4)):
            rhs = sc.rhs(B, nrhs, seed=B)
            r2, r2i = h.schur_batch_condense(rhs, items=True)
            assert r2.shape == (nrhs, sc.ns) and r2i.shape == (B, nrhs, sc.ns)
            assert same(r2, group_sum(list(r2i))), f"B = {B}, nrhs = {nrhs}: the sum of the r2_b"
            assert same(h.schur_batch_condense(rhs), r2)
    h.schur_batch_release()
    finalize_b(h)


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "S_add-rhs0"])
@pytest.mark.parametrize("name", sorted(sbd.DESIGNS))
def test_fused_solve_as_bits(name, with_add):
    sc = sbd.scenario(name)
    B = mid_size(sc)
    vals = sc.vals(B)
    S_add = sym(sc.ns, 1) if with_add else None
    h = sc.handle()
    h.schur_batch_reserve(B, nrhs_max=max(NRHS))
    h.ls_factor_schur_batch(vals, sc.n1pos, sc.n1neg)
    sflag = h.schur_batch_factor(S_add)
    assert sflag == 1
    # the same decomposition with B single handles, the sums in NumPy by the rule, okkt_schur_factor(S) on the first of them
    singles = [sc.handle() for _ in range(B)]
    for b, hb in enumerate(singles):
        hb.ls_factor_schur(vals[b], sc.n1pos, sc.n1neg)
    S = group_sum([hb.schur() for hb in singles], add=S_add)
    assert singles[0].schur_factor(S) == 1
    assert h.schur_inertia == singles[0].schur_inertia
    tot = np.sum([hb.inertia for hb in singles], axis=0) + np.array(singles[0].schur_inertia)
    assert tuple(h.total_inertia) == tuple(int(t) for t in tot)
    for nrhs in NRHS:
        rhs = sc.rhs(B, nrhs, seed=10 + nrhs)
        rhs0 = np.random.default_rng(400 + nrhs).normal(size=(nrhs, sc.ns)) if with_add else None
        X = h.schur_batch_solve(rhs, rhs0)
        # x_L is the same in every item
        x2 = X[0][:, sc.idx]
        for b in range(1, B):
            assert same(X[b][:, sc.idx], x2), f"nrhs = {nrhs}: x_L of item {b}"
        # its own parts: the summed r2 (+ rhs0 last), the dense solve (read off x_L), the expansion
        assert same(h.schur_batch_expand(rhs, x2), X), f"nrhs = {nrhs}: the fused solve is not expand(x2)"
        # the single handles
        r2 = group_sum([hb.schur_condense(rhs[b]).reshape(nrhs, -1) for b, hb in enumerate(singles)], add=rhs0)
        r2b = h.schur_batch_condense(rhs)
        assert same(r2b if rhs0 is None else r2b + rhs0, r2)
        x2s = singles[0].schur_dense_solve(r2).reshape(nrhs, -1)
        assert same(x2, x2s), f"nrhs = {nrhs}: x_L against the dense solve of a single handle"
        for b, hb in enumerate(singles):
            assert same(hb.schur_expand(rhs[b], x2s).reshape(nrhs, -1), X[b]), f"nrhs = {nrhs}: item {b}"
        # device pointers, rhs and sol apart (the host entry stages both in one buffer: rhs aliasing sol), and in place
        d_rhs, d_sol = h.dev_upload(rhs), h.dev_alloc(rhs.nbytes)
        d_r0 = None if rhs0 is None else h.dev_upload(rhs0)
        h.schur_batch_solve_dev(d_rhs, d_sol, B, nrhs, d_rhs0=d_r0)
        assert same(h.dev_download(d_sol, rhs.shape), X)
        assert same(h.dev_download(d_rhs, rhs.shape), rhs)
        h.schur_batch_solve_dev(d_rhs, d_rhs, B, nrhs, d_rhs0=d_r0)
        assert same(h.dev_download(d_rhs, rhs.shape), X)
        for p in (d_rhs, d_sol, d_r0):
            if p is not None:
                h.dev_free(p)
    for hb in singles:
        finalize_b(hb)
    finalize_b(h)


def arrowhead(sc, B, S_add):
    """the dense arrowhead matrix of items 0 .. B-1: the interiors on the diagonal, the linking variables last, A0 = sum_b A22_b + S_add"""
    n1, ns = sc.n1, sc.ns
    K = np.zeros((B * n1 + ns, B * n1 + ns))
    for b in range(B):
        M = sc.dense_item(b)
        s = slice(b * n1, (b + 1) * n1)
        K[s, s] = M[:n1, :n1]
        K[s, B * n1:] = M[:n1, n1:]
        K[B * n1:, s] = M[n1:, :n1]
        K[B * n1:, B * n1:] += M[n1:, n1:]
    if S_add is not None:
        K[B * n1:, B * n1:] += S_add
    return K


@pytest.mark.parametrize("name", sorted(sbd.DESIGNS))
def test_it_solves_the_arrowhead_system(name):
    sc = sbd.scenario(name)
    B = mid_size(sc)
    n1, ns, perm = sc.n1, sc.ns, sc.d.perm
    S_add = sym(ns, 2)
    K = arrowhead(sc, B, S_add)
    nrhs = 2
    rhs = sc.rhs(B, nrhs, seed=21)
    rhs0 = np.random.default_rng(22).normal(size=(nrhs, ns))
    big = np.zeros((nrhs, B * n1 + ns))
    for b in range(B):
        big[:, b * n1:(b + 1) * n1] = rhs[b][:, perm[:n1]]
        big[:, B * n1:] += rhs[b][:, sc.idx]
    big[:, B * n1:] += rhs0
    XT = np.linalg.solve(K, big.T).T
    h = sc.handle()
    h.schur_batch_reserve(B, nrhs_max=nrhs)
    h.ls_factor_schur_batch(sc.vals(B), sc.n1pos, sc.n1neg)
    assert h.schur_batch_factor(S_add) == 1
    X = h.schur_batch_solve(rhs, rhs0)
    got = np.zeros_like(XT)
    for b in range(B):
        got[:, b * n1:(b + 1) * n1] = X[b][:, perm[:n1]]
    got[:, B * n1:] = X[0][:, sc.idx]
    e = max(float(np.max(np.abs(g - t)) / np.max(np.abs(t))) for g, t in zip(got, XT))
    print(f"SCHURBATCH arrowhead {name} B={B} dim={K.shape[0]} forward error {e:.3e}")
    assert e <= TOL_X, e
    finalize_b(h)


@pytest.mark.parametrize("name", ["set-65-small-only", "three-levels-chain", "childless-set"])
def test_total_inertia_is_the_arrowhead_matrix_s(name):
    sc = sbd.scenario(name)
    B = 3
    for S_add in (None, -sym(sc.ns, 3)):
        w = np.linalg.eigvalsh(arrowhead(sc, B, S_add))
        assert np.min(np.abs(w)) > 1e-8
        h = sc.handle()
        h.schur_batch_reserve(B)
        h.ls_factor_schur_batch(sc.vals(B), sc.n1pos, sc.n1neg)
        items = np.array(h.schur_batch_inertia)
        assert (items[:, 1] > 0).all() and (items[:, 0] > 0).all(), "the interiors are meant to be indefinite"
        assert (items.sum(axis=1) == sc.n1).all()
        assert h.schur_batch_factor(S_add) == 1
        assert tuple(h.total_inertia) == (int((w > 0).sum()), int((w < 0).sum()), 0, 0)
        finalize_b(h)


def first_diagonal(sc):
    """the place, in the value array, of the diagonal entry of the first pivot of the first front (a leaf)"""
    j = int(sc.d.perm[0])
    e = int(sc.colptr[j])
    assert sc.rowval[e] == j
    return e


@pytest.mark.parametrize("what", ["zero-pivot", "nan"])
def test_a_bad_item_stays_alone(what):
    name, B, bad = "set-65-small-only", 5, 2
    sc, vals, ref = sbd.reference(name, B)
    vals = vals.copy()
    vals[bad, first_diagonal(sc)] = 0.0 if what == "zero-pivot" else np.nan
    lone = sbd.single_item(sc, vals[bad], [])
    h = sc.handle()
    h.schur_batch_reserve(B, nrhs_max=2)
    flags = h.ls_factor_schur_batch(vals, sc.n1pos, sc.n1neg)
    for b in range(B):
        want = lone if b == bad else ref[b]
        assert int(flags[b]) == want["flag"] and h.schur_batch_inertia[b] == want["inertia"], b
        assert same(h.schur_batch(b), want["S"]), b
    assert int(flags[bad]) == 0
    zer, nonf = h.schur_batch_inertia[bad][2], h.schur_batch_inertia[bad][3]
    assert (zer >= 1 if what == "zero-pivot" else True) and zer + nonf >= 1
    rhs = sc.rhs(B, 2, seed=31)
    _, r2i = h.schur_batch_condense(rhs, items=True)
    good = sc.handle()
    for b in range(B):
        if b == bad:
            continue
        good.ls_factor_schur(vals[b], sc.n1pos, sc.n1neg)
        assert same(r2i[b], good.schur_condense(rhs[b]).reshape(2, -1)), b
        h.schur_batch_select(b)
        assert same(h.diag(), ref[b]["D"])
    finalize_b(good)
    # the sum holds the bad item's non-finite entries, and the dense factor reports them
    assert not np.isfinite(h.schur_batch(-1)).all()
    assert h.schur_batch_factor() == 0
    assert h.schur_inertia[3] > 0 and h.total_inertia[3] >= h.schur_inertia[3]
    finalize_b(h)


def test_shifts_are_added_to_the_assembled_diagonal():
    """shift[b] on the first nshift diagonal entries (original numbering), interior and set alike: the bits of the same items with the
    shift added to their values by the caller"""
    sc = sbd.scenario("set-65-small-only")
    B, nshift = 3, sc.dim // 2
    shifts = np.array([0.0, 1e-3, 0.5])
    vals = sc.vals(B)
    cols = np.repeat(np.arange(sc.dim), np.diff(sc.colptr))
    dm = (cols == sc.rowval) & (sc.rowval < nshift)
    assert dm[sc.colptr[sc.idx[sc.idx < nshift]]].all() and (sc.idx < nshift).any(), "the shift is meant to reach the set's diagonal too"
    shifted = vals.copy()
    shifted[:, dm] += shifts[:, None]
    got = {}
    for key, (v, sh) in {"shift": (vals, shifts), "values": (shifted, None)}.items():
        h = sc.handle()
        h.schur_batch_reserve(B)
        flags = h.ls_factor_schur_batch(v, sc.n1pos, sc.n1neg, shifts=sh, nshift=nshift)
        S = [h.schur_batch(b) for b in range(B)]
        D = []
        for b in range(B):
            h.schur_batch_select(b)
            D.append(h.diag())
        got[key] = (list(flags), h.schur_batch_inertia, S, D, h.schur_batch(-1))
        finalize_b(h)
    a, b = got["shift"], got["values"]
    assert a[0] == b[0] and a[1] == b[1]
    assert all(same(x, y) for x, y in zip(a[2], b[2])) and all(same(x, y) for x, y in zip(a[3], b[3])) and same(a[4], b[4])
    assert not same(a[2][2], sbd.reference("set-65-small-only", 3)[2][2]["S"])


def test_second_smaller_batch_sums_its_own_items_only():
    name = "set-65-small-only"
    sc = sbd.scenario(name)
    vals = sc.vals(7)
    h = sc.handle()
    h.schur_batch_reserve(7, nrhs_max=2)
    h.ls_factor_schur_batch(vals, sc.n1pos, sc.n1neg)
    first = h.schur_batch(-1)
    second = vals[[5, 3, 6]]
    h.ls_factor_schur_batch(second, sc.n1pos, sc.n1neg)
    items = [h.schur_batch(b) for b in range(3)]
    S = h.schur_batch(-1)
    assert same(S, group_sum(items)) and not same(S, first)
    _, _, ref = sbd.reference(name, 7)
    for b, src in enumerate((5, 3, 6)):
        assert same(items[b], ref[src]["S"])
    with pytest.raises(OkktError, match="outside"):
        h.schur_batch(3)
    rhs = sc.rhs(3, 2, seed=41)
    r2, r2i = h.schur_batch_condense(rhs, items=True)
    assert same(r2, group_sum(list(r2i)))
    with pytest.raises(OkktError, match="no factored batch of at least"):
        h.schur_batch_condense(sc.rhs(7, 1))
    assert h.schur_batch_factor() == 1
    X = h.schur_batch_solve(rhs)
    assert same(h.schur_batch_expand(rhs, X[0][:, sc.idx]), X)
    finalize_b(h)


def test_refusals_and_stale_reservations():
    sc = sbd.scenario("set-2-leaf")
    lib = L.load()
    h = sc.handle()
    vals = sc.vals(3)
    rhs = sc.rhs(3, 1)

    def refused(call, text):
        with pytest.raises(OkktError) as ei:
            call()
        assert f"({L.OKKT_ERR_INVALID})" in str(ei.value) and text in str(ei.value), str(ei.value)

    refused(lambda: h.ls_factor_schur_batch(vals, sc.n1pos, sc.n1neg), "no slots are reserved")
    refused(lambda: h.schur_batch(0), "no slots are reserved")
    refused(lambda: h.schur_batch_solve(rhs), "no slots are reserved")
    refused(lambda: h.schur_batch_select(0), "no slots are reserved")
    h.schur_batch_reserve(3, nrhs_max=2)
    refused(lambda: h.schur_batch(-1), "no factored batch")
    refused(lambda: h.schur_batch_factor(), "no factored batch")
    refused(lambda: h.ls_factor_schur_batch(sc.vals(4), sc.n1pos, sc.n1neg), "B must be in 1 .. the reserved 3")
    refused(lambda: h.ls_factor_schur_batch(vals, sc.n1pos + 1, sc.n1neg), "n1 + m1")
    h.ls_factor_schur_batch(vals, sc.n1pos, sc.n1neg)
    refused(lambda: h.schur_batch_solve(rhs), "no okkt_schur_batch_factor")
    S = np.zeros((sc.ns, sc.ns))
    assert lib.okkt_schur_batch_get(h._h, 0, L.p_f64(S), sc.ns - 1) == L.OKKT_ERR_INVALID and "ld < ns" in lib.okkt_last_error(h._h).decode()
    assert lib.okkt_schur_batch_factor(h._h, L.p_f64(S), sc.ns - 1, None, None) == L.OKKT_ERR_INVALID and "ld < ns" in lib.okkt_last_error(h._h).decode()
    assert h.schur_batch_factor() == 1
    refused(lambda: h.schur_batch_solve(sc.rhs(3, 3)), "nrhs outside")
    refused(lambda: h.schur_batch_solve(sc.rhs(2, 1)), "B is not that of the last")
    refused(lambda: h.schur_batch_select(3), "b outside")
    # the handle's own factor is not touched by the batch: there is none
    refused(lambda: h.schur_solve(rhs[0]), "no complete okkt_factor_schur")
    X = h.schur_batch_solve(rhs)
    # a new factorisation of the items makes the dense factor stale
    h.ls_factor_schur_batch(vals, sc.n1pos, sc.n1neg)
    refused(lambda: h.schur_batch_solve(rhs), "no okkt_schur_batch_factor")
    assert h.schur_batch_factor() == 1 and same(h.schur_batch_solve(rhs), X)
    # a changed set: the handle is not analysed, the reservation is stale -- released, and the call refused
    h.set_schur(sc.idx[::-1].copy())
    refused(lambda: h.schur_batch_solve(rhs), "the plan has changed")
    refused(lambda: h.schur_batch_solve(rhs), "no slots are reserved")
    h.set_perm(np.concatenate([sc.d.perm[:sc.n1], sc.idx[::-1]]))      # (the permutation ends with the set in its order)
    h.analyze(sc.matrix(np.zeros(len(sc.rowval))))
    h.schur_batch_reserve(2)
    h.schur_batch_release()
    refused(lambda: h.schur_batch(0), "no slots are reserved")
    finalize_b(h)


def test_items_under_debug_poison():
    """case 1 on two designs with the items' arenas, the partials and the r2 buffers starting as NaNs (a child process)"""
    env = dict(os.environ, OKKT_DEBUG_POISON="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schur_batch_case.py"), "set-65-small-only", "duplicates"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CASE_OK" in p.stdout, (p.stdout[-400:], p.stderr[-1500:])
