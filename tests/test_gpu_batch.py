"""Uniform batches on the GPU: every item of a batch, in level mode and in item mode, against a fresh
single handle that factors and solves the same values -- flag, inertia, D, the factor and the solutions as bits.

The plans are small on purpose (designed trees of front_trees.py built without amalgamation, the hanging chain, S-tiny): what can go
wrong is an item reaching into another item's slot, a level launched out of order, a block size that changes the arithmetic, or a
slot that keeps something from the batch before."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["level", "item"]
NRHS = (1, 2, 3, 4, 5)          # column groups of 1, 2, 4 and 4 + 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Equal as bits (NaNs included), which is what np.array_equal asks of finite values and more."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Plan:
    """A pattern (lower triangle, CSC arrays as the C ABI takes them), how to analyse it, the wanted inertia, value sets."""

    def __init__(self, colptr, rowval, base, n, m, perm=None, sym="symmetric", **opts):
        self.colptr, self.rowval, self.base = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64), np.asarray(base, np.float64)
        self.dim = len(self.colptr) - 1
        self.n, self.m, self.perm, self.sym, self.opts = n, m, perm, sym, opts

    def matrix(self, vals):
        return (self.dim, self.colptr, self.rowval, np.ascontiguousarray(vals), 0)

    def handle(self):
        h = linear_solver_HIP(self.sym, False, False, **self.opts)
        initialize_b(h)
        if self.perm is not None:
            h.set_perm(self.perm)
        h.analyze(self.matrix(self.base))
        return h

    def values(self, B, seed=0):
        """B value sets: every entry of the base scaled by its own factor in [0.7, 1.3] (signs, and so the designed inertia, stay)."""
        rng = np.random.default_rng(100 + seed)
        return self.base[None, :] * rng.uniform(0.7, 1.3, size=(B, len(self.base)))

    def diag_mask(self):
        cols = np.repeat(np.arange(self.dim), np.diff(self.colptr))
        return cols == self.rowval


def from_design(roots, **opts):
    d = ft.build(roots)
    A = sp.csc_matrix(d.A)
    return Plan(A.indptr, A.indices, A.data, d.npos, d.nneg, perm=d.perm, ordering=2, **dict(ft.NO_RELAX, **opts))


def from_kkt(prob, delta):
    K = sp.tril(synth.augmented_matrix(prob, delta=delta), format="csc")
    K.sort_indices()
    return Plan(K.indptr, K.indices, K.data, prob["n"], prob["m"])


def three_levels():
    # leaves of 32 and of 33 rows in ONE level: the single handle runs them with 64 and with 256 threads, the batch with 256
    return [ft.N(40, 0, *[ft.N(17, 16, *[ft.N(16 + (i % 2), 16) for i in range(20)]) for _ in range(3)])]


def with_duplicates():
    """The scattered design with every fifth entry split into two halves (and one diagonal entry into three parts): a raw CSC with
    duplicated entries, which the assembly sums serially in input order."""
    d = ft.build([ft.N(30, 0, ft.N(10, 12, scatter=True), ft.N(8, 20, scatter=True))])
    A = sp.csc_matrix(d.A)
    colptr, rowval, val = [0], [], []
    for j in range(A.shape[0]):
        for e in range(A.indptr[j], A.indptr[j + 1]):
            parts = 3 if (A.indices[e] == j and j % 7 == 0) else (2 if e % 5 == 0 else 1)
            for q in range(parts):
                rowval.append(A.indices[e])
                val.append(A.data[e] * (0.5 if parts == 2 else (0.25, 0.5, 0.25)[q] if parts == 3 else 1.0))
        colptr.append(len(rowval))
    return Plan(colptr, rowval, val, d.npos, d.nneg, perm=d.perm, ordering=2, **ft.NO_RELAX)


PLANS = {
    "single-front": (lambda: from_design([ft.N(12)]), (1, 3, 7, 130)),
    "leaves-only": (lambda: from_design([ft.N(5), ft.N(33), ft.N(7), ft.N(20)]), (1, 3, 7, 130)),
    "three-levels-32-33": (lambda: from_design(three_levels()), (1, 3, 7)),
    "front-136": (lambda: from_design([ft.N(136)], small_front_max=136), (1, 3, 7)),
    "scattered": (lambda: from_design([ft.N(30, 0, ft.N(10, 12, scatter=True), ft.N(8, 20, scatter=True))]), (1, 3, 7)),
    "duplicates": (with_duplicates, (1, 3, 7)),
    "chain40": (lambda: from_kkt(synth.hanging_chain(N_h=40), 1.0), (1, 3, 7)),
    "S-tiny": (lambda: from_kkt(synth.make_config("S-tiny", seed=3), 1e-4), (1, 3, 7)),
}


def single(plan, vals, rhs_sets=()):
    """A fresh handle: flag, inertia, D, L, and the solutions of every block of right-hand sides (nrhs x dim each)."""
    h = plan.handle()
    flag = h.ls_factor_b(plan.matrix(vals), plan.n, plan.m)
    out = dict(flag=flag, inertia=h.inertia, D=h.diag(), L=h.factor_csc(), X=[])
    for Bk in rhs_sets:
        Bk = np.ascontiguousarray(Bk)
        X = np.empty_like(Bk)
        h._check(h._lib.okkt_solve(h._h, L.p_f64(Bk), L.p_f64(X), Bk.shape[0]), "okkt_solve")
        out["X"].append(X)
    finalize_b(h)
    return out


def rhs_sets(dim, item):
    rng = np.random.default_rng(1000 + item)
    return [rng.normal(size=(k, dim)) for k in NRHS]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The plan, its value sets and what fresh handles make of them: computed once, shared by both modes."""
    make, sizes = PLANS[name]
    plan = make()
    Bmax = max(sizes)
    vals = plan.values(Bmax)
    # right-hand sides for the first seven items (every column group); the items beyond solve one column
    ref = [single(plan, vals[b], rhs_sets(plan.dim, b) if b < 7 else rhs_sets(plan.dim, b)[:1]) for b in range(Bmax)]
    return plan, vals, ref


def check_factors(h, ref, items):
    for b in items:
        h.batch_select(b)
        assert same(h.diag(), ref[b]["D"]), f"D of item {b}"
        Lb = h.factor_csc()
        assert np.array_equal(Lb.indptr, ref[b]["L"].indptr) and np.array_equal(Lb.indices, ref[b]["L"].indices)
        assert same(Lb.data, ref[b]["L"].data), f"L of item {b}"
        assert h.inertia == ref[b]["inertia"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(PLANS))
def test_every_item_equals_a_fresh_handle(name, mode):
    plan, vals, ref = reference(name)
    sizes = PLANS[name][1]
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    assert h.batch_query()["eligible"] == 1
    h.batch_reserve(max(sizes), nrhs_max=max(NRHS), mode=mode)
    for B in sizes:
        flags = h.ls_factor_batch(vals[:B], plan.n, plan.m)
        assert h.batch_mode_used() == mode
        assert [int(f) for f in flags] == [ref[b]["flag"] for b in range(B)]
        assert h.batch_inertia == [ref[b]["inertia"] for b in range(B)]
        for k, nrhs in enumerate(NRHS if B <= 7 else NRHS[:1]):
            rhs = np.stack([rhs_sets(plan.dim, b)[k] for b in range(B)])
            X = h.ls_solve_batch(rhs)
            for b in range(B):
                assert same(X[b], ref[b]["X"][k]), f"B = {B}, nrhs = {nrhs}: solution of item {b}"
        check_factors(h, ref, range(B) if B <= 7 else (0, 64, B - 1))
    h.batch_release()
    finalize_b(h)


@pytest.mark.parametrize("mode", MODES)
def test_shared_values_with_shifts(mode):
    """val_stride = 0 and a shift per item, against per-item values with the shift added to the first nshift diagonal entries."""
    plan, vals, _ = reference("S-tiny")
    base = vals[0]
    shifts = np.array([0.0, 1e-8, 3e-3, 0.5, 7.0])
    nshift = plan.n
    dm = plan.diag_mask() & (plan.rowval < nshift)
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    h.batch_reserve(len(shifts), nrhs_max=2, mode=mode)
    flags = h.ls_factor_batch(base, plan.n, plan.m, shifts=shifts, nshift=nshift)
    rhs = np.stack([rhs_sets(plan.dim, b)[1] for b in range(len(shifts))])
    X = h.ls_solve_batch(rhs)
    for b, sh in enumerate(shifts):
        v = base.copy()
        v[dm] = v[dm] + sh
        r = single(plan, v, [rhs[b]])
        assert int(flags[b]) == r["flag"] and h.batch_inertia[b] == r["inertia"]
        assert same(X[b], r["X"][0])
        check_factors(h, {b: r}, [b])
    finalize_b(h)


@pytest.mark.parametrize("mode", MODES)
def test_definite_kind(mode):
    """sym = definite: the Cholesky rule (every pivot > 0), one item with a negative diagonal entry fails alone."""
    n = 50
    A = sp.diags([np.full(n, 4.0), np.full(n - 1, -1.0), np.full(n - 3, 0.5)], [0, -1, -3], format="csc")
    plan = Plan(A.indptr, A.indices, A.data, n, 0, sym="definite")
    vals = plan.values(3)
    vals[1, np.flatnonzero(plan.diag_mask())[17]] = -2.0
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    h.batch_reserve(3, nrhs_max=1, mode=mode)
    flags = h.ls_factor_batch(vals, n, 0)
    ref = {b: single(plan, vals[b]) for b in range(3)}
    assert [int(f) for f in flags] == [1, 0, 1] == [ref[b]["flag"] for b in range(3)]
    assert h.batch_inertia == [ref[b]["inertia"] for b in range(3)]
    check_factors(h, ref, range(3))
    finalize_b(h)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poison", ["zero-pivot", "nan"])
def test_a_bad_item_stays_alone(poison, mode):
    """The middle item has an exact zero first pivot, or holds a NaN: it is counted in that item alone, the neighbours' counts, D,
    factors and solutions are those of fresh handles."""
    plan, vals, ref = reference("leaves-only")
    v = vals[:3].copy()
    first = int(plan.perm[0])            # the first pivot of the first front, in the caller's numbering
    e = next(e for e in range(plan.colptr[first], plan.colptr[first + 1]) if plan.rowval[e] == first)
    v[1, e] = 0.0 if poison == "zero-pivot" else np.nan
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    h.batch_reserve(3, nrhs_max=1, mode=mode)
    flags = h.ls_factor_batch(v, plan.n, plan.m)
    mid = single(plan, v[1])
    assert int(flags[1]) == 0 == mid["flag"] and h.batch_inertia[1] == mid["inertia"]
    assert (mid["inertia"][2] > 0) if poison == "zero-pivot" else (mid["inertia"][3] > 0)
    assert [int(flags[0]), int(flags[2])] == [ref[0]["flag"], ref[2]["flag"]] == [1, 1]
    assert [h.batch_inertia[0], h.batch_inertia[2]] == [ref[0]["inertia"], ref[2]["inertia"]]
    rhs = np.stack([rhs_sets(plan.dim, b)[0] for b in range(3)])
    X = h.ls_solve_batch(rhs)
    for b in (0, 2):
        assert same(X[b], ref[b]["X"][0])
    check_factors(h, ref, (0, 2))
    h.batch_select(1)
    assert same(h.diag(), mid["D"])
    finalize_b(h)


@pytest.mark.parametrize("mode", MODES)
def test_two_batches_in_the_same_slots(mode):
    """A second batch in the slots of the first: nothing of the first is left in it (and a smaller batch leaves the slots beyond it alone)."""
    plan, vals, ref = reference("three-levels-32-33")
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    h.batch_reserve(4, nrhs_max=4, mode=mode)
    first = h.ls_factor_batch(vals[:4], plan.n, plan.m)
    assert [int(f) for f in first] == [ref[b]["flag"] for b in range(4)]
    other = plan.values(3, seed=9)
    other[:, plan.diag_mask()] *= 1.5
    flags = h.ls_factor_batch(other, plan.n, plan.m)
    rhs = np.stack([rhs_sets(plan.dim, b)[3] for b in range(3)])
    X = h.ls_solve_batch(rhs)
    for b in range(3):
        r = single(plan, other[b], [rhs[b]])
        assert int(flags[b]) == r["flag"] and h.batch_inertia[b] == r["inertia"]
        assert same(X[b], r["X"][0])
        check_factors(h, {b: r}, [b])
    with pytest.raises(OkktError):      # the fourth slot belongs to no factored item of the last batch
        h.batch_select(3)
    finalize_b(h)


@pytest.mark.parametrize("mode", MODES)
def test_selected_slot_serves_the_other_entry_points(mode):
    """After batch_select the handle is what okkt_factor of that item would have left: refinement and the selected inverse give the
    same bits as on the fresh handle."""
    plan, vals, _ = reference("chain40")
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    h.batch_reserve(3, nrhs_max=1, mode=mode)
    h.ls_factor_batch(vals[:3], plan.n, plan.m)
    h.batch_select(1)
    f = plan.handle()
    f.ls_factor_b(plan.matrix(vals[1]), plan.n, plan.m)
    b = rhs_sets(plan.dim, 1)[1]
    xs, infos = h.ls_solve_refine(vals[1], b, max_steps=3)
    xf, inff = f.ls_solve_refine(vals[1], b, max_steps=3)
    assert same(xs, xf) and infos["steps"] == inff["steps"] and same(infos["omega_per_rhs"], inff["omega_per_rhs"])
    h.selinv()
    f.selinv()
    assert same(h.inverse_diag(), f.inverse_diag())
    assert same(h.ls_solve(b[0]), f.ls_solve(b[0]))
    # and the handle's own factorisation afterwards is untouched by the slots
    assert h.ls_factor_b(plan.matrix(vals[2]), plan.n, plan.m) == f.ls_factor_b(plan.matrix(vals[2]), plan.n, plan.m)
    assert same(h.diag(), f.diag())
    finalize_b(h)
    finalize_b(f)


def test_refusals_on_the_device():
    plan, vals, _ = reference("S-tiny")
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    lib = h._lib
    with pytest.raises(OkktError, match="no slots"):
        h.ls_factor_batch(vals[:2], plan.n, plan.m)
    h.batch_reserve(2, nrhs_max=2)
    with pytest.raises(OkktError, match="reserved"):
        h.ls_factor_batch(vals[:3], plan.n, plan.m)
    with pytest.raises(OkktError, match="n \\+ m"):
        h.ls_factor_batch(vals[:2], plan.n + 1, plan.m)
    with pytest.raises(OkktError, match="no factored batch"):
        h.ls_solve_batch(np.zeros((2, plan.dim)))
    assert list(h.ls_factor_batch(vals[:2], plan.n, plan.m)) == [1, 1]
    with pytest.raises(OkktError, match="nrhs"):
        h.ls_solve_batch(np.zeros((2, 3, plan.dim)))
    h.set_scaling("ruiz")
    with pytest.raises(OkktError, match="scaling"):
        h.ls_factor_batch(vals[:2], plan.n, plan.m)
    with pytest.raises(OkktError, match="scaling"):
        h.batch_reserve(2)
    h.set_scaling("none")
    # a plan with big fronts: refused with the reason, the handle keeps working
    prob = synth.make_config("S-small", seed=3)
    big = from_kkt(prob, 1e-4)
    g = big.handle()
    assert g.stats()["n_big_fronts"] > 0
    assert lib.okkt_batch_reserve(g._h, 2, 1) == L.OKKT_ERR_INVALID and "small fronts only" in lib.okkt_last_error(g._h).decode()
    assert g.ls_factor_b(big.matrix(big.base), big.n, big.m) == 1
    # a re-analysis releases the slots
    other, small = reference("leaves-only")[0], reference("single-front")[0]
    h2 = other.handle()
    h2.batch_reserve(2)
    h2.set_perm(small.perm)
    h2.analyze(small.matrix(small.base))
    with pytest.raises(OkktError, match="no slots"):
        h2.ls_factor_batch(small.values(2), small.n, small.m)
    h2.batch_reserve(2)
    assert list(h2.ls_factor_batch(small.values(2), small.n, small.m)) == [1, 1]
    finalize_b(h)
    finalize_b(g)
    finalize_b(h2)


@pytest.mark.parametrize("rebuilt", [False, True])
def test_a_partition_set_after_the_reservation_is_refused(rebuilt):
    """okkt_dist_set_partition works on the analysed handle: the plan the slots were laid out for is gone.  Every batch call refuses,
    also after another call has set the (partitioned) plan up again, and a new reservation is refused with the reason."""
    plan, vals, ref = reference("three-levels-32-33")
    h = plan.handle()
    assert h.stats()["n_big_fronts"] == 0
    h.batch_reserve(3, nrhs_max=1)
    assert [int(f) for f in h.ls_factor_batch(vals[:3], plan.n, plan.m)] == [ref[b]["flag"] for b in range(3)]
    assert h._lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    if rebuilt:      # sets the device plan up again, as a partitioned one, and runs nothing on it (then refuses: there is no factor)
        assert h._lib.okkt_get_diag(h._h, L.p_f64(np.zeros(plan.dim))) == L.OKKT_ERR_INVALID
    with pytest.raises(OkktError, match="no slots|device plan has changed"):
        h.ls_factor_batch(vals[:3], plan.n, plan.m)
    with pytest.raises(OkktError, match="no slots|device plan has changed"):
        h.ls_solve_batch(np.zeros((3, plan.dim)))
    with pytest.raises(OkktError, match="no slots|device plan has changed"):
        h.batch_select(0)
    with pytest.raises(OkktError, match="partitioned"):
        h.batch_reserve(3)
    # back to one part: a new reservation works and gives the same bits
    assert h._lib.okkt_dist_set_partition(h._h, 1, 0) == L.OKKT_OK
    h.batch_reserve(3, nrhs_max=1)
    assert [int(f) for f in h.ls_factor_batch(vals[:3], plan.n, plan.m)] == [ref[b]["flag"] for b in range(3)]
    check_factors(h, ref, range(3))
    finalize_b(h)
