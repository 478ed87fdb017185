"""Schur mode on the host (okkt_set_schur): what the analysis builds for a chosen set, on host_symbolic_only
handles -- the set refused when it is malformed, placed last in its own order as one final supernode, an ordering-2 permutation
checked, a cleared set indistinguishable from none, and the Schur calls refused without a set."""
import numpy as np
import pytest

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP


def _handle(**opts):
    s = linear_solver_HIP("symmetric", host_symbolic_only=1, **opts)
    initialize_b(s)
    return s


def _kkt(seed=3):
    prob = synth.make_problem(600, 400, seed=seed)
    return synth.augmented_matrix(prob, delta=1e-8), prob["n"], prob["m"]


def _mixed_set(n, m, ns, seed=0):
    rng = np.random.default_rng(seed)
    k = ns // 2
    return np.concatenate([rng.choice(n, ns - k, replace=False), n + rng.choice(m, k, replace=False)])[rng.permutation(ns)]


def _set_schur_rc(s, idx):
    p = L.i64(np.asarray(idx, dtype=np.int64))
    return s._lib.okkt_set_schur(s._h, len(p), L.p_i64(p) if len(p) else None)


def test_set_schur_refuses_malformed_sets():
    K, n, m = _kkt()
    s = _handle()
    s.analyze(K)
    dim = n + m
    assert _set_schur_rc(s, [3, 5, 3]) == L.OKKT_ERR_INVALID
    assert "duplicate" in s._lib.okkt_last_error(s._h).decode()
    assert _set_schur_rc(s, [1, -2]) == L.OKKT_ERR_INVALID
    assert _set_schur_rc(s, [0, dim]) == L.OKKT_ERR_INVALID
    assert _set_schur_rc(s, np.arange(dim)) == L.OKKT_ERR_INVALID
    assert s._lib.okkt_set_schur(s._h, -1, None) == L.OKKT_ERR_INVALID
    # none of the refused calls changed the plan: the handle is still analysed without a set
    assert s.perm().shape == (dim,)
    finalize_b(s)
    # before any analysis the order is unknown: okkt_analyze refuses an out-of-range set or one that leaves no interior
    for bad in ([0, dim + 4], np.arange(dim)):
        s = _handle()
        s.set_schur(bad)
        with pytest.raises(OkktError, match="Schur set"):
            s.analyze(K)
        finalize_b(s)


@pytest.mark.parametrize("ordering", [0, 1, 3, 5])
@pytest.mark.parametrize("ns", [1, 17, 129])
def test_schur_set_is_the_last_supernode(ordering, ns):
    K, n, m = _kkt()
    dim = n + m
    idx = _mixed_set(n, m, ns, seed=ns)
    s = _handle(ordering=ordering)
    s.set_schur(idx)
    s.analyze(K)
    perm = s.perm()
    assert sorted(perm.tolist()) == list(range(dim))
    np.testing.assert_array_equal(perm[dim - ns:], idx)
    parent, cnt = s.etree()
    n1 = dim - ns
    # the set is a dense chain: column n1 + t has the parent n1 + t + 1 and ns - t entries
    np.testing.assert_array_equal(parent[n1:], np.append(np.arange(n1 + 1, dim), -1))
    np.testing.assert_array_equal(cnt[n1:], ns - np.arange(ns))
    # ... and no interior column belongs to its supernode: the last interior column is not a fundamental-supernode
    # predecessor of the set, and the front of the last supernode has exactly ns rows
    st = s.stats()
    assert st["max_front"] >= ns
    interior_parents = parent[:n1]
    assert np.all(interior_parents < dim) and np.all((interior_parents == -1) | (interior_parents > np.arange(n1)))
    finalize_b(s)


def test_interior_order_comes_from_a11():
    """The interior is ordered on the pattern of A11: the interior part of the permutation, read as an order of A11, gives A11
    the fill of the plan that A11 gets on its own (the whole-matrix postorder may permute it, which changes no fill)."""
    K, n, m = _kkt()
    dim = n + m
    idx = _mixed_set(n, m, 40, seed=1)
    inner = np.setdiff1d(np.arange(dim), idx)
    A11 = K[inner][:, inner].tocsc()
    for ordering in (3, 5):
        a = _handle(ordering=ordering)
        a.set_schur(idx)
        a.analyze(K)
        loc = np.full(dim, -1)
        loc[inner] = np.arange(dim - 40)
        b = _handle(ordering=ordering)
        b.analyze(A11)
        c = _handle(ordering=2)
        c.set_perm(loc[a.perm()[: dim - 40]])
        c.analyze(A11)
        assert c.stats()["nnzL"] == b.stats()["nnzL"]
        for h in (a, b, c):
            finalize_b(h)


def test_user_permutation_must_end_with_the_set():
    K, n, m = _kkt()
    dim = n + m
    idx = _mixed_set(n, m, 9, seed=2)
    inner = np.setdiff1d(np.arange(dim), idx)
    s = _handle(ordering=2)
    s.set_schur(idx)
    s.set_perm(np.concatenate([inner, idx[::-1]]))
    with pytest.raises(OkktError, match="must end with the Schur set"):
        s.analyze(K)
    s.set_perm(np.concatenate([inner[::-1], idx]))
    s.analyze(K)
    np.testing.assert_array_equal(s.perm()[dim - 9:], idx)
    finalize_b(s)


def test_cleared_set_is_no_set():
    K, n, m = _kkt()
    fresh = _handle()
    fresh.analyze(K)
    s = _handle()
    s.set_schur(_mixed_set(n, m, 30))
    s.analyze(K)
    s.set_schur([])
    s.analyze(K)
    np.testing.assert_array_equal(s.perm(), fresh.perm())
    p1, c1 = s.etree()
    p0, c0 = fresh.etree()
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(c1, c0)
    a, b = s.stats(), fresh.stats()
    for key in ("nnzL", "nnzL_stored", "flops_exact", "nsuper", "nlevels", "max_front", "ordering_used"):
        assert a[key] == b[key], key
    finalize_b(s)
    finalize_b(fresh)


def test_schur_calls_refused_without_a_set():
    K, n, m = _kkt()
    s = _handle()
    s.analyze(K)
    vals = np.asarray(K.data, dtype=np.float64)
    inert = L.OkktInertia()
    for rc in (
        s._lib.okkt_factor_schur(s._h, L.p_f64(vals), n, m, L.OKKT_SYM_SYMMETRIC, inert),
        s._lib.okkt_get_schur(s._h, L.p_f64(np.zeros(4)), 2),
        s._lib.okkt_schur_condense(s._h, L.p_f64(np.zeros(n + m)), L.p_f64(np.zeros(4)), 1),
        s._lib.okkt_schur_expand(s._h, L.p_f64(np.zeros(n + m)), L.p_f64(np.zeros(4)), L.p_f64(np.zeros(n + m)), 1),
    ):
        assert rc == L.OKKT_ERR_INVALID
        assert "not in Schur mode" in s._lib.okkt_last_error(s._h).decode()
    finalize_b(s)


def test_whole_matrix_calls_refused_in_schur_mode():
    K, n, m = _kkt()
    s = _handle()
    s.set_schur([0, n])
    s.analyze(K)
    vals = np.asarray(K.data, dtype=np.float64)
    x = np.zeros(n + m)
    for rc in (
        s._lib.okkt_factor(s._h, L.p_f64(vals), n, m, L.OKKT_SYM_SYMMETRIC, None),
        s._lib.okkt_solve(s._h, L.p_f64(x), L.p_f64(x), 1),
        s._lib.okkt_condest(s._h, L.p_f64(vals), 2, None),
        s._lib.okkt_dist_set_partition(s._h, 2, 0),
    ):
        assert rc == L.OKKT_ERR_INVALID
        assert "Schur mode" in s._lib.okkt_last_error(s._h).decode()
    # the handle stays usable: the plan is still there
    assert s.perm()[-2:].tolist() == [0, n]
    finalize_b(s)
