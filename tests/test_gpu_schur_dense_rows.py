"""Dense rows of J kept out of the Schur complement (okkt_opts.schur_dense_rows): the Schur kinds factor the bordered matrix
A = [[H + J_s' S_s J_s + delta I, J_d'], [J_d, -diag(s_d / y_d)]] instead of Q = H + J' S J + delta I.  Its Schur complement of the
(2,2) block is Q, so directions, inertia flags and the delta loop must be those of the plain Schur system -- checked against the
oracle's dense Q, against the same handle with the option off and against the symmetric kind."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd import kkt_system_solver as KS
from oracle import kkt_oracle as KO

pytestmark = pytest.mark.gpu


def with_dense_rows(prob, k, seed=0, lo=0.6, hi=1.0):
    """prob with k rows appended to J, each over a random 60 - 100 % of the columns (s, y extended; synth.CONFIGS untouched)."""
    rng = np.random.default_rng(seed + 500)
    n, m = prob["n"], prob["m"]
    rows, cols, vals = [], [], []
    for r in range(k):
        c = np.sort(rng.choice(n, size=int(rng.uniform(lo, hi) * n), replace=False))
        rows.append(np.full(len(c), r)); cols.append(c); vals.append(rng.normal(size=len(c)) / np.sqrt(len(c)))
    Jd = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(k, n)) if k else sp.csc_matrix((0, n))
    J = sp.vstack([prob["J"], Jd], format="csc")
    J.sort_indices()
    out = dict(prob)
    out.update(J=J, m=m + k, s=np.concatenate([prob["s"], np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=k))]),
               y=np.concatenate([prob["y"], np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=k))]))
    return out


def synth_iterate(prob, Iterate, seed=0):
    rng = np.random.default_rng(seed)
    n, m = prob["n"], prob["m"]
    return Iterate(x=rng.normal(size=n), y=prob["y"].copy(), s=prob["s"].copy(), mu=prob["mu"], J=prob["J"], H=prob["H"],
                   grad=rng.normal(size=n), cons=prob["s"] + 0.1 * rng.normal(size=m), a_norm_penalty_par=1e-4)


def moved(cls, base, seed):
    """A current iterate different from the factor iterate (new s, y, Jacobian values, gradient): one_phase.jl:262-279."""
    rng = np.random.default_rng(seed + 100)
    J2 = base.J.copy(); J2.data = J2.data * (1.0 + 0.05 * rng.normal(size=J2.nnz))
    return cls(x=base.x + 0.01, y=base.y * rng.uniform(0.7, 1.4, size=len(base.y)), s=base.s * rng.uniform(0.7, 1.4, size=len(base.s)),
               mu=0.5 * base.mu, J=J2, H=base.H, grad=base.grad + 0.1 * rng.normal(size=len(base.x)), cons=base.cons + 0.01,
               a_norm_penalty_par=base.a_norm_penalty_par)


def solver(kind, it, delta=None, **opts):
    k = KS.HIP_KKT_solver(kind, **opts)
    k.initialize_b(it)
    k.form_system_b(it)
    flag = k.factor_b(delta) if delta is not None else None
    return k, flag


def rel(a, b):
    return np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))) if len(b) else 0.0


@pytest.mark.parametrize("kd", [1, 3, 8])
def test_border_exists(kd):
    prob = with_dense_rows(synth.make_config("S-small", seed=1, well_scaled=True), kd, seed=kd)
    n, m = prob["n"], prob["m"]
    it = synth_iterate(prob, KS.Class_iterate, 1)
    k, flag = solver("schur", it, 1e-6, schur_dense_rows=-1)
    assert list(k.dense_rows()) == list(range(m - kd, m))
    A = k.matrix()
    assert A.shape == (n + kd, n + kd)
    Js, Jd = prob["J"][: m - kd], prob["J"][m - kd:]
    sig = prob["y"] / prob["s"]
    Qs = sp.tril(Js.T @ sp.diags(sig[: m - kd]) @ Js + prob["H"]).tocsc()
    pat = sp.tril(abs(Js).T @ abs(Js) + abs(prob["H"]) + sp.identity(n)).tocsc()
    assert A.nnz <= pat.nnz + Jd.nnz + kd
    # the blocks: Q_s, J_d below it, -s_d / y_d on the border diagonal
    Ad = A.toarray()
    assert np.max(np.abs(Ad[:n, :n] - Qs.toarray())) <= 1e-12 * max(1.0, abs(Qs).max())
    assert np.array_equal(Ad[n:, :n], Jd.toarray())
    assert np.array_equal(np.diag(Ad[n:, n:]), -prob["s"][m - kd:] / prob["y"][m - kd:])
    assert flag == 1 and k.inertia[:3] == (n, kd, 0)
    # schur_diag keeps describing diag(Q) of the whole Q
    Q = prob["J"].T @ sp.diags(sig) @ prob["J"] + prob["H"]
    assert np.allclose(k.schur_diag, Q.diagonal(), rtol=1e-13)
    k.finalize_b()


@pytest.mark.parametrize("kind", ["schur", "schur_direct"])
@pytest.mark.parametrize("seed,kd", [(2, 1), (3, 4)])
def test_directions_against_the_oracle(kind, seed, kd):
    prob = with_dense_rows(synth.make_config("S-small", seed=seed, well_scaled=True), kd, seed=seed)
    results = {}
    for dro in (0, -1):
        it = synth_iterate(prob, KS.Class_iterate, seed)
        k, flag = solver(kind, it, 1e-6, schur_dense_rows=dro)
        assert len(k.dense_rows()) == (kd if dro else 0)
        k.kkt_associate_rhs_b(moved(KS.Class_iterate, it, seed), KS.Reduct_stable())
        k.compute_direction_b()
        results[dro] = (flag, k.dir.x.copy(), k.dir.y.copy(), k.dir.s.copy(), k.kkt_err_norm.ratio)
        k.finalize_b()
    oit = synth_iterate(prob, KO.Iterate, seed)
    ko = KO.pick_KKT_solver(kind)
    ko.initialize_b(oit); ko.form_system_b(oit)
    oflag = ko.factor_b(1e-6)
    ko.kkt_associate_rhs_b(moved(KO.Iterate, oit, seed), KO.Reduct_stable())
    ko.compute_direction_b()
    flag, dx, dy, ds, ratio = results[-1]
    assert flag == oflag == 1
    for got, ref in ((dx, ko.dir.x), (dy, ko.dir.y), (ds, ko.dir.s)):
        assert rel(got, ref) <= 1e-8
    assert ratio <= 10.0 * results[0][4] + 1e-15


@pytest.mark.parametrize("seed", [5, 6])
def test_delta_loop_matches_the_oracle(seed):
    prob = with_dense_rows(synth.make_config("S-small", seed=seed, convex=False, well_scaled=True), 3, seed=seed)
    n = prob["n"]
    it = synth_iterate(prob, KS.Class_iterate, seed)
    k, _ = solver("schur", it, schur_dense_rows=-1)
    assert len(k.dense_rows()) == 3
    k0, _ = solver("schur", synth_iterate(prob, KS.Class_iterate, seed))
    oit = synth_iterate(prob, KO.Iterate, seed)
    ko = KO.pick_KKT_solver("schur")
    ko.initialize_b(oit); ko.form_system_b(oit)
    assert abs(k.diag_min() - ko.diag_min()) <= 1e-12 * abs(ko.diag_min())
    for delta in (0.0, 1e-3, 10.0, 1e6):
        k.factor_b(delta); ko.factor_b(delta)
        assert k.is_diag_dom() == KO.is_diag_dom(sp.csc_matrix(ko.Q)[:n, :n]), delta
    status, num_fac, delta = k.ipopt_strategy_b(it)
    so, nfo, do, _ = KO.ipopt_strategy_b(oit, ko)
    assert (status, num_fac) == (so, nfo) and num_fac >= 1
    assert abs(delta - do) <= 1e-12 * abs(do)
    s0, nf0, d0 = k0.ipopt_strategy_b(synth_iterate(prob, KS.Class_iterate, seed))
    assert (s0, nf0) == (status, num_fac) and abs(d0 - delta) <= 1e-12 * abs(d0)
    assert k.diag_dom_warnings == k0.diag_dom_warnings
    k.finalize_b(); k0.finalize_b()


@pytest.mark.parametrize("kind", ["schur", "schur_direct"])
def test_batched_directions_equal_the_one_by_one_ones(kind):
    prob = with_dense_rows(synth.make_config("S-small", seed=4, well_scaled=True), 3, seed=4)
    it = synth_iterate(prob, KS.Class_iterate, 4)
    etas = [KS.Reduct_affine(), KS.Class_reduction_factors(0.3, 0.3, 0.3), KS.Reduct_stable(), KS.Class_reduction_factors(0.2, 0.0, 0.2),
            KS.Class_reduction_factors(0.05, 0.0, 0.05)]
    k, flag = solver(kind, it, 1e-6, schur_dense_rows=-1)
    assert flag == 1 and len(k.dense_rows()) == 3
    cur = moved(KS.Class_iterate, it, 4)
    for q in (3, 5):
        k.kkt_associate_rhs_b(cur, etas[0])
        batch = k.compute_directions_b(etas[:q])
        for eta, (d, kerr) in zip(etas[:q], batch):
            k.kkt_associate_rhs_b(cur, eta); k.compute_direction_b()
            for a in ("x", "y", "s"):
                assert rel(getattr(d, a), getattr(k.dir, a)) <= 1e-12, (q, a)
            assert abs(kerr.ratio - k.kkt_err_norm.ratio) <= 1e-6 * k.kkt_err_norm.ratio + 1e-15
    k.finalize_b()


def test_option_on_without_a_dense_row_is_bitwise_the_option_off():
    prob = synth.make_config("S-C3", seed=0, well_scaled=True)
    out = {}
    for dro in (0, -1):
        it = synth_iterate(prob, KS.Class_iterate, 0)
        k, flag = solver("schur", it, 1e-6, schur_dense_rows=dro)
        assert len(k.dense_rows()) == 0
        k.kkt_associate_rhs_b(it, KS.Reduct_affine())
        k.compute_direction_b()
        out[dro] = (k.matrix(), flag, k.inertia, k.dir.x.copy(), k.dir.y.copy(), k.dir.s.copy())
        k.finalize_b()
    a, b = out[0], out[-1]
    assert a[0].shape == b[0].shape and np.array_equal(a[0].indptr, b[0].indptr) and np.array_equal(a[0].indices, b[0].indices)
    assert np.array_equal(a[0].data, b[0].data)
    assert a[1] == b[1] == 1 and a[2] == b[2]
    for u, v in zip(a[3:], b[3:]):
        assert np.array_equal(u, v)


def test_hanging_chain():
    prob = synth.hanging_chain()
    n, m = prob["n"], prob["m"]
    runs = {}
    for dro in (0, -1):
        it = synth_iterate(prob, KS.Class_iterate, 0)
        k, _ = solver("schur", it, schur_dense_rows=dro)
        status, num_fac, delta = k.ipopt_strategy_b(it)
        k.kkt_associate_rhs_b(it, KS.Reduct_affine())
        k.compute_direction_b()
        runs[dro] = (list(k.dense_rows()), (status, num_fac, delta), k.dir.x.copy(), k.dir.y.copy(), k.dir.s.copy())
        k.finalize_b()
    N = (n - 2) // 2
    assert runs[-1][0] == [N, 2 * N + 3]        # the two length rows (+c and -c), dense in u
    assert runs[0][0] == []
    assert runs[-1][1][:2] == runs[0][1][:2] and abs(runs[-1][1][2] - runs[0][1][2]) <= 1e-12 * abs(runs[0][1][2])
    oit = synth_iterate(prob, KO.Iterate, 0)
    ko = KO.pick_KKT_solver("schur")
    ko.initialize_b(oit); ko.form_system_b(oit)
    so, nfo, do, _ = KO.ipopt_strategy_b(oit, ko)
    assert (so, nfo) == runs[-1][1][:2] and abs(do - runs[-1][1][2]) <= 1e-12 * abs(do)
    ko.kkt_associate_rhs_b(oit, KO.Reduct_affine()); ko.compute_direction_b()
    for i, ref in zip((2, 3, 4), (ko.dir.x, ko.dir.y, ko.dir.s)):
        assert rel(runs[-1][i], runs[0][i]) <= 1e-8
        assert rel(runs[-1][i], ref) <= 1e-8


def test_every_row_dense_equals_the_symmetric_kind():
    prob = synth.make_config("S-small", seed=8, well_scaled=True)
    it = synth_iterate(prob, KS.Class_iterate, 8)
    k, flag = solver("schur", it, 1e-6, schur_dense_rows=1)
    longer = np.flatnonzero(np.diff(prob["J"].tocsr().indptr) > 1)   # every row with more than one entry: all but a handful
    assert list(k.dense_rows()) == list(longer) and len(longer) >= prob["m"] - 5
    ky, flagy = solver("symmetric", it, 1e-6)
    assert flag == flagy == 1
    assert k.inertia[:3] == (prob["n"], len(longer), 0) and ky.inertia[:3] == (prob["n"], prob["m"], 0)
    for kk in (k, ky):
        kk.kkt_associate_rhs_b(it, KS.Reduct_affine()); kk.compute_direction_b()
    for a in ("x", "y", "s"):
        assert rel(getattr(k.dir, a), getattr(ky.dir, a)) <= 1e-9, a
    k.finalize_b(); ky.finalize_b()
    # the edges: m = 0 (nothing to border) and a threshold no row passes (k = 0)
    for p, dro in ((synth.make_problem(n=50, m=0, seed=1, well_scaled=True), 1), (synth.make_config("S-tiny", seed=1, well_scaled=True), 10_000)):
        it = synth_iterate(p, KS.Class_iterate, 1)
        k, flag = solver("schur", it, 1e-6, schur_dense_rows=dro)
        k0, flag0 = solver("schur", synth_iterate(p, KS.Class_iterate, 1), 1e-6)
        assert len(k.dense_rows()) == 0 and flag == flag0 == 1
        for kk in (k, k0):
            kk.kkt_associate_rhs_b(it, KS.Reduct_affine()); kk.compute_direction_b()
        assert np.array_equal(k.dir.x, k0.dir.x) and np.array_equal(k.dir.y, k0.dir.y)
        k.finalize_b(); k0.finalize_b()


def test_estimate_y_tilde_and_ls_solve():
    prob = with_dense_rows(synth.make_problem(n=300, m=420, seed=3, well_scaled=True), 4, seed=3)
    n = prob["n"]
    g = np.random.default_rng(3).normal(size=n)
    y_hip = KS.estimate_y_tilde(prob["J"], g, schur_dense_rows=-1)
    y_ref = KO.estimate_y_tilde(prob["J"], g)
    assert rel(y_hip, y_ref) <= 1e-9
    it = synth_iterate(prob, KS.Class_iterate, 3)
    k, flag = solver("schur", it, 1e-6, schur_dense_rows=-1)
    assert flag == 1 and len(k.dense_rows()) == 4
    oit = synth_iterate(prob, KO.Iterate, 3)
    ko = KO.pick_KKT_solver("schur")
    ko.initialize_b(oit); ko.form_system_b(oit); ko.factor_b(1e-6)
    Q = sp.csc_matrix(ko.Q)
    Qd = (sp.tril(Q) + sp.tril(Q, -1).T).toarray()                # H is lower-stored: the symmetric Q it stands for
    r = np.random.default_rng(4).normal(size=n)
    x = k.ls_solve(r)
    assert x.shape == (n,)
    assert rel(x, np.linalg.solve(Qd, r)) <= 1e-9
    k.finalize_b()


def test_metric_size_with_four_dense_rows():
    # before any large allocation: the library and its binding know the option
    assert hasattr(L.load(), "okkt_kkt_get_dense_rows")
    assert "schur_dense_rows" in [f for f, _ in L.OkktOpts._fields_]
    base = synth.make_config("S-metric", seed=0, well_scaled=True)
    n = base["n"]
    prob = with_dense_rows(base, 4, seed=9, lo=1.0, hi=1.0)          # four rows of n = 40 000 entries
    k0, _ = solver("schur", synth_iterate(base, KS.Class_iterate, 0))
    nnz_q, arena_q = k0.matrix().nnz, k0.linear_solver_stats()["arena_bytes"]
    k0.finalize_b()
    it = synth_iterate(prob, KS.Class_iterate, 0)
    k, flag = solver("schur", it, 1e-6, schur_dense_rows=-1)
    assert len(k.dense_rows()) == 4
    A = k.matrix()
    assert A.nnz <= 1.05 * nnz_q + 4 * n + 4
    assert k.linear_solver_stats()["arena_bytes"] <= 1.2 * arena_q
    ky, flagy = solver("symmetric", it, 1e-6)
    assert flag == flagy == 1
    for kk in (k, ky):
        kk.kkt_associate_rhs_b(it, KS.Reduct_affine()); kk.compute_direction_b()
    for a in ("x", "y", "s"):
        assert rel(getattr(k.dir, a), getattr(ky.dir, a)) <= 1e-8, a
    k.finalize_b(); ky.finalize_b()


def test_invalid_option_value_is_refused():
    lib = L.load()
    o = L.OkktOpts()
    lib.okkt_default_opts(C.byref(o))
    h = C.c_void_p()
    o.schur_dense_rows = -2
    for kind in (L.OKKT_KKT_SCHUR, L.OKKT_KKT_SCHUR_DIRECT):
        assert lib.okkt_kkt_create(C.byref(h), C.byref(o), kind) == L.OKKT_ERR_INVALID
    assert lib.okkt_kkt_create(C.byref(h), C.byref(o), L.OKKT_KKT_SYMMETRIC) == L.OKKT_OK      # the other kinds ignore it
    lib.okkt_kkt_destroy(h)
