"""okkt_eigs on the GPU: the eigenpairs of the factored matrix nearest zero by block shift-invert Krylov-Schur,
against numpy.linalg.eigh of the dense matrix on the designs of eigs_ref.py, which sit around the constants of the new kernels.

What is asserted, per returned pair (lambda, v), v of full length with unit leading part:
  rho <= 4 tol |lambda| + floor, where rho is recomputed here in long double from the dense matrix: ||F v - lambda v||_2 / ||v||_2, in
    pencil mode ||S x - lambda x||_2 / ||x||_2 on the dense Schur complement S = F11 - F12 F22^-1 F21 and the leading part x.  The
    library never supplies the tolerance.  floor = 64 * 2^-52 || |F| |v| ||_2 (pencil mode: with |F11| + |F12| |F22^-1| |F21| and |x|):
    v comes out of one solve pass, whose componentwise backward error on these quasi-definite and diagonally dominant designs is a few
    units of 2^-52 (the refinement tests find omega_0 there); the double-double residual pass itself adds one rounding.
  |lambda - lambda_true| <= rho + n 2^-52 ||S||_2: the symmetric residual bound plus eigh's own error (S = F in standard mode), the
    returned values matched one to one against the nev true ones of smallest modulus.
  The library's resid against the long-double ||lambda B v - F v||_2 of the same v, to the same floor.
  Unit leading part, sign rule, V'V = I to 2^-40 on the leading parts, and for an eigenvalue at distance g from the rest of the spectrum
    the sine of the angle to eigh's vector <= (rho + n 2^-52 ||S||_2) / g (Davis and Kahan; the second term is eigh's vector error).
Every case runs with max_restarts = 20 and must end with status 0 or 2; test_eigs_host.py shows the reference needs at most 10.

Not covered: a fresh block after an invariant subspace (info.fresh_blocks > 0).  It needs a caller-supplied start block inside an
invariant subspace, and okkt_eigs has no such option: a hashed block has a component in every direction."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import eigs_ref as R
import lanczos_ref as LR
from conftest import iterate_from_record
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
FLOOR_C = 64
RESTARTS = 20


def factored(c, **opts):
    h = linear_solver_HIP("symmetric", **opts)
    initialize_b(h)
    h.ls_factor_b(c.A, c.npos, c.dim - c.npos)
    return h


def run(h, c, with_values=True, **over):
    kw = dict(c.opts(), max_restarts=RESTARTS)
    kw.update(over)
    return h.eigs(c.nev, c.A if with_values else None, **kw)


@functools.lru_cache(maxsize=None)
def dense_ld(cid):
    """(F, |F|, S, |S| bound) in long double; S by direct division, the (2,2) block of the pencil designs being diagonal."""
    c = R.cases()[cid]
    F = c.F.astype(LD)
    if not c.pencil:
        return F, np.abs(c.F), F, np.abs(c.F)
    k = c.nlead
    d = np.diag(c.F[k:, k:])
    assert np.array_equal(c.F[k:, k:], np.diag(d)) and np.all(d != 0.0)
    F12 = F[:k, k:]
    S = F[:k, :k] - (F12 / d.astype(LD)) @ F12.T
    Sabs = np.abs(c.F[:k, :k]) + (np.abs(c.F[:k, k:]) / np.abs(d)) @ np.abs(c.F[:k, k:]).T
    return F, np.abs(c.F), S, Sabs


def check_pairs(c, lam, V, resid, info):
    n, nev = c.n, c.nev
    F, Fabs, S, Sabs = dense_ld(c.id)
    assert info["status"] in (0, 2) and info["true_residuals"] == 1
    assert np.all(np.isfinite(lam)) and np.all(np.diff(np.abs(lam)) >= 0.0)
    X = V[:, :n]
    rho = np.zeros(nev)
    for j in range(nev):
        v, x = V[j].astype(LD), X[j].astype(LD)
        r = S @ x - LD(lam[j]) * x
        rho[j] = float(np.sqrt(r @ r) / np.sqrt(x @ x))
        floor = FLOOR_C * EPS * float(np.linalg.norm(Sabs @ np.abs(X[j])))
        print(f"{c.id} pair {j}: lambda={lam[j]:.12e} rho={rho[j]:.3e} 4 tol |lambda|={4 * c.tol * abs(lam[j]):.3e} floor={floor:.3e} resid={resid[j]:.3e}")
        assert rho[j] <= 4 * c.tol * abs(lam[j]) + floor
        # the library's residual: the same quantity for the full vector
        Bv = v.copy()
        Bv[n:] = 0
        rf = F @ v - LD(lam[j]) * Bv
        full = float(np.sqrt(rf @ rf))
        assert abs(resid[j] - full) <= FLOOR_C * EPS * float(np.linalg.norm(Fabs @ np.abs(V[j])))
        # unit leading part, sign rule
        assert abs(np.linalg.norm(X[j]) - 1.0) <= 8 * EPS
        assert X[j][np.argmax(np.abs(X[j]))] > 0.0
    # one to one against the nev true eigenvalues of smallest modulus
    eigh_err = n * EPS * c.snorm2
    got, want = np.argsort(lam), np.argsort(c.w[:nev])
    for a, b in zip(got, want):
        assert abs(lam[a] - c.w[b]) <= rho[a] + eigh_err, (c.id, a, b)
    assert np.linalg.norm(X @ X.T - np.eye(nev), 2) <= 2.0 ** -40
    # Davis-Kahan for the separated ones
    for a, b in zip(got, want):
        others = np.delete(c.w, b)
        g = np.min(np.abs(others - c.w[b])) if len(others) else np.inf
        if g <= 1e-6 * abs(c.w[b]):
            continue
        u = c.U[:, b]
        sine = np.linalg.norm(X[a] - u * (u @ X[a]))
        assert sine <= (rho[a] + eigh_err) / g + 8 * EPS, (c.id, a, sine, g)
    return rho


@pytest.mark.parametrize("cid", list(R.cases()))
def test_eigenpairs_against_eigh(cid):
    c = R.cases()[cid]
    h = factored(c)
    lam, V, resid, info = run(h, c)
    print(cid, info)
    check_pairs(c, lam, V, resid, info)
    assert info["basis"] == (c.max_basis or R.default_basis(c.n, c.nev, c.block)) and info["bytes"] > 0
    if info["dropped_columns"] == 0 and info["fresh_blocks"] == 0:
        assert info["solves"] == info["sweeps"] * c.block + (c.nev if c.pencil else 0)
    if c.n <= info["basis"]:
        assert info["status"] == 2                     # the basis spans the space before anything else stops the method
    if c.n < c.block:
        assert info["dropped_columns"] >= c.block - c.n and info["sweeps"] == 1
    if c.max_basis == 2 * c.nev + 3 * c.block:
        assert info["restarts"] >= 1
    if c.max_basis == 128:
        assert info["restarts"] == 0
    assert info["nconv"] == c.nev or info["status"] == 2
    # without the values: the same pairs, the Ritz residuals
    lam2, V2, resid2, info2 = run(h, c, with_values=False)
    assert info2["true_residuals"] == 0 and lam2.tobytes() == lam.tobytes() and V2.tobytes() == V.tobytes()
    assert np.all(resid2 <= c.tol) or info2["status"] == 2
    finalize_b(h)


def test_multiplicity_three_with_block_four():
    c = next(c for c in R.cases().values() if c.name == "repeated3x40")
    h = factored(c)
    lam, V, resid, info = run(h, c)
    check_pairs(c, lam, V, resid, info)
    floor = c.dim * EPS * c.norm2 + 4 * c.tol * np.max(np.abs(lam))
    assert np.max(np.abs(lam[:3] - c.w[0])) <= floor and np.max(np.abs(lam[3:] - c.w[3])) <= floor
    finalize_b(h)


def test_bits():
    """Two calls, the host and the device form, and a handle scaled by powers of two give the same bits."""
    for name, pencil in (("kkt257", False), ("pencil257", True)):
        c = next(c for c in R.cases().values() if c.name == name and c.block == 4 and c.max_basis == 0)
        h = factored(c)
        lam, V, resid, info = run(h, c)
        lam2, V2, resid2, info2 = run(h, c)
        assert (lam.tobytes(), V.tobytes(), resid.tobytes(), info) == (lam2.tobytes(), V2.tobytes(), resid2.tobytes(), info2)
        run(h, c, max_basis=128)                       # the workspace grows
        lam2, V2, resid2, info2 = run(h, c)
        info2["bytes"] = info["bytes"]
        assert (lam.tobytes(), V.tobytes(), resid.tobytes(), info) == (lam2.tobytes(), V2.tobytes(), resid2.tobytes(), info2)
        d_vals = h.dev_upload(c.A.data)
        d_vecs = h.dev_alloc(8 * c.dim * c.nev)
        lam3, resid3, info3 = h.eigs_dev(c.nev, d_vals, d_vecs, max_restarts=RESTARTS, **c.opts())
        V3 = h.dev_download(d_vecs, (c.nev, c.dim))
        info3["bytes"] = info["bytes"]
        assert (lam.tobytes(), V.tobytes(), resid.tobytes(), info) == (lam3.tobytes(), V3.tobytes(), resid3.tobytes(), info3)
        h.dev_free(d_vals)
        h.dev_free(d_vecs)
        finalize_b(h)
        s = 2.0 ** np.random.default_rng(3).integers(-6, 7, size=c.dim)
        hs = linear_solver_HIP("symmetric")
        initialize_b(hs)
        hs.analyze(c.A)
        hs.set_scaling("user", s=s)
        hs.ls_factor_b(c.A, c.npos, c.dim - c.npos)
        lam4, V4, resid4, info4 = run(hs, c)
        info4["bytes"] = info["bytes"]
        assert (lam.tobytes(), V.tobytes(), resid.tobytes(), info) == (lam4.tobytes(), V4.tobytes(), resid4.tobytes(), info4)
        finalize_b(hs)


def test_operator_identity():
    """nev = 1: okkt_solve(v) is v / lambda, to rho / lambda^2 (F^-1 of the residual) plus the solve's own backward error."""
    c = next(c for c in R.cases().values() if c.name == "kkt257" and c.nev == 1)
    h = factored(c)
    lam, V, resid, info = run(h, c)
    rho = check_pairs(c, lam, V, resid, info)
    y = h.ls_solve(V[0])
    bound = rho[0] / lam[0] ** 2 + FLOOR_C * EPS * np.linalg.norm(np.abs(c.F) @ np.abs(y)) / abs(lam[0])
    assert np.linalg.norm(y - V[0] / lam[0]) <= bound
    finalize_b(h)


# ---- the KKT level ---------------------------------------------------------------------------------------------------------------------
def kkt_factored(it, kind, delta, **opts):
    k = KS.HIP_KKT_solver(kind, **opts)
    k.initialize_b(it)
    k.form_system_b(it)
    k.factor_b(delta)
    return k


def q_rho(Q, lam, X):
    Ql = Q.astype(LD)
    out = []
    for j in range(len(lam)):
        x = X[j].astype(LD)
        r = Ql @ x - LD(lam[j]) * x
        out.append(float(np.sqrt(r @ r) / np.sqrt(x @ x)))
    return np.array(out)


@pytest.mark.parametrize("design", ["operator-full-37", "indefinite-37", "convex-37"])
def test_kkt_kinds_agree(design):
    if design == "operator-full-37":
        it, delta = LR.operator_design(KS.Class_iterate, 37, "full"), 0.0
    elif design == "indefinite-37":
        it, delta = LR.indefinite_design(KS.Class_iterate, 37, -3.7), 16.0
    else:
        it, delta = LR.convex_design(KS.Class_iterate, 37), 0.0
    Q = LR.dense_q(it) + delta * np.eye(it.dim())
    w = np.linalg.eigvalsh(Q)
    w = w[np.argsort(np.abs(w))]
    nev = next(k for k in (3, 2, 4, 1) if abs(w[k]) >= R.MIN_GAP * abs(w[k - 1]))
    qnorm = np.max(np.abs(w))
    got = {}
    for kind, opts in (("symmetric", {}), ("schur", {}), ("schur", {"schur_dense_rows": 20})):
        k = kkt_factored(it, kind, delta, **opts)
        lam, X, resid, info = k.eigs(nev, tol=1e-10)
        assert info["status"] in (0, 2) and X.shape == (nev, it.dim())
        rho = q_rho(Q, lam, X)
        print(design, kind, opts, info, lam, rho)
        for j in range(nev):
            assert abs(lam[j] - w[j]) <= rho[j] + it.dim() * EPS * qnorm
            assert abs(np.linalg.norm(X[j]) - 1.0) <= 8 * EPS and X[j][np.argmax(np.abs(X[j]))] > 0.0
        got[(kind, bool(opts))] = (lam, rho)
        # the same factor through its level-1 handle
        ls = linear_solver_HIP.of_kkt(k)
        lam1, _, _, info1 = ls.eigs(nev, tol=1e-10, nlead=it.dim() if ls._dim > it.dim() else 0)
        assert lam1.tobytes() == lam.tobytes()
        if design == "convex-37" and kind == "symmetric":
            einfo, _ = k.min_eig()
            assert lam[0] <= einfo["rho"] + einfo["rho_margin"]
        k.finalize_b()
    ls_, rs = got[("symmetric", False)]
    for key in (("schur", False), ("schur", True)):
        lc, rc = got[key]
        assert np.all(np.abs(ls_ - lc) <= rs + rc + 2 * it.dim() * EPS * qnorm)


def test_kkt_refusals(golden):
    it = LR.convex_design(KS.Class_iterate, 37)
    k = KS.HIP_KKT_solver("symmetric")
    k.initialize_b(it)
    k.form_system_b(it)
    with pytest.raises(OkktError, match="no complete factorisation"):
        k.eigs(2)
    assert k.factor_b(0.0) == 1
    with pytest.raises(OkktError, match="nev must be 1..32"):
        k.eigs(0)
    lam, X, resid, info = k.eigs(2)                     # the handle stays usable
    assert info["status"] in (0, 2)
    k.finalize_b()
    itc = iterate_from_record(golden["toy_lps"][0], KS.Class_iterate)
    kc = KS.HIP_KKT_solver("clever_symmetric")
    kc.initialize_b(itc)
    kc.form_system_b(itc)
    assert kc.factor_b(1e-8) == 1
    with pytest.raises(OkktError, match="clever-symmetric"):
        kc.eigs(1)
    assert kc.factor_b(1e-8) == 1
    kc.finalize_b()


# ---- refusals and status 3 -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = next(c for c in R.cases().values() if c.name == "kkt65" and not c.pencil)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(c.A)
    with pytest.raises(OkktError, match="before a complete factorisation"):
        h.eigs(1)
    h.ls_factor_b(c.A, c.npos, c.dim - c.npos)
    for kw, msg in ((dict(nev=0), "nev must be 1..32"), (dict(nev=33), "nev must be 1..32"), (dict(nev=4, nlead=3), "nev exceeds the order"),
                    (dict(nev=1, block=0), "block must be 1..4"), (dict(nev=1, block=5), "block must be 1..4"),
                    (dict(nev=6, max_basis=23), "max_basis must be"), (dict(nev=6, max_basis=129), "max_basis must be"),
                    (dict(nev=1, max_restarts=-1), "max_restarts < 0"), (dict(nev=1, tol=-1.0), "tol must be"),
                    (dict(nev=1, nlead=-1), "nlead must be"), (dict(nev=1, nlead=c.dim + 1), "nlead must be")):
        with pytest.raises(OkktError, match=msg):
            h.eigs(**kw)
    lam, V, resid, info = run(h, c)                    # the handle stays usable
    check_pairs(c, lam, V, resid, info)
    # max_restarts = 0 on a basis too small to converge in: status 1, the current Ritz pairs
    big = next(c for c in R.cases().values() if c.name == "kkt1029" and c.max_basis == 16)
    hb = factored(big)
    lam, V, resid, info = run(hb, big, max_restarts=0)
    assert info["status"] == 1 and info["restarts"] == 0 and 0 <= info["nconv"] < big.nev and np.all(np.isfinite(lam)) and np.all(np.isfinite(V))
    finalize_b(hb)
    finalize_b(h)
    # an early exit that stopped short
    prob = synth.make_config("S-small", seed=2, convex=False, neg_shift=50.0, well_scaled=True)
    n, m = prob["n"], prob["m"]
    K0 = synth.augmented_matrix(prob, delta=0.0)
    early = linear_solver_HIP("symmetric", early_exit=1)
    initialize_b(early)
    assert early.ls_factor_b(K0, n, m) == 0 and sum(early.inertia) < n + m
    with pytest.raises(OkktError, match="early exit"):
        early.eigs(1)
    finalize_b(early)
    # a partitioned handle, a handle in Schur mode
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.analyze(c.A)
    assert h._lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    with pytest.raises(OkktError, match="partitioned"):
        h.eigs(1)
    finalize_b(h)
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.set_schur([0, 1])
    h.analyze(c.A)
    with pytest.raises(OkktError, match="Schur mode"):
        h.eigs(1)
    finalize_b(h)


def test_zero_pivot_gives_status_3():
    Z = sp.csc_matrix(np.diag([1.0, 0.0, 2.0]))
    h = linear_solver_HIP("symmetric")
    initialize_b(h)
    h.ls_factor_b(Z, 3, 0)
    lam, V, resid, info = h.eigs(1, Z)
    assert info["status"] == 3 and info["sweeps"] == 1 and np.all(np.isnan(lam)) and np.all(np.isnan(resid)) and np.all(np.isnan(V))
    x = h.ls_solve(np.array([1.0, 0.0, 2.0]))          # the handle is as it was
    assert x[0] == 1.0 and x[2] == 1.0
    finalize_b(h)
