"""The host side of okkt_eigs (no GPU needed): the dense symmetric eigen-solver (csrc/sym_eig.h, cyclic Jacobi)
through okkt_debug_sym_eig against numpy.linalg.eigh, the C ABI symbols, the argument refusals that stand in front of the device, and
the numpy restatement of the method (eigs_ref.py) on every design and option set the GPU tests run.

The eigen-solver's bound.  sym_eig.h derives it: a sweep is m - 1 sets of disjoint rotations, each a backward perturbation of at most
6 u ||G||_2 (u = 2^-53), i.e. 3 (m - 1) 2^-52 ||G||_2 per sweep; at most 20 sweeps; the entries left under the threshold add less than
2^-52 ||G||_2.  Hence |theta_j - true| <= 61 m 2^-52 ||G||_2 and ||S'S - I||_2 <= 61 m 2^-52; eigh's own error, m 2^-52 ||G||_2, is added
on the eigenvalue side: the constant asserted is 62.

The reference must converge (status 0, or 2 when the basis spans the space) within 10 restarts on every case; the GPU tests run the
same cases with max_restarts = 20, so the cap hides nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eigs_ref as R
from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("okkt_eigs", "okkt_eigs_dev", "okkt_kkt_eigs", "okkt_debug_sym_eig")
EPS = 2.0 ** -52
JACOBI_C = 62


def sym_eig(G):
    m = G.shape[0]
    a = L.f64(G)
    theta, S = np.zeros(m), np.zeros((m, m))
    rc = L.load().okkt_debug_sym_eig(m, L.p_f64(a), L.p_f64(theta), L.p_f64(S))
    return rc, theta, S


def test_symbols_and_structs():
    lib = L.load()
    txt = open(os.path.join(ROOT, "include", "okkt.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name + " is not declared in include/okkt.h"
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert [f for f, _ in L.OkktEigsOpts._fields_] == ["nev", "block", "max_basis", "max_restarts", "tol", "nlead", "seed"]
    assert C.sizeof(L.OkktEigsOpts) == 40
    assert [f for f, _ in L.OkktEigsInfo._fields_] == ["status", "nconv", "sweeps", "solves", "restarts", "basis", "fresh_blocks",
                                                       "dropped_columns", "true_residuals", "bytes"]
    assert C.sizeof(L.OkktEigsInfo) == 48


def check_sym_eig(G):
    m = G.shape[0]
    rc, theta, S = sym_eig(G)
    assert rc == 0
    w = np.linalg.eigvalsh(G)
    norm2 = max(abs(w[0]), abs(w[-1]))
    bound = JACOBI_C * m * EPS * norm2
    assert np.max(np.abs(np.sort(theta) - w)) <= bound
    assert np.linalg.norm(S.T @ S - np.eye(m), 2) <= JACOBI_C * m * EPS
    # the pairs belong together, and the order is |theta| descending, the positive one of equal moduli first
    assert np.linalg.norm(G @ S - S * theta, 2) <= 2 * bound + 1e-300
    key = [(-abs(t), -t) for t in theta]
    assert key == sorted(key)
    return theta, S


@pytest.mark.parametrize("m", [1, 2, 3, 17, 64, 127, 128])
def test_sym_eig_against_eigh(m):
    rng = np.random.default_rng(m)
    G = rng.normal(size=(m, m))
    check_sym_eig(0.5 * (G + G.T))
    # graded: entries over 1e-15 .. 1
    d = 10.0 ** rng.uniform(-7.5, 0.0, size=m)
    G = rng.normal(size=(m, m))
    check_sym_eig(0.5 * (G + G.T) * np.outer(d, d))
    # what a restart leaves: a diagonal and the coupling to one new block
    G = np.diag(10.0 ** rng.uniform(-6.0, 6.0, size=m) * rng.choice([-1.0, 1.0], size=m))
    q = min(4, m)
    G[:, m - q:] = rng.normal(size=(m, q))
    G[m - q:, :] = G[:, m - q:].T
    G[m - q:, m - q:] = 0.5 * (G[m - q:, m - q:] + G[m - q:, m - q:].T)
    check_sym_eig(G)


def test_sym_eig_repeated_zero_and_ties():
    Qm, _ = np.linalg.qr(np.random.default_rng(5).normal(size=(12, 12)))
    d = np.array([3.0, 3.0, 3.0, -3.0, 1.0, 1.0, 0.0, 0.0, -0.5, 0.5, 2.0, 2.0])
    G = (Qm * d) @ Qm.T
    theta, _ = check_sym_eig(0.5 * (G + G.T))
    assert np.max(np.abs(np.sort(theta) - np.sort(d))) <= JACOBI_C * 12 * EPS * 3.0
    for m in (1, 5, 128):
        rc, theta, S = sym_eig(np.zeros((m, m)))
        assert rc == 0 and np.all(theta == 0.0) and np.array_equal(S, np.eye(m))
    # exact ties of the modulus: the positive one first
    rc, theta, S = sym_eig(np.diag([-2.0, 2.0, 1.0, -1.0]))
    assert rc == 0 and theta.tolist() == [2.0, -2.0, 1.0, -1.0]
    # only the upper triangle is read
    G = np.array([[2.0, 1.0], [np.nan, 3.0]])
    rc, theta, _ = sym_eig(G)
    assert rc == 0 and np.allclose(np.sort(theta), np.linalg.eigvalsh(np.array([[2.0, 1.0], [1.0, 3.0]])))


def test_sym_eig_refusals():
    lib = L.load()
    for bad in (np.nan, np.inf, -np.inf):
        G = np.eye(4)
        G[1, 2] = bad
        theta, S = np.full(4, 7.0), np.full((4, 4), 7.0)
        assert lib.okkt_debug_sym_eig(4, L.p_f64(L.f64(G)), L.p_f64(theta), L.p_f64(S)) == L.OKKT_ERR_INVALID
        assert np.all(theta == 7.0) and np.all(S == 7.0)          # outputs untouched
    G = np.eye(129)
    theta, S = np.zeros(129), np.zeros((129, 129))
    assert lib.okkt_debug_sym_eig(129, L.p_f64(G), L.p_f64(theta), L.p_f64(S)) == L.OKKT_ERR_INVALID
    assert lib.okkt_debug_sym_eig(0, L.p_f64(G), L.p_f64(theta), L.p_f64(S)) == L.OKKT_ERR_INVALID
    assert lib.okkt_debug_sym_eig(4, None, L.p_f64(theta), L.p_f64(S)) == L.OKKT_ERR_INVALID


def test_hashed_start_block():
    """Odd multiples of 2^-53 strictly inside (-1, 1), a function of (seed, column, row) alone."""
    v = R.hashed_column(1, 0, 300)
    assert np.all(np.abs(v) < 1.0) and np.all((v * 2.0 ** 53) % 2 == 1)
    assert np.array_equal(v, R.hashed_column(1, 0, 300)) and np.array_equal(v[:100], R.hashed_column(1, 0, 100))
    assert not np.array_equal(v, R.hashed_column(1, 1, 300)) and not np.array_equal(v, R.hashed_column(2, 0, 300))
    assert abs(v.mean()) < 0.2 and 0.2 < v.std() < 0.8
    assert R.mix(0) == 0xE220A8397B1DCDAF                         # splitmix64's first output for the state 0


@pytest.mark.parametrize("cid", list(R.cases()))
def test_reference_converges_within_ten_restarts(cid):
    c = R.cases()[cid]
    lam, V, info = R.reference_eigs(c.F, c.nev, max_restarts=10, **c.opts())
    print(cid, info)
    assert info["status"] in (0, 2) and info["restarts"] <= 10
    want = c.w[: c.nev]
    # one to one against the nev true eigenvalues of smallest modulus
    assert np.max(np.abs(np.sort(lam) - np.sort(want))) <= 1e-6 * np.max(np.abs(want)) + 4 * c.dim * EPS * c.norm2
    assert np.all(np.diff(np.abs(lam)) >= -4 * c.dim * EPS * c.norm2)
    for j in range(c.nev):
        v = V[j]
        assert abs(np.linalg.norm(v[: c.n]) - 1.0) <= 8 * EPS and v[np.argmax(np.abs(v[: c.n]))] > 0.0
        Bv = np.concatenate([v[: c.n], np.zeros(c.dim - c.n)])
        assert np.linalg.norm(c.F @ v - lam[j] * Bv) <= 4 * c.tol * abs(lam[j]) + 64 * EPS * np.linalg.norm(np.abs(c.F) @ np.abs(v))


def test_designs_are_what_the_tests_need():
    cs = R.cases()
    ids = list(cs)
    assert {c.dim for c in cs.values()} >= set(R.SIZES)
    assert any(c.pencil and abs(np.linalg.det(c.F[c.nlead:, c.nlead:])) > 0 for c in cs.values())
    tiny = next(c for c in cs.values() if c.name == "tiny100")
    assert 1e-13 <= abs(tiny.w[0]) / tiny.norm2 <= 1e-11
    rep = next(c for c in cs.values() if c.name == "repeated3x40")
    w = rep.w
    floor = rep.dim * EPS * rep.norm2                              # eigh's own error
    assert abs(w[0] - w[2]) <= floor and abs(w[3] - w[5]) <= floor and abs(w[3]) > abs(w[0]) * 1.005
    assert all(c.gap >= R.MIN_GAP for c in cs.values()) and len(set(ids)) == len(ids)
    assert any(c.max_basis == 2 * c.nev + 3 * c.block for c in cs.values()) and any(c.max_basis == 128 for c in cs.values())


def test_argument_refusals_need_no_device():
    """On a host_symbolic_only handle every argument check answers before the device is asked for."""
    c = next(c for c in R.cases().values() if c.name == "kkt65" and not c.pencil)
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    with pytest.raises(OkktError, match="okkt_analyze has not been called"):
        h.eigs(1)
    h.analyze(c.A)
    for kw, msg in ((dict(nev=0), "nev must be 1..32"), (dict(nev=33), "nev must be 1..32"), (dict(nev=66), "nev must be 1..32"),
                    (dict(nev=4, nlead=3), "nev exceeds the order"), (dict(nev=1, block=0), "block must be 1..4"),
                    (dict(nev=1, block=5), "block must be 1..4"), (dict(nev=6, max_basis=23), "max_basis must be"),
                    (dict(nev=6, max_basis=129), "max_basis must be"), (dict(nev=1, max_restarts=-1), "max_restarts < 0"),
                    (dict(nev=1, tol=-1.0), "tol must be"), (dict(nev=1, tol=float("nan")), "tol must be"),
                    (dict(nev=1, nlead=-1), "nlead must be"), (dict(nev=1, nlead=c.dim + 1), "nlead must be")):
        with pytest.raises(OkktError, match=msg):
            h.eigs(**kw)
    o = h._eigs_opts(1, 4, 0, 20, 0.0, 0, 1)
    lam, res = np.zeros(1), np.zeros(1)
    assert h._lib.okkt_eigs(h._h, None, None, L.p_f64(lam), None, L.p_f64(res), None) == L.OKKT_ERR_INVALID
    assert h._lib.okkt_eigs(h._h, C.byref(o), None, None, None, L.p_f64(res), None) == L.OKKT_ERR_INVALID
    assert h._lib.okkt_eigs(None, C.byref(o), None, L.p_f64(lam), None, L.p_f64(res), None) == L.OKKT_ERR_INVALID
    # valid arguments: the device is what is missing
    assert h._lib.okkt_eigs(h._h, C.byref(o), None, L.p_f64(lam), None, L.p_f64(res), None) == L.OKKT_ERR_NO_DEVICE
    assert h._lib.okkt_eigs_dev(h._h, C.byref(o), None, L.p_f64(lam), None, L.p_f64(res), None) == L.OKKT_ERR_NO_DEVICE
    finalize_b(h)
