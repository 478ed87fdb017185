"""Host tests of the KKT-layer designs (tests/kkt_designs.py) and exact references (tests/kkt_exact.py): every design still lands
on the route and at the edge it exists for (the rules of csrc/kkt.hip restated in kkt_designs), together they cover every route,
the references accept a float evaluation of the same formulas and reject one that drops a term, and every term is far above the
rounding bound.  The binding brings a CSC with duplicates to canonical form."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_designs as KD
import kkt_exact as KE
from onephase_jl_amd import kkt_system_solver as KS

BANDS = (4, 8, 16, 32, 64)


@pytest.mark.parametrize("name", list(KD.DESIGNS))
def test_design_hits_its_route(name):
    d = KD.DESIGNS[name]
    r = KD.routes(d)
    assert d.expect and {k: r[k] for k in d.expect} == d.expect, (name, r)


def test_designs_cover_every_route_and_edge():
    R = {n: KD.routes(d) for n, d in KD.DESIGNS.items()}
    D = KD.DESIGNS
    assert {r["G"] for r in R.values()} == {16, 8, 4, 0}
    assert {512, 513, 1024, 1025, 2048, 2049} <= {r["maxcol"] for r in R.values()}
    # the list kernel as the only route of a J row longer than 2048 entries (dense rows off)
    assert any(R[n]["G"] == 0 and D[n].dense == 0 and np.diff(D[n].J.tocsr().indptr).max() > 2048 for n in D)
    # a border entry that moves the longest column over a boundary
    assert any(R[n]["kd"] and R[n]["maxcol"] == 513 and
               np.diff(KD.q_pattern(D[n].H, D[n].J, KD.dense_rows(D[n].J, D[n].dense))[0].indptr).max() == 512 for n in D)
    rows = {"lprJr": lambda d: d.m, "lprJc": lambda d: d.n, "lprH": lambda d: d.n}
    for fam, count in rows.items():
        for b in BANDS:
            hit = [n for n in D if R[n][fam] == b and count(D[n]) > 0]
            assert hit, (fam, b)
            # a launch whose last workgroup is partial
            assert any(count(D[n]) % (256 // b) for n in hit), (fam, b)
            # one partial workgroup only: rows below 256 / LPR (impossible for H at 16+ lanes: a lower-triangular column averages
            # at most (n + 1) / 2 entries)
            if not (fam == "lprH" and b >= 16):
                assert any(count(D[n]) < 256 // b for n in hit), (fam, b)
    assert any(d.n == 1 and d.m == 1 for d in D.values())
    assert any(d.m == 0 for d in D.values())
    assert any(d.H.nnz == 0 and d.n > 0 for d in D.values())
    assert any(d.n > 0 and (d.H.diagonal() == 0).all() and d.H.nnz > 0 for d in D.values())
    assert any((np.diff(d.J.tocsr().indptr) == 0).any() and (np.diff(d.J.tocsc().indptr) == 0).any() for d in D.values())
    for d in D.values():
        Jr = np.diff(d.J.tocsr().indptr)
        if d.m > 1 and Jr.max() >= 100 * np.mean(np.delete(Jr, np.argmax(Jr))) and d.dense == 0 and d.factor:
            break
    else:
        raise AssertionError("no design with a row 100 times longer than the others")


def _float_q(d, drows=()):
    keep = np.ones(d.m, bool)
    keep[list(drows)] = False
    Js = d.J.tocsr()[keep]
    return sp.tril(Js.T @ sp.diags(d.y[keep] / d.s[keep]) @ Js + d.H).tocsc()


@pytest.mark.parametrize("name", ["b4", "b16", "star513", "tiny32c", "border3"])
def test_q_reference_accepts_a_float_sum_and_rejects_a_dropped_term(name):
    d = KD.DESIGNS[name]
    drows = KD.dense_rows(d.J, d.dense)
    ex = KE.q_exact(d.H, d.J, d.y / d.s, drows)
    A = _float_q(d, drows)
    assert np.max(KE.q_ratios(A, ex, d.n)) <= 1.0
    # every term far above the bound: dropping any one of them cannot pass
    for e in ex.values():
        assert e[3] > 2.0 * KE.gamma(e[2] + 3) * e[1]
    Jr = d.J.tocsr()
    i = next(i for i in range(d.m) if i not in set(drows) and Jr.indptr[i + 1] > Jr.indptr[i])
    a = Jr.indices[Jr.indptr[i]]
    B = A.tolil()
    B[a, a] = B[a, a] - Jr.data[Jr.indptr[i]] ** 2 * (d.y[i] / d.s[i])
    assert np.max(KE.q_ratios(B.tocsc(), ex, d.n)) > 1.0


def test_single_term_reference_agrees_with_fractions():
    rng = np.random.default_rng(5)
    n = 90
    J = sp.csc_matrix((KD._vals(rng, 80), (np.zeros(80, int), np.arange(80))), shape=(1, n))
    H = KD._h(rng, n, 2)
    d = KD.Design("t", "", H, J, *KD._sy(rng, 1))
    A = _float_q(d)
    # the device pattern: the diagonal always present
    A = (A + sp.identity(n) * 0.0).tocsc()
    A.sort_indices()
    r1, r2 = KE.q_ratios_single_term(A, H, J, d.y / d.s), KE.q_ratios(A, KE.q_exact(H, J, d.y / d.s), n)
    assert np.max(r1) <= 1.0 and np.max(r2) <= 1.0
    A.data[7] = np.nextafter(A.data[7], 0) * (1 - 1e-12)
    assert np.max(KE.q_ratios_single_term(A, H, J, d.y / d.s)) > 1.0 and np.max(KE.q_ratios(A, KE.q_exact(H, J, d.y / d.s), n)) > 1.0


@pytest.mark.parametrize("name", ["b8", "b64", "jc64_tiny"])
def test_row_references_accept_float_and_reject_a_dropped_term(name):
    d = KD.DESIGNS[name]
    p = KD.point(d)
    J, s, y = d.J, d.s, d.y
    eta = (0.5, 0.25, 0.375)
    mu, pen = p["mu"], 1e-4
    rD = -((p["grad"] - J.T @ y) + ((mu * eta[2]) * pen) * (J.T @ np.ones(d.m))) * (1 - eta[1])
    rP = -(p["cons"] - s) * (1 - eta[0])
    rC = mu * eta[2] - s * y
    for r in KE.rhs_ratios(J, p["grad"], p["cons"], s, y, mu, pen, eta, rD, rP, rC):
        assert np.max(r) <= 1.0
    Jc = J.tocsc()
    j = int(np.argmax(np.diff(Jc.indptr)))
    bad = rD.copy()
    bad[j] += Jc.data[Jc.indptr[j]] * y[Jc.indices[Jc.indptr[j]]] * (1 - eta[1])
    assert np.max(KE.rhs_ratios(J, p["grad"], p["cons"], s, y, mu, pen, eta, bad, rP, rC)[0]) > 1.0
    dx = p["x"]
    sig = y / s
    dy = -(J @ dx - (rP + rC / y)) * sig
    for direct, ds in ((False, J @ dx - rP), (True, (rC - dy * s) / y)):
        for r in KE.dyds_ratios(J, dx, rP, rC, y, s, dy, ds, direct):
            assert np.max(r) <= 1.0
    i = int(np.argmax(np.diff(J.tocsr().indptr)))
    Jr = J.tocsr()
    bad = dy.copy()
    bad[i] += Jr.data[Jr.indptr[i]] * dx[Jr.indices[Jr.indptr[i]]] * sig[i]
    assert np.max(KE.dyds_ratios(J, dx, rP, rC, y, s, bad, J @ dx - rP, False)[0]) > 1.0
    # N err: the float evaluation of update_kkt_error! is within the bound of the exact maxima
    delta = KD.shift(d)
    ds = J @ dx - rP
    Hs = d.H + sp.tril(d.H, -1).T
    eD = np.abs(delta * dx + Hs @ dx - J.T @ dy - rD)
    eP, eM = np.abs(J @ dx - ds - rP), np.abs(s * dy + y * ds - rC)
    for got, e in zip((eD.max(), eP.max(), eM.max()), KE.kkt_error_exact(d.H, J, s, y, delta, dx, dy, ds, rD, rP, rC)):
        assert KE.max_ratio(got, e) <= 1.0


def test_binding_canonicalises_duplicates():
    A = sp.csc_matrix((np.array([1.0, 2.0, 4.0]), np.array([1, 1, 0]), np.array([0, 2, 3])), shape=(2, 2))
    assert A.has_sorted_indices is not None and not A.has_canonical_format
    B = KS._csc(A)
    assert B.has_canonical_format and B is not A
    assert np.array_equal(B.toarray(), np.array([[0.0, 4.0], [3.0, 0.0]]))
    assert np.array_equal(A.indices, [1, 1, 0])            # the caller's matrix is left alone
    assert KS._csc(B) is B
