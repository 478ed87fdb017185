"""Host tests of the clever-symmetric designs (kkt_designs.CLEVER_DESIGNS) and of their exact references (kkt_exact.clever_*): the
oracle's compute_indicies finds exactly the designed groups, leaders and ratios; together the designs hold every edge the GPU tests
rely on; every reference accepts a plain float evaluation of the oracle's Clever_Symmetric_KKT_solver formulas and rejects the
mutations a subtly wrong kernel would make; every term is at least twice its bound, so a dropped one cannot hide."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_designs as KD
import kkt_exact as KE
from oracle import kkt_oracle as KO

CD = KD.CLEVER_DESIGNS
ETA = (0.5, 0.25, 0.375)


@pytest.mark.parametrize("name", list(CD))
def test_oracle_finds_the_designed_groups(name):
    d = CD[name]
    first, groups = KO.compute_indicies(d.J)
    assert first == [mem[0] for mem, _ in d.groups] and len(groups) == d.m_new
    assert [g.first for g in groups] == first
    assert [([r.ind for r in g.ls], [r.ratio for r in g.ls]) for g in groups] == d.groups      # members in ls order, ratios bitwise
    assert sorted(j for mem, _ in d.groups for j in mem) == list(range(d.m))                   # every row in exactly one group


def test_clever_designs_cover_every_edge():
    sizes = {len(mem) for d in CD.values() for mem, _ in d.groups}
    assert {1, 2, 3} <= sizes and max(sizes) >= 5
    ratios = {r for d in CD.values() for _, rat in d.groups for r in rat[1:]}
    pow2 = {r for r in ratios if math.frexp(abs(r))[0] == 0.5}
    assert any(r > 0 for r in pow2) and any(r < 0 for r in pow2) and any(abs(r) > 1 for r in pow2) and any(abs(r) < 1 for r in pow2)
    # members scattered through the row order, not appended: a group with a foreign row between two of its members
    assert any(max(mem) - min(mem) >= len(mem) for d in CD.values() for mem, _ in d.groups if len(mem) > 1)
    # a leader that is not the group's lowest row, from a ratio that is no power of two
    assert any(mem[0] > min(mem) and math.frexp(abs(rat[1]))[0] != 0.5 for d in CD.values() for mem, rat in d.groups if len(mem) == 2)

    def pairs_with_one_pattern(d):
        Jr = d.J.tocsr()
        Jr.sort_indices()
        lead = {j: mem[0] for mem, _ in d.groups for j in mem}
        by = {}
        for i in range(d.m):
            c = tuple(Jr.indices[Jr.indptr[i]:Jr.indptr[i + 1]])
            if c:
                by.setdefault(c, []).append(i)
        for rows in by.values():
            for a in rows:
                for b in rows:
                    if a < b and lead[a] != lead[b]:
                        va, vb = Jr.data[Jr.indptr[a]:Jr.indptr[a + 1]], Jr.data[Jr.indptr[b]:Jr.indptr[b + 1]]
                        yield float(np.max(np.abs(va / va[0] - vb / vb[0])))
    gaps = [g for d in CD.values() for g in pairs_with_one_pattern(d)]
    assert any(0 < g < 1e-11 for g in gaps), "no near-parallel pair that must not merge"
    assert any(g > 1e-2 for g in gaps), "no pair with one pattern and unrelated values"
    assert any((np.diff(d.J.tocsr().indptr) == 0).sum() >= 3 and (np.diff(d.J.tocsc().indptr) == 0).any() for d in CD.values())
    for d in CD.values():       # the empty rows form one group
        assert sum(1 for mem, _ in d.groups if d.J.tocsr().indptr[mem[0] + 1] == d.J.tocsr().indptr[mem[0]]) <= 1
    assert any(d.m_new < 256 < d.m for d in CD.values()) and any(d.m_new > 256 for d in CD.values())
    for d in CD.values():
        if d.m_new > 1:
            assert d.m_new % 256 and (d.n + d.m_new) % 256 and (d.H.nnz + d.J.nnz + d.m_new) % 256, d.name
    assert any(d.H.nnz > 0 and (d.H.diagonal() == 0).all() for d in CD.values())
    assert any(0 < np.count_nonzero(d.H.diagonal()) < d.n for d in CD.values())
    assert any(d.H.nnz == 0 and d.n > 0 and d.m > 0 for d in CD.values())
    assert any(d.m == 0 for d in CD.values())
    assert any(d.n == 1 and d.m == 2 and d.m_new == 1 for d in CD.values())
    assert sum(1 for n_ in ("b8", "b64", "jc64_tiny") if CD[n_].J is KD.DESIGNS[n_].J) >= 2
    assert all(max(len(mem) for mem, _ in CD[n_].groups if CD[n_].J.tocsr()[mem[0]].nnz) == 1 for n_ in ("b8", "b64", "jc64_tiny"))


# ---- a plain float evaluation of the oracle's formulas ---------------------------------------------------------------------------
def float_eval(d, rescale, seed=0):
    p = KD.point(d)
    it = KO.Iterate(x=p["x"], y=d.y, s=d.s, mu=p["mu"], J=d.J, H=d.H, grad=p["grad"], cons=p["cons"])
    ko = KO.Clever_Symmetric_KKT_solver(None, None, rescale)
    ko.initialize_b(it)
    ko.form_system_b(it)
    n = d.n
    u = d.s / d.y
    gU = np.array([g.u for g in ko.para_row_info])
    g = np.zeros(d.m)
    for grp in ko.para_row_info:
        for row in grp.ls:
            g[row.ind] = row.g
    D = ko.diag_rescale
    ptr, idx = KE.clever_pattern(d.H, d.J, ko.first_para_indicies)
    Q = sp.csc_matrix(ko.Q).todok()
    A = sp.csc_matrix((np.array([Q.get((int(i), j), 0.0) for j in range(len(ptr) - 1) for i in idx[ptr[j]:ptr[j + 1]]]), idx, ptr),
                      shape=(len(ptr) - 1,) * 2)
    assert A.nnz == sp.csc_matrix(ko.Q).nnz + int(np.sum(d.H.diagonal() == 0))
    A_true = A.copy()
    for j in range(n):
        A_true.data[A.indptr[j] + list(A.indices[A.indptr[j]:A.indptr[j + 1]]).index(j)] = d.H.diagonal()[j]
    J2, s2, y2 = KD.moved(d)
    cur = KO.Iterate(x=p["x"], y=y2, s=s2, mu=p["mu"], J=J2, H=d.H, grad=p["grad"], cons=p["cons"])
    rhs = KO.System_rhs.build(cur, KO.Class_reduction_factors(*ETA))
    rP, rC = rhs.primal_r, rhs.comp_r
    symrhs = rP + rC / d.y
    crhs = np.zeros(d.m_new)
    for i, grp in enumerate(ko.para_row_info):
        for row in grp.ls:
            crhs[i] += row.g * symrhs[row.ind]
    sol = KD._vals(np.random.default_rng(seed + 3000), n + d.m_new)
    xv = sol * D
    dx, v = xv[:n], xv[n:]
    dy = u ** (-1.0) * symrhs
    for i, grp in enumerate(ko.para_row_info):
        tmp = -(crhs[i] + grp.u * v[i])
        for row in grp.ls:
            dy[row.ind] += row.u ** (-1.0) * row.ratio * tmp
    ds = d.J @ dx - rP
    return dict(u=u, gU=gU, g=g, D=D, A=A, A_true=A_true, rP=rP, rC=rC, symrhs=symrhs, crhs=crhs, sol=sol, dx=dx, v=v, dy=dy, ds=ds,
                mu=p["mu"], xinf=float(np.max(np.abs(p["x"]))) if n else 0.0, first=ko.first_para_indicies)


def ok(r):
    return len(r) == 0 or float(np.max(r)) <= 1.0


@pytest.mark.parametrize("rescale", KD.RESCALES)
@pytest.mark.parametrize("name", list(CD))
def test_references_accept_the_float_evaluation(name, rescale):
    d = CD[name]
    e = float_eval(d, rescale)
    rU, rg = KE.clever_u_g_ratios(d.groups, e["u"], e["gU"], e["g"])
    assert ok(rU) and ok(rg)
    assert ok(KE.clever_d_ratios(rescale, e["mu"], e["xinf"], d.n, e["gU"], e["D"]))
    assert ok(KE.clever_q_ratios(e["A"], d.H, d.J, e["first"], e["gU"], e["D"], "scaled"))
    assert ok(KE.clever_q_ratios(e["A_true"], d.H, d.J, e["first"], e["gU"], e["D"], "true"))
    assert ok(KE.clever_symrhs_ratios(e["rP"], e["rC"], d.y, e["symrhs"]))
    assert ok(KE.clever_crhs_ratios(d.groups, e["g"], e["symrhs"], e["crhs"]))
    assert ok(KE.clever_unscale_ratios(e["sol"], e["D"], d.n, e["dx"], e["v"]))
    assert ok(KE.clever_dy_ratios(d.groups, e["u"], e["symrhs"], e["crhs"], e["gU"], e["v"], e["dy"]))
    assert ok(KE.ds_ratios(d.J, e["dx"], e["rP"], e["ds"]))
    # every term at least twice its bound
    for (mem, rat), U_ in zip(d.groups, e["gU"]):
        for j, r in zip(mem, rat):
            assert r * r / e["u"][j] > 2.0 * KE.gamma(len(mem) + 3) / U_
            assert abs(e["g"][j] * e["symrhs"][j]) > 2.0 * KE.gamma(len(mem)) * sum(abs(e["g"][t] * e["symrhs"][t]) for t in mem)
    for j, (t0, t1, ab) in KE.clever_dy_terms(d.groups, e["u"], e["symrhs"], e["crhs"], e["gU"], e["v"]).items():
        assert min(abs(t0), abs(t1)) > 2.0 * KE.gamma(6) * ab
    for i in range(d.m):
        assert min(abs(e["rP"][i]), abs(e["rC"][i] / d.y[i])) > 2.0 * KE.gamma(2) * (abs(e["rP"][i]) + abs(e["rC"][i] / d.y[i]))


def _big_group(d):
    """A group of at least three members whose last member's ratio is not 1 (a pair if the design has no larger group)."""
    c = [(g_, mem, rat) for g_, (mem, rat) in enumerate(d.groups) if len(mem) >= 2 and abs(rat[-1]) != 1.0]
    return max(c, key=lambda t: len(t[1]))


@pytest.mark.parametrize("name", ["cg_mix", "cg_big", "cg_h0"])
def test_references_reject_the_group_mutations(name):
    d = CD[name]
    e = float_eval(d, "u_only")
    u = e["u"]
    g_, mem, rat = _big_group(d)
    # a member dropped from U; the ratio not squared in U
    for bad_u in (1.0 / sum(r * r / u[j] for j, r in zip(mem[:-1], rat[:-1])), 1.0 / sum(abs(r) / u[j] for j, r in zip(mem, rat))):
        gU = e["gU"].copy(); gU[g_] = bad_u
        assert not ok(KE.clever_u_g_ratios(d.groups, u, gU, e["g"])[0])
    # the leader's ratio used for every member: in g, in dy
    g = e["g"].copy(); g[mem[-1]] = e["gU"][g_] * rat[0] / u[mem[-1]]
    assert not ok(KE.clever_u_g_ratios(d.groups, u, e["gU"], g)[1])
    dy = e["dy"].copy()
    j = mem[-1]
    dy[j] = e["symrhs"][j] / u[j] + (rat[0] / u[j]) * -(e["crhs"][g_] + e["gU"][g_] * e["v"][g_])
    assert not ok(KE.clever_dy_ratios(d.groups, u, e["symrhs"], e["crhs"], e["gU"], e["v"], dy))
    # rC not divided by y
    assert not ok(KE.clever_symrhs_ratios(e["rP"], e["rC"], d.y, e["rP"] + e["rC"]))
    # D_i^2 instead of D_i D_j on an off-diagonal entry (a leader's J entry: D_j = 1, D_i = mu / sqrt(U))
    A = e["A"].copy()
    p = next(p for j in range(d.n) for p in range(A.indptr[j], A.indptr[j + 1]) if A.indices[p] >= d.n)
    i = A.indices[p]
    A.data[p] = A.data[p] * e["D"][i]
    assert not ok(KE.clever_q_ratios(A, d.H, d.J, e["first"], e["gU"], e["D"], "scaled"))
    # a value one ulp beyond the bound of a single product
    dx = e["dx"].copy(); dx[0] = np.nextafter(np.nextafter(dx[0], np.inf), np.inf)
    assert not ok(KE.clever_unscale_ratios(e["sol"], e["D"], d.n, dx, e["v"]))
    # a row that no group lists
    with pytest.raises(AssertionError):
        KE.clever_dy_ratios(d.groups[:-1], u, e["symrhs"], e["crhs"], e["gU"], e["v"], e["dy"])


@pytest.mark.parametrize("name", ["cg_mix", "b8"])
def test_references_reject_the_wrong_x_diagonal(name):
    d = CD[name]
    e = float_eval(d, "u_and_x")
    assert np.count_nonzero(d.H.diagonal()) and e["D"][0] != 1.0
    # the scaled diagonal kept with delta != 0; the unscaled one kept with delta = 0
    assert not ok(KE.clever_q_ratios(e["A"], d.H, d.J, e["first"], e["gU"], e["D"], "true"))
    assert not ok(KE.clever_q_ratios(e["A_true"], d.H, d.J, e["first"], e["gU"], e["D"], "scaled"))
    # the x scale left out of D
    D = e["D"].copy(); D[: d.n] = 1.0
    assert not ok(KE.clever_d_ratios("u_and_x", e["mu"], e["xinf"], d.n, e["gU"], D))
    # mu / U instead of mu / sqrt(U)
    D = e["D"].copy(); D[d.n] = e["mu"] / e["gU"][0]
    assert not ok(KE.clever_d_ratios("u_and_x", e["mu"], e["xinf"], d.n, e["gU"], D))


def test_pattern_reference_on_a_small_case():
    H = sp.csc_matrix(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 3.0, 4.0]]))
    J = sp.csc_matrix(np.array([[1.0, 0, 2.0], [2.0, 0, 4.0], [0, 0, 0], [0, 5.0, 0]]))
    first, _ = KO.compute_indicies(J)
    assert first == [0, 2, 3]
    ptr, idx = KE.clever_pattern(H, J, first)
    assert list(ptr) == [0, 3, 6, 8, 9, 10, 11] and list(idx) == [0, 1, 3, 1, 2, 5, 2, 3, 3, 4, 5]
