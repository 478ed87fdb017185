"""Exact references of the KKT layer's assembly and row kernels (csrc/kkt.hip), with the rounding bound each device value must meet.

Every reference is the exact value of the operation on the double inputs the device saw: fractions.Fraction in general, error-free
products (Veltkamp / Dekker in numpy) summed with math.fsum for the one design too large for Fraction (a J row of 2100 entries:
2.2 million entries of Q).  sigma_i = fl(y_i / s_i) is an input: IEEE division makes it bitwise the device's sig.

Bound of a value that sums k products (any order, with or without FMA contraction), followed by c more operations:
    |computed - exact| <= gamma_{k+c} * (sum of the absolute values of the terms),   gamma_j = j u / (1 - j u),  u = 2^-53.
Each check returns err / bound per value; a value passes at <= 1.  The absolute sums are rounded sums of positive numbers and the
bound carries a factor 1 + 1e-9 for that."""
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
SLACK = 1.0 + 1e-9


def gamma(k):
    return k * U / (1.0 - k * U)


def F(x):
    return Fraction(float(x))


def _ratio(computed, exact, bound):
    """|computed - exact| / bound, exactly compared (bound 0: 0 when equal, inf otherwise)."""
    err = abs(F(computed) - exact)
    if bound == 0.0:
        return 0.0 if err == 0 else math.inf
    return float(err / F(bound * SLACK))


# ---- Q = J_s' diag(sigma) J_s + H (lower), the Schur kinds' assembly -----------------------------------------------------------
def q_exact(H, J, sig, skip_rows=()):
    """Per lower entry (a, b): [exact value, sum |terms|, number of J terms k, smallest |term|] of tril(J_s' S J_s + H), J_s = J
    without the rows in skip_rows (the dense rows of a bordered system)."""
    out = {}
    Jr = J.tocsr()
    Jr.sort_indices()
    skip = set(int(i) for i in skip_rows)
    for i in range(J.shape[0]):
        if i in skip:
            continue
        c = Jr.indices[Jr.indptr[i]:Jr.indptr[i + 1]]
        v = Jr.data[Jr.indptr[i]:Jr.indptr[i + 1]]
        fv = [F(x) for x in v]
        fs = F(sig[i])
        for p in range(len(c)):
            fp = fv[p] * fs
            for q in range(p + 1):
                t = fp * fv[q]
                a = abs(float(v[p]) * float(sig[i]) * float(v[q]))
                e = out.get((int(c[p]), int(c[q])))
                if e is None:
                    out[(int(c[p]), int(c[q]))] = [t, a, 1, a]
                else:
                    e[0] += t; e[1] += a; e[2] += 1; e[3] = min(e[3], a)
    Hc = H.tocoo()
    for a, b, h in zip(Hc.row, Hc.col, Hc.data):
        e = out.setdefault((int(a), int(b)), [Fraction(0), 0.0, 0, math.inf])
        e[0] += F(h); e[1] += abs(float(h)); e[3] = min(e[3], abs(float(h)))
    return out


def q_ratios(A, ex, n):
    """err / bound of every entry of the Q_s block (rows and columns < n) of the device matrix A against q_exact's entries; entries
    of the pattern that no term reaches must be exactly 0."""
    A = A.tocsc()
    r = []
    for b in range(n):
        for p in range(A.indptr[b], A.indptr[b + 1]):
            a = int(A.indices[p])
            if a >= n:
                continue
            e = ex.get((a, b))
            if e is None:
                r.append(0.0 if A.data[p] == 0.0 else math.inf)
            else:
                r.append(_ratio(A.data[p], e[0], gamma(e[2] + 3) * e[1]))
    return np.array(r)


def _split(a):
    c = 134217729.0 * a             # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e = a * b exactly (Dekker; no FMA in numpy)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def q_ratios_single_term(A, H, J, sig):
    """q_ratios for a Q in which every entry holds at most one J term (the long-row design): exact (J_ia sigma_i) J_ib as four
    doubles from error-free products, plus H_ab, the difference to the device value rounded once by math.fsum."""
    A = A.tocoo()
    Jr = J.tocsr()
    n = J.shape[1]
    # the J term of each entry: (row, value in column a, value in column b); at most one per entry
    ta, tb, tv, tsig = [], [], [], []
    for i in range(J.shape[0]):
        c, v = Jr.indices[Jr.indptr[i]:Jr.indptr[i + 1]], Jr.data[Jr.indptr[i]:Jr.indptr[i + 1]]
        P, Q = np.tril_indices(len(c))
        ta.append(c[P]); tb.append(c[Q]); tv.append(np.stack([v[P], v[Q]])); tsig.append(np.full(len(P), sig[i]))
    ta, tb = np.concatenate(ta).astype(np.int64), np.concatenate(tb).astype(np.int64)
    tv, tsig = np.concatenate(tv, axis=1), np.concatenate(tsig)
    key = ta * n + tb
    assert len(np.unique(key)) == len(key), "an entry with two J terms: use q_ratios"
    keep = (A.row < n) & (A.col < n)
    akey = A.row[keep].astype(np.int64) * n + A.col[keep]
    aval = A.data[keep]
    order = np.argsort(key)
    pos = np.searchsorted(key[order], akey)
    pos = np.minimum(pos, len(key) - 1)
    hit = key[order][pos] == akey
    t = order[pos]
    Ja, Jb, sg = np.where(hit, tv[0, t], 0.0), np.where(hit, tv[1, t], 0.0), np.where(hit, tsig[t], 0.0)
    p1, e1 = two_prod(Ja, sg)
    p2, e2 = two_prod(p1, Jb)
    p3, e3 = two_prod(e1, Jb)
    Hl = sp.csr_matrix(H)
    h = np.asarray(Hl[A.row[keep], A.col[keep]]).ravel()
    diff = np.array([math.fsum(r) for r in np.stack([aval, -p2, -e2, -p3, -e3, -h], axis=1).tolist()])
    bound = gamma(4) * (np.abs(Ja * sg * Jb) + np.abs(h)) * SLACK
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, np.abs(diff) / bound, np.where(diff == 0, 0.0, np.inf))


def diag_ratios(got, H, J, sig):
    """err / bound of schur_diag = diag(H) + sum_i J_ij^2 sigma_i (the whole J), per column."""
    Jc = J.tocsc()
    out = []
    Hd = H.diagonal()
    for j in range(J.shape[1]):
        v, r = Jc.data[Jc.indptr[j]:Jc.indptr[j + 1]], Jc.indices[Jc.indptr[j]:Jc.indptr[j + 1]]
        ex = F(Hd[j]) + sum((F(x) * F(x) * F(sig[i]) for x, i in zip(v, r)), Fraction(0))
        ab = abs(float(Hd[j])) + float(np.sum(v * v * sig[r]))
        out.append(_ratio(got[j], ex, gamma(len(v) + 3) * ab))
    return np.array(out)


# ---- row products ------------------------------------------------------------------------------------------------------------------
def dots(A, x):
    """Per row of A (CSR): [exact sum_j A_ij x_j, sum |A_ij x_j|, k]."""
    A = A.tocsr()
    fx = [F(v) for v in x]
    out = []
    for i in range(A.shape[0]):
        s, ab = Fraction(0), 0.0
        for p in range(A.indptr[i], A.indptr[i + 1]):
            j = A.indices[p]
            s += F(A.data[p]) * fx[j]
            ab += abs(float(A.data[p]) * float(x[j]))
        out.append((s, ab, int(A.indptr[i + 1] - A.indptr[i])))
    return out


def hess(H, x):
    """Per row of hess_product (eval.jl:221-234): (L x)_i + (L' x)_i - diag(L)_i x_i of the lower-stored H: [exact, sum |terms|
    (the diagonal counted three times, as the device touches it), k = the terms of row and column i]."""
    L = H.tocsr()
    Lt = H.T.tocsr()
    r1, r2 = dots(L, x), dots(Lt, x)
    d = H.diagonal()
    return [(a[0] + b[0] - F(d[i]) * F(x[i]), a[1] + b[1] + abs(float(d[i]) * float(x[i])), a[2] + b[2]) for i, (a, b) in enumerate(zip(r1, r2))]


def rhs_ratios(J, grad, cons, s, y, mu, pen, eta, rD, rP, rC):
    """okkt_kkt_system_rhs against System_rhs (system_rhs.jl:57-73 as oracle/kkt_oracle.py:100-110 restates it) in exact
    arithmetic: dual_r = -(grad - J'y + (mu eta_mu) pen J'1) (1 - eta_D), primal_r = -(cons - s)(1 - eta_P), comp_r = mu eta_mu - s y."""
    etaP, etaD, etaM = (F(e) for e in eta)
    JT = J.T.tocsr()
    jy, j1 = dots(JT, y), dots(JT, np.ones(J.shape[0]))
    c = F(mu) * etaM * F(pen)
    rd = []
    for i in range(J.shape[1]):
        ex = -((F(grad[i]) - jy[i][0]) + c * j1[i][0]) * (1 - etaD)
        ab = (abs(grad[i]) + jy[i][1] + float(abs(c)) * j1[i][1]) * float(abs(1 - etaD))
        rd.append(_ratio(rD[i], ex, gamma(jy[i][2] + 6) * ab))
    rp = [_ratio(rP[i], -(F(cons[i]) - F(s[i])) * (1 - etaP), gamma(3) * (abs(cons[i]) + abs(s[i])) * float(abs(1 - etaP))) for i in range(len(s))]
    rc = [_ratio(rC[i], F(mu) * etaM - F(s[i]) * F(y[i]), gamma(3) * (abs(mu * float(etaM)) + abs(s[i] * y[i]))) for i in range(len(s))]
    return np.array(rd), np.array(rp), np.array(rc)


def dyds_ratios(J, dx, rP, rC, y, s, dy, ds, direct):
    """dy, ds of the Schur kinds from the device's own dx (schur.jl:113-116, schur_direct.jl:54-56): dy = -(J dx - (rP + rC ./ y)) .* sig
    with sig = fl(y ./ s); ds = J dx - rP, or (rC - dy .* s) ./ y with the device's dy (direct).  J, y, s: those the kind reads."""
    sig = y / s
    jd = dots(J, dx)
    rdy, rds = [], []
    for i in range(J.shape[0]):
        Jdx, ab, k = jd[i]
        ex = -(Jdx - (F(rP[i]) + F(rC[i]) / F(y[i]))) * F(sig[i])
        rdy.append(_ratio(dy[i], ex, gamma(k + 4) * (ab + abs(rP[i]) + abs(rC[i] / y[i])) * sig[i]))
        if direct:
            rds.append(_ratio(ds[i], (F(rC[i]) - F(dy[i]) * F(s[i])) / F(y[i]), gamma(3) * (abs(rC[i]) + abs(dy[i] * s[i])) / y[i]))
        else:
            rds.append(_ratio(ds[i], Jdx - F(rP[i]), gamma(k + 1) * (ab + abs(rP[i]))))
    return np.array(rdy), np.array(rds)


def kkt_error_exact(H, J, s, y, delta, dx, dy, ds, rD, rP, rC):
    """update_kkt_error! (kkt_system_solver.jl:27-47,67-96; oracle/kkt_oracle.py:190-214) componentwise, in exact arithmetic, with the
    matrices and s, y of the factor iterate: per block (|e_i| exact as a float, bound of the device's |e_i|)."""
    jdx, jty, hx = dots(J, dx), dots(J.T, dy), hess(H, dx)
    eD, bD = [], []
    for i in range(J.shape[1]):
        e = F(delta) * F(dx[i]) + hx[i][0] - jty[i][0] - F(rD[i])
        eD.append(abs(e)); bD.append(gamma(hx[i][2] + jty[i][2] + 6) * (abs(delta * dx[i]) + hx[i][1] + jty[i][1] + abs(rD[i])) * SLACK)
    eP, bP, eM, bM = [], [], [], []
    for i in range(J.shape[0]):
        eP.append(abs(jdx[i][0] - F(ds[i]) - F(rP[i])))
        bP.append(gamma(jdx[i][2] + 2) * (jdx[i][1] + abs(ds[i]) + abs(rP[i])) * SLACK)
        eM.append(abs(F(s[i]) * F(dy[i]) + F(y[i]) * F(ds[i]) - F(rC[i])))
        bM.append(gamma(3) * (abs(s[i] * dy[i]) + abs(y[i] * ds[i]) + abs(rC[i])) * SLACK)
    return (eD, np.array(bD)), (eP, np.array(bP)), (eM, np.array(bM))


def assert_within(r, what):
    """Every err / bound of r is at most 1."""
    assert len(r) == 0 or np.max(r) <= 1.0, (what, float(np.max(r)), int(np.argmax(r)))


def check_err(res, d, tag, delta):
    """The N err record res[tag/err] of a case runner against kkt_error_exact of its own dx, dy, ds and rhs at design d and delta:
    the three maxima within their bounds, rhs_norm, overall and ratio exactly.  Returns kkt_error_exact's blocks."""
    dx, dy, ds, rD, rP, rC = (res[f"{tag}/{k}"] for k in ("dx", "dy", "ds", "rD", "rP", "rC"))
    eD, eP, eM = kkt_error_exact(d.H, d.J, d.s, d.y, delta, dx, dy, ds, rD, rP, rC)
    got = res[f"{tag}/err"]
    for g, e, what in zip(got[:3], (eD, eP, eM), ("error_D", "error_P", "error_mu")):
        assert max_ratio(g, e) <= 1.0, (tag, what, g)
    inf = lambda v: float(np.max(np.abs(v))) if len(v) else 0.0
    assert got[4] == max(inf(rD), inf(rP), inf(rC))          # rhs_norm: maxima are exact
    assert got[3] == max(got[:3]) and got[5] == got[3] / got[4]
    return eD, eP, eM


def max_ratio(got, e_b):
    """err / bound of a device maximum against the exact |e_i| with per-component bounds b_i: |max_i |e^_i| - max_i |e_i|| <= max_i b_i."""
    e, b = e_b
    if len(e) == 0:
        return 0.0 if got == 0.0 else math.inf
    return _ratio(got, max(e), float(np.max(b)) / SLACK)


# ---- the clever-symmetric kind (clever_symmetric.jl) -----------------------------------------------------------------------------
# groups: [(members in ls order, their ratios to the leader)] sorted by leader, as kkt_designs.CleverDesign holds them.  u = fl(s / y)
# is an input (IEEE division: bitwise the device's), 1 / u is a rounding of the path.
def _sqrt_frac(x):
    """sqrt of a positive Fraction as a Fraction, from math.isqrt: relative error below 2^-250, far inside SLACK."""
    k = 300 + x.denominator.bit_length()
    return Fraction(math.isqrt((x.numerator << (2 * k)) // x.denominator), 1 << k)


def clever_u_exact(groups, u):
    """Per group the exact U_g = 1 / sum_t ratio_t^2 (1 / u_t)."""
    return [1 / sum((F(r) * F(r) / F(u[j]) for j, r in zip(mem, rat)), Fraction(0)) for mem, rat in groups]


def clever_u_g_ratios(groups, u, gU, g):
    """update_indicies! (k_clever_groups).  U_g: k positive terms, each 1 / u, ratio^2 and their product, k - 1 additions (fused or
    not), one reciprocal: gamma_{k+3} U.  g_j = U_g ratio_j (1 / u_j) (g indexed by row) with the computed U, 1 / u and two products:
    gamma_{k+6} |g_j| against the exact U."""
    ex = clever_u_exact(groups, u)
    rU, rg = [], []
    for (mem, rat), U_, got in zip(groups, ex, gU):
        k = len(mem)
        rU.append(_ratio(got, U_, gamma(k + 3) * float(U_)))
        for j, r in zip(mem, rat):
            e = U_ * F(r) / F(u[j])
            rg.append(_ratio(g[j], e, gamma(k + 6) * abs(float(e))))
    return np.array(rU), np.array(rg)


def clever_d_ratios(mode, mu, xinf, n, gU, D):
    """diag_rescale (k_clever_rescale and the host's x scale) from the DEVICE's U_g: 1 (none; the x part of u_only), exactly;
    1 / sqrt(1 + |x|_inf) and mu / sqrt(U_g) within gamma_4: the addition, the square root and the division taken as at most one
    ulp each -- the bound does not rely on a correctly rounded device sqrt.  The exact root is a 2^-250 accurate Fraction."""
    out = []
    dx = _sqrt_frac(1 / (1 + F(xinf))) if mode == "u_and_x" else Fraction(1)
    for i in range(n):
        out.append(_ratio(D[i], dx, gamma(4) * float(dx) if mode == "u_and_x" else 0.0))
    for g_, U_ in enumerate(gU):
        e = Fraction(1) if mode == "none" else F(mu) / _sqrt_frac(F(U_))
        out.append(_ratio(D[n + g_], e, 0.0 if mode == "none" else gamma(4) * float(e)))
    return np.array(out)


def clever_pattern(H, J, firsts):
    """The lower pattern of M = [[H 0]; [J_new -U]], J_new = J[firsts, :]: per column j < n the row j itself if H has no diagonal
    there, H's rows, then n + g for every leader row firsts[g] stored in column j of J, ascending; per column n + g its diagonal."""
    H, J = H.tocsc(), J.tocsc()
    H.sort_indices(); J.sort_indices()
    n = J.shape[1]
    grp = {int(r): g for g, r in enumerate(firsts)}
    ptr, idx = [0], []
    for j in range(n):
        hr = [int(r) for r in H.indices[H.indptr[j]:H.indptr[j + 1]]]
        idx += ([] if j in hr else [j]) + hr + sorted(n + grp[int(r)] for r in J.indices[J.indptr[j]:J.indptr[j + 1]] if int(r) in grp)
        ptr.append(len(idx))
    for g in range(len(firsts)):
        idx.append(n + g); ptr.append(len(idx))
    return np.array(ptr, np.int64), np.array(idx, np.int64)


def clever_q_ratios(A, H, J, firsts, gU, D, xdiag="scaled"):
    """Every stored entry of the device's Q = D M D (CSC, the pattern of clever_pattern) from the DEVICE's D and U_g: (D_i v) D_j with
    v an entry of H, of a leader's J row or -U_g -- two products, no sum: gamma_2 |value|.  The x diagonal: xdiag = "scaled":
    (D_j h_jj) D_j (after form_system, and after factor! with delta = 0); "true": H's diagonal, unscaled, bit for bit (after factor!
    with delta != 0).  A diagonal entry that H does not store is exactly 0."""
    A = A.tocsc()
    n = J.shape[1]
    Hd, Jd = sp.dok_matrix(H.tocsc()), sp.dok_matrix(J.tocsc())
    out = []
    for j in range(A.shape[1]):
        for p in range(A.indptr[j], A.indptr[j + 1]):
            i = int(A.indices[p])
            if j >= n:
                v = -float(gU[j - n])
            elif i >= n:
                v = float(Jd[int(firsts[i - n]), j])
            else:
                v = float(Hd.get((i, j), 0.0))
            if i == j and j < n and xdiag == "true":
                out.append(0.0 if A.data[p] == v and not (v == 0.0 and math.copysign(1.0, A.data[p]) < 0) else math.inf)
                continue
            e = F(D[i]) * F(v) * F(D[j])
            out.append(_ratio(A.data[p], e, gamma(2) * abs(float(e))))
    return np.array(out)


def clever_symrhs_ratios(rP, rC, y, symrhs):
    """symmetric_primal_rhs = rP + rC / y (k_clever_symrhs): a division and an addition, gamma_2 (|rP| + |rC / y|)."""
    return np.array([_ratio(symrhs[i], F(rP[i]) + F(rC[i]) / F(y[i]), gamma(2) * (abs(rP[i]) + abs(rC[i] / y[i]))) for i in range(len(y))])


def clever_crhs_ratios(groups, g, symrhs, crhs):
    """crhs_g = sum_t g_t symrhs_t (k_clever_crhs) from the device's g and symrhs: k products summed, gamma_k sum |terms|."""
    out = []
    for (mem, _), got in zip(groups, crhs):
        ex = sum((F(g[j]) * F(symrhs[j]) for j in mem), Fraction(0))
        out.append(_ratio(got, ex, gamma(len(mem)) * sum(abs(g[j] * symrhs[j]) for j in mem)))
    return np.array(out)


def clever_unscale_ratios(sol, D, n, dx, v):
    """dx, v = sol .* D (k_clever_unscale): one product, gamma_1 |value|."""
    got = np.concatenate([dx, v])
    return np.array([_ratio(got[i], F(sol[i]) * F(D[i]), gamma(1) * abs(sol[i] * D[i])) for i in range(len(got))])


def clever_dy_terms(groups, u, symrhs, crhs, gU, v):
    """Per row j the two exact terms of dy_j = (1 / u_j) symrhs_j + ((1 / u_j) ratio_j) (-(crhs_g + U_g v_g)) and the sum of the
    absolute values the bound takes (|crhs| + |U v| inside the second)."""
    t = {}
    for g_, (mem, rat) in enumerate(groups):
        br = -(F(crhs[g_]) + F(gU[g_]) * F(v[g_]))
        ab = abs(crhs[g_]) + abs(gU[g_] * v[g_])
        for j, r in zip(mem, rat):
            t[j] = (F(symrhs[j]) / F(u[j]), F(r) / F(u[j]) * br, abs(symrhs[j] / u[j]) + abs(r / u[j]) * ab)
    return t


def clever_dy_ratios(groups, u, symrhs, crhs, gU, v, dy):
    """dir.y (k_clever_y) from the device's own inputs: 1 / u, the product U v, its sum with crhs, three more products and the last
    sum -- no value passes more than six roundings: gamma_6 times the sum of the absolute values of the two terms."""
    t = clever_dy_terms(groups, u, symrhs, crhs, gU, v)
    assert sorted(t) == list(range(len(dy))), "a row that no group lists"
    return np.array([_ratio(dy[j], t[j][0] + t[j][1], gamma(6) * t[j][2]) for j in range(len(dy))])


def ds_ratios(J, dx, rP, ds):
    """ds = J dx - rP from the device's dx, as dyds_ratios' non-direct branch."""
    return np.array([_ratio(ds[i], e - F(rP[i]), gamma(k + 1) * (ab + abs(rP[i]))) for i, (e, ab, k) in enumerate(dots(J, dx))])
