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


def max_ratio(got, e_b):
    """err / bound of a device maximum against the exact |e_i| with per-component bounds b_i: |max_i |e^_i| - max_i |e_i|| <= max_i b_i."""
    e, b = e_b
    if len(e) == 0:
        return 0.0 if got == 0.0 else math.inf
    return _ratio(got, max(e), float(np.max(b)) / SLACK)
