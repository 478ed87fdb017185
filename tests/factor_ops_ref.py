"""Host reference of the factor-as-an-operator calls (include/okkt.h), from what the handle exports:
factor_csc() (L, strictly lower, permuted numbering), diag() (D), perm() (perm[new] = old) and scaling() (s, original order; None for
an unscaled factor).  Products are accumulated in numpy.longdouble; the quadratic form is exact (fractions.Fraction); the probes of
okkt_factor_error are reproduced from the documented hash.

Factor coordinates: the library holds S P F P^T S = L D L^T; index j of a vector in factor order is original index perm[j]."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LD = np.longdouble


def gamma(m):
    """gamma_m = m u / (1 - m u), elementwise"""
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def _segment_sum(values, seg, n):
    """out[i] = sum of values[e] over seg[e] == i, in long double (seg need not be sorted)"""
    out = np.zeros(n, dtype=LD)
    if len(values) == 0:
        return out
    order = np.argsort(seg, kind="stable")
    s = seg[order]
    v = values[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    out[s[starts]] = np.add.reduceat(v, starts)
    return out


class Factor:
    def __init__(self, Lcsc, d, perm, s=None):
        Lc = sp.csc_matrix(Lcsc)
        self.n = Lc.shape[0]
        self.rows = Lc.indices.astype(np.int64)
        self.cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(Lc.indptr))
        self.val = Lc.data.astype(LD)
        self.aval = np.abs(self.val)
        self.d = np.asarray(d, dtype=np.float64)
        self.perm = np.asarray(perm, dtype=np.int64)
        self.s = None if s is None else np.asarray(s, dtype=np.float64)
        # counts with the unit diagonal: c_j of column j, r_i of row i
        self.colcount = 1 + np.diff(Lc.indptr).astype(np.int64)
        self.rowcount = 1 + np.bincount(self.rows, minlength=self.n).astype(np.int64)
        self.cmax = int(self.colcount.max())
        self.rmax = int(self.rowcount.max())

    # factor coordinates, long double
    def mul_L(self, v, absolute=False):
        v = np.asarray(v, dtype=LD)
        val = self.aval if absolute else self.val
        return v + _segment_sum(val * v[self.cols], self.rows, self.n)

    def mul_LT(self, x, absolute=False):
        x = np.asarray(x, dtype=LD)
        val = self.aval if absolute else self.val
        return x + _segment_sum(val * x[self.rows], self.cols, self.n)

    def to_factor(self, x, absolute=False):
        """P S^-1 x"""
        x = np.asarray(x, dtype=LD)
        t = x if self.s is None else x / self.s.astype(LD)
        t = t[self.perm]
        return np.abs(t) if absolute else t

    def from_factor(self, y):
        """S^-1 P^T y"""
        out = np.zeros(self.n, dtype=LD)
        out[self.perm] = y
        return out if self.s is None else out / self.s.astype(LD)

    def mul_LDLT(self, x, absolute=False):
        """S^-1 P^T L D L^T P S^-1 x, original coordinates (absolute: |L||D||L^T| and |x|)"""
        d = np.abs(self.d).astype(LD) if absolute else self.d.astype(LD)
        u = self.mul_LT(self.to_factor(x, absolute), absolute)
        return self.from_factor(self.mul_L(d * u, absolute))

    def rhs_to_factor(self, b):
        """P S b: what the forward sweep starts from"""
        b = np.asarray(b, dtype=LD)
        t = b if self.s is None else b * self.s.astype(LD)
        return t[self.perm]


def quadform_exact(d, z):
    """(q_pos, q_neg) as Fractions: the sums of d_j z_j^2 over d_j > 0 and over d_j < 0"""
    qp, qn = Fraction(0), Fraction(0)
    for dj, zj in zip(np.asarray(d, dtype=np.float64).tolist(), np.asarray(z, dtype=np.float64).tolist()):
        if dj > 0:
            qp += Fraction(dj) * Fraction(zj) ** 2
        elif dj < 0:
            qn += Fraction(dj) * Fraction(zj) ** 2
    return qp, qn


_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64(z):
    """the finaliser of splitmix64 on an array of uint64 (arithmetic modulo 2^64)"""
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return z ^ (z >> np.uint64(31))


def probe(p, n):
    """probe p of okkt_factor_error: entry i (original index) is -1 when the top bit of mix64((p << 32) ^ i) is set, else +1"""
    i = np.arange(n, dtype=np.uint64)
    top = mix64((np.uint64(p) << np.uint64(32)) ^ i) >> np.uint64(63)
    return np.where(top == 1, -1.0, 1.0)


class Matrix:
    """the full symmetric matrix of a lower triangle (CSC; upper entries ignored, duplicates summed), products in long double"""

    def __init__(self, A_lower):
        A = sp.tril(sp.csc_matrix(A_lower)).tocsc()
        A.sum_duplicates()
        Fm = (A + sp.tril(A, -1).T).tocoo()
        self.n = A.shape[0]
        self.r = Fm.row.astype(np.int64)
        self.c = Fm.col.astype(np.int64)
        self.v = Fm.data.astype(LD)

    def mul(self, x, absolute=False):
        x = np.asarray(x, dtype=LD)
        if absolute:
            return _segment_sum(np.abs(self.v) * np.abs(x[self.c]), self.r, self.n)
        return _segment_sum(self.v * x[self.c], self.r, self.n)


def factor_error(F, A_lower, probes=2):
    """okkt_factor_error on the host: dict(rho, norm_abs_ldlt, norm_f, eta, eta_row) and the per-row quotients of every probe"""
    M = Matrix(A_lower)
    e = np.ones(F.n)
    fe = M.mul(e, absolute=True)
    ae = F.mul_LDLT(e, absolute=True)
    den = fe + ae
    eta, row, quot = 0.0, -1, []
    for p in range(probes):
        v = probe(p, F.n)
        r = np.abs(M.mul(v) - F.mul_LDLT(v))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(r == 0, LD(0), r / den).astype(np.float64)
        quot.append(q)
        i = int(np.argmax(q))          # the lowest row of the maximum
        if row < 0 or q[i] > eta or (q[i] == eta and i < row):
            eta, row = float(q[i]), i
    na, nf = float(ae.max()), float(fe.max())
    return dict(rho=na / nf, norm_abs_ldlt=na, norm_f=nf, eta=eta, eta_row=row), quot, (fe, ae)


def eta_bound(cmax, rmax, h):
    """The bound of DESIGN.md section 8.12 on eta for a factor without pivot trouble: the factorisation's own error
    gamma_{max(cmax, rmax) + h + 3}, the three chained products gamma_{cmax + rmax + h + 2}, the rounding of the difference and of the
    computed denominator."""
    gf = float(gamma(max(cmax, rmax) + h + 3))
    gp = float(gamma(cmax + rmax + h + 2))
    return (gf + gp + 2 * U) * (1 + 2 * gp)


def product_bound(cmax, rmax, h):
    return float(gamma(cmax + rmax + h + 2))


CONTROL = "mixed-level-scatter"      # the design of the negative control of okkt_factor_error


def perturbed(A, F):
    """(the matrix with its largest diagonal entry multiplied by 1 + 2^-20, that row, the quotient the row must produce:
    |delta| / ((|F'| + |L||D||L^T|) e)_row with F' the perturbed matrix)"""
    A = sp.csc_matrix(A).copy()
    dg = A.diagonal()
    row = int(np.argmax(np.abs(dg)))
    Al = A.tolil()
    Al[row, row] = dg[row] * (1.0 + 2.0 ** -20)
    Ap = sp.csc_matrix(Al)
    delta = abs(Ap[row, row] - dg[row])
    fe = Matrix(Ap).mul(np.ones(F.n), absolute=True)
    ae = F.mul_LDLT(np.ones(F.n), absolute=True)
    return Ap, row, float(delta / (fe[row] + ae[row]))


# ---- dense restatements for the self-check ---------------------------------------------------------------------------------------

def dense_static_ldlt(Af, perm):
    """L (unit lower, dense) and d of the static-pivot LDL^T of P Af P^T, in float64"""
    B = np.array(Af[np.ix_(perm, perm)], dtype=np.float64)
    n = B.shape[0]
    Lm = np.eye(n)
    d = np.zeros(n)
    for j in range(n):
        d[j] = B[j, j]
        Lm[j + 1:, j] = B[j + 1:, j] / d[j]
        B[j + 1:, j + 1:] -= np.outer(Lm[j + 1:, j], B[j + 1:, j])
    return Lm, d
