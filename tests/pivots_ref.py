"""NumPy restatement of the threshold pivot report and of the robust driver.

static_ldlt(A, order, ncols) eliminates the first ncols columns of A[order][:, order] without pivoting (right-looking, fp64): L, d and
the trailing Schur complement.  column_maxima restates the report: per pivot column g = max |L_ij| over the stored rows below the
diagonal (a NaN or an Inf counts as +Inf), the partner the lowest such row that attains it, 0 / -1 for a column without rows.  report
counts them against 1 / u.  robust_rounds restates ls_factor_robust at natural ordering (the interior ascending, then the set), with
tests/dense_ldlt_ref.py's Bunch-Kaufman for the dense block, and solve_refine restates the refinement loop with long-double residuals.

Powers of two make the designed cases exact: a multiplier J_ij / H_jj is then the same bits in whichever order the updates are summed."""
import os
import sys

import numpy as np
import scipy.linalg
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ldlt_ref as dref  # noqa: E402

TOL = 2.0 ** -52


def full(A):
    """The dense symmetric matrix of a lower triangle (sparse or dense)."""
    A = A.toarray() if sp.issparse(A) else np.array(A, dtype=np.float64)
    return np.tril(A) + np.tril(A, -1).T


def static_ldlt(A, order=None, ncols=None):
    """(L, d, S): unit lower L (dim x ncols), the pivots d and the Schur complement of the first ncols columns of A[order][:, order]."""
    A = full(A)
    n = A.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    ncols = n if ncols is None else ncols
    W = A[np.ix_(order, order)].copy()
    L = np.zeros((n, ncols))
    d = np.zeros(ncols)
    with np.errstate(all="ignore"):
        for j in range(ncols):
            d[j] = W[j, j]
            L[j, j] = 1.0
            l = W[j + 1:, j] / d[j]
            L[j + 1:, j] = l
            W[j + 1:, j + 1:] -= np.outer(l, W[j + 1:, j])
    return L, d, W[ncols:, ncols:]


def column_max(vals, rows):
    """(g, p) of one column: its stored values below the diagonal and their rows, ascending."""
    if len(vals) == 0:
        return 0.0, -1
    a = np.abs(np.asarray(vals, dtype=np.float64))
    a = np.where(np.isfinite(a), a, np.inf)
    k = int(np.argmax(a))       # the first of equal values: the lowest row
    return float(a[k]), int(rows[k])


def column_maxima(Lcsc, perm, ncols=None):
    """(g, partner) in the original numbering from the strictly lower L in the permuted numbering (CSC, stored zeros kept, rows
    ascending); columns from ncols on (the Schur set) get 0 / -1."""
    n = Lcsc.shape[0]
    ncols = n if ncols is None else ncols
    perm = np.asarray(perm)
    g = np.zeros(n)
    p = np.full(n, -1, dtype=np.int64)
    ip, ix, v = Lcsc.indptr, Lcsc.indices, Lcsc.data
    for j in range(ncols):
        gj, pj = column_max(v[ip[j]:ip[j + 1]], ix[ip[j]:ip[j + 1]])
        g[perm[j]] = gj
        p[perm[j]] = perm[pj] if pj >= 0 else -1
    return g, p


def dense_strict_lower_csc(L, mask=None):
    """The strictly lower part of a dense L (dim x ncols) as CSC with every entry stored (or those of a boolean mask)."""
    n, nc = L.shape
    rows, cols = np.tril_indices(n, -1, nc)
    if mask is not None:
        keep = mask[rows, cols]
        rows, cols = rows[keep], cols[keep]
    M = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    M.sort_indices()
    with np.errstate(all="ignore"):
        M.data = np.array([L[r, c] for r, c in zip(M.indices, np.repeat(np.arange(n), np.diff(M.indptr)))], dtype=np.float64)
    return M


def report(g, u):
    """okkt_pivot_info's counts from g (original order), and the rejected columns in the order of okkt_get_rejected_pivots."""
    g = np.asarray(g)
    rej = np.flatnonzero(g > 1.0 / u)
    rej = rej[np.lexsort((rej, -g[rej]))]
    mx = float(g.max()) if len(g) else 0.0
    return dict(u=u, rejected=len(rej), nonfinite_cols=int(np.sum(g == np.inf)), max_multiplier=mx,
                max_col=int(np.flatnonzero(g == mx)[0]) if len(g) else -1), rej


def omega(Af, x, b):
    """Componentwise backward error with the residual in long double."""
    r = np.abs((b.astype(np.longdouble) - Af.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64))
    den = np.abs(Af) @ np.abs(x) + np.abs(b)
    with np.errstate(all="ignore"):
        q = np.where(den > 0, r / den, np.where(r > 0, np.inf, 0.0))
    return float(np.max(q)) if np.all(np.isfinite(q)) else np.inf


class Factor:
    """A restated factorisation of A at order = (interior ascending, then the set): static L D L' on the interior, Bunch-Kaufman on S."""

    def __init__(self, A, cur):
        self.Af = full(A)
        dim = self.Af.shape[0]
        cur = np.asarray(cur, dtype=np.int64)
        self.order = np.concatenate([np.setdiff1d(np.arange(dim), cur), cur]).astype(np.int64)
        self.n1 = dim - len(cur)
        self.L, self.d, self.S = static_ldlt(self.Af, self.order, self.n1)
        self.bk = dref.bunch_kaufman(self.S) if len(cur) else None

    def multipliers(self):
        return column_maxima(dense_strict_lower_csc(self.L), self.order, self.n1)

    def inertia(self):
        pos, neg = int(np.sum(self.d > 0)), int(np.sum(self.d < 0))
        zero = self.n1 - pos - neg
        if self.bk is not None:
            pos, neg, zero = pos + self.bk["inertia"][0], neg + self.bk["inertia"][1], zero + self.bk["inertia"][2]
        return pos, neg, zero

    def solve(self, b):
        n1 = self.n1
        bp = b[self.order]
        with np.errstate(all="ignore"):
            y1 = scipy.linalg.solve_triangular(self.L[:n1], bp[:n1], lower=True, unit_diagonal=True, check_finite=False) if n1 else bp[:0]
            x2 = np.zeros(0)
            z = y1 / self.d
            if self.bk is not None:
                r2 = (bp[n1:] - self.L[n1:] @ y1)[self.bk["perm"]]
                w = scipy.linalg.solve_triangular(self.bk["L"], r2, lower=True, unit_diagonal=True, check_finite=False)
                w = np.linalg.solve(self.bk["D"], w)
                w = scipy.linalg.solve_triangular(self.bk["L"].T, w, lower=False, unit_diagonal=True, check_finite=False)
                x2 = np.zeros_like(w)
                x2[self.bk["perm"]] = w
                z = z - self.L[n1:].T @ x2
            x1 = scipy.linalg.solve_triangular(self.L[:n1].T, z, lower=False, unit_diagonal=True, check_finite=False) if n1 else z
        x = np.zeros_like(b)
        x[self.order] = np.concatenate([x1, x2])
        return x


def solve_refine(F, b, max_steps=5, tol=TOL):
    """The loop of okkt_solve_refine on a restated factor: (x, dict(steps, status, omega0, omega))."""
    x = F.solve(b)
    w0 = wprev = None
    xprev = None
    steps = 0
    for it in range(max_steps + 1):
        w = omega(F.Af, x, b)
        if it == 0:
            w0 = w
        if not np.isfinite(w):
            if it > 0:
                x, w, steps = xprev, wprev, steps - 1
            return x, dict(steps=steps, status=3, omega0=w0, omega=w)
        if w <= tol:
            return x, dict(steps=steps, status=0, omega0=w0, omega=w)
        if it > 0 and w > 0.5 * wprev:
            if w > wprev:
                x, w, steps = xprev, wprev, steps - 1
            return x, dict(steps=steps, status=2, omega0=w0, omega=w)
        if it >= max_steps:
            return x, dict(steps=steps, status=1, omega0=w0, omega=w)
        r = (b.astype(np.longdouble) - F.Af.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
        xprev, wprev = x, w
        x = x + F.solve(r)
        steps += 1
    raise AssertionError("unreachable")


def robust_rounds(A, n, m, u=1e-8, max_rounds=3, max_set=None):
    """ls_factor_robust at natural ordering.  Returns (flag, info, F): info as the driver's, F the final restated Factor; raises
    RuntimeError where the driver raises OkktError."""
    dim = full(A).shape[0]
    if max_set is None:
        max_set = max(64, int(np.ceil(np.sqrt(dim))))
    cur = np.zeros(0, dtype=np.int64)
    rejected, biggest = [], []
    F = None
    for rnd in range(1, max_rounds + 1):
        F = Factor(A, cur)
        g, p = F.multipliers()
        rep, rej = report(g, u)
        rejected.append(rep["rejected"])
        biggest.append(rep["max_multiplier"])
        if rep["rejected"] == 0:
            break
        par = p[rej]
        grown = np.union1d(cur, np.union1d(rej, par[par >= 0])).astype(np.int64)
        if rnd == max_rounds:
            raise RuntimeError(f"columns are still rejected after {max_rounds} rounds: {rejected}")
        if len(grown) > max_set or len(grown) >= dim:
            raise RuntimeError(f"the Schur set would grow to {len(grown)} variables (max_set = {max_set})")
        cur = grown
    pos, neg, zero = F.inertia()
    flag = int((pos, neg, zero) == (n, m, 0))
    info = dict(rounds=len(rejected), set=cur, rejected=rejected, max_multiplier=biggest, mode="schur" if len(cur) else "plain")
    return flag, info, F


def long_double_solution(A, b, steps=4):
    """The reference solution of the fp64 system: LU with partial pivoting refined with long-double residuals."""
    Af = full(A)
    lu = scipy.linalg.lu_factor(Af)
    x = scipy.linalg.lu_solve(lu, b)
    for _ in range(steps):
        r = (b.astype(np.longdouble) - Af.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
        x = x + scipy.linalg.lu_solve(lu, r)
    return x


def fwd_err(x, xt):
    return float(np.max(np.abs(x - xt)) / np.max(np.abs(xt)))


# ---- the designed KKT systems of the robust route: K = [H J'; J -diag(sigma)], lower triangle, entries powers of two -------------

def designed_kkt(n=40, m=24, tiny=(3, 11, 19, 27, 35), tiny_sigma=(1, 9, 17), seed=0):
    """H diagonal with entries in {1, 2, 4} except H[t] = 2^-40 for t in `tiny`; sigma in {1, 2} except 2^-45 on `tiny_sigma`; J sparse
    with entries +-2^k.  The t-th tiny variable meets exactly one constraint, 2 t (entry 1): its multiplier is 2^40 exactly, and no
    cancellation couples two tiny pivots.  Every constraint also meets a few ordinary variables, one of them with the entry 2^-8, so
    that the static pivot -(sigma + 2^40 + 2^-16 + ...) of a tiny variable's constraint is rounded.
    Returns (K lower CSC, n, m, designed rejected columns, their partners)."""
    rng = np.random.default_rng(seed)
    H = 2.0 ** rng.integers(0, 3, size=n)
    sig = 2.0 ** rng.integers(0, 2, size=m)
    J = np.zeros((m, n))
    ordinary = np.setdiff1d(np.arange(n), tiny)
    for i in range(m):
        cols = rng.choice(ordinary, size=3, replace=False)
        J[i, cols] = rng.choice([-1.0, 1.0], size=3) * 2.0 ** rng.integers(-2, 2, size=3)
        J[i, cols[0]] = np.sign(J[i, cols[0]]) * 2.0 ** -8
    partners = []
    for t, v in enumerate(tiny):
        H[v] = 2.0 ** -40
        J[2 * t, v] = 1.0
        partners.append(n + 2 * t)
    for i in tiny_sigma:
        sig[i] = 2.0 ** -45
    K = np.zeros((n + m, n + m))
    K[:n, :n] = np.diag(H)
    K[n:, :n] = J
    K[n:, n:] = -np.diag(sig)
    Ks = sp.csc_matrix(np.tril(K))
    Ks.sort_indices()
    return Ks, n, m, np.array(sorted(tiny), dtype=np.int64), np.array(partners, dtype=np.int64)
