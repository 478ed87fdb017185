"""A numpy restatement of okkt_solve_gmres for one right-hand side: x = F \\ b, then outer steps of one
extra-precise residual and one right-preconditioned GMRES(restart) cycle on A d = r (classical Gram-Schmidt with one full
reorthogonalisation, Givens rotations, the same stopping rules and the same counts as the device), and plain iterative refinement
with the same residual for comparison.  The residual is taken in np.longdouble and rounded once, standing in for the device's
double-double; the factor F is given as a solve function."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

EPS = 2.0 ** -52
INNER_TOL = 1e-10        # OKKT_GMRES_INNER_TOL


class LongResidual:
    """r = b - A x in long double rounded once and omega = max_i |r_i| / (|A||x| + |b|)_i for the full symmetric CSR M."""

    def __init__(self, M):
        self.M = sp.csr_matrix(M)
        self.data = self.M.data.astype(np.longdouble)
        self.absd = np.abs(self.M.data)

    def product(self, z):
        """A z in long double, rounded once"""
        prod = self.data * z.astype(np.longdouble)[self.M.indices]
        return np.add.reduceat(prod, self.M.indptr[:-1]).astype(np.float64)

    def __call__(self, b, x):
        prod = self.data * x.astype(np.longdouble)[self.M.indices]
        r = (b.astype(np.longdouble) - np.add.reduceat(prod, self.M.indptr[:-1])).astype(np.float64)
        den = np.add.reduceat(self.absd * np.abs(x[self.M.indices]), self.M.indptr[:-1]) + np.abs(b)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.abs(r) == 0, 0.0, np.abs(r) / den)
        if not np.all(np.isfinite(x)):
            return r, float("nan")
        return r, float(np.max(ratio)) if len(r) else 0.0


def dense_solver(F):
    """F \\ v by a pivoted LU of the dense F (a stand-in for the device's factor of the same matrix)."""
    lu = sla.lu_factor(np.asarray(F.todense() if sp.issparse(F) else F))
    return lambda v: sla.lu_solve(lu, v)


def _cycle(resid, solve, r, beta, cap, restart):
    """One GMRES cycle on A d = r with right preconditioner F; returns (d or None, iterations, solves)."""
    n = len(r)
    V = np.zeros((restart + 1, n))
    V[0] = r / beta
    H = np.zeros((restart + 1, restart))
    cs = np.zeros(restart)
    sn = np.zeros(restart)
    g = np.zeros(restart + 1)
    g[0] = beta
    m = 0
    iters = 0
    solves = 0
    for j in range(cap):
        z = solve(V[j])
        solves += 1
        w = resid.product(z)
        iters += 1
        h1 = V[: j + 1] @ w
        w = w - V[: j + 1].T @ h1
        h2 = V[: j + 1] @ w
        w = w - V[: j + 1].T @ h2
        h = np.zeros(j + 2)
        h[: j + 1] = h1 + h2
        h[j + 1] = np.sqrt(w @ w)
        if not np.all(np.isfinite(h)):
            break
        col = h.copy()
        for i in range(j):
            t = cs[i] * col[i] + sn[i] * col[i + 1]
            col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
            col[i] = t
        d = np.hypot(col[j], col[j + 1])
        if not (d > 0.0) or not np.isfinite(d):
            break
        cs[j], sn[j] = col[j] / d, col[j + 1] / d
        col[j], col[j + 1] = d, 0.0
        g[j + 1] = -sn[j] * g[j]
        g[j] = cs[j] * g[j]
        H[: j + 2, j] = col
        m = j + 1
        if abs(g[j + 1]) <= INNER_TOL * beta or not (h[j + 1] > 0.0):
            break
        V[j + 1] = w / h[j + 1]
    if m == 0:
        return None, iters, solves
    y = np.zeros(m)
    for i in range(m - 1, -1, -1):
        y[i] = (g[i] - H[i, i + 1: m] @ y[i + 1: m]) / H[i, i]
    return solve(V[:m].T @ y), iters, solves + 1


def gmres_ir(resid, solve, b, restart=30, max_iters=200, tol=EPS):
    """The device's algorithm for one right-hand side.  Returns (x, info) with the keys of okkt_gmres_info (solves here counts
    solves of one right-hand side) and the omega of every outer step."""
    x = solve(b)
    solves = 1
    iters = cycles = 0
    wprev = 0.0
    xprev = x
    best = None
    omegas = []
    it = 0
    while True:
        r, w = resid(b, x)
        beta = float(np.sqrt(r @ r))
        omegas.append(w)
        if it == 0:
            omega0 = w
        if not np.isfinite(w) or not np.isfinite(beta):
            status = 3
            best = (xprev, wprev) if it > 0 else (x, w)
            break
        if w <= tol:
            status, best = 0, (x, w)
            break
        if it > 0 and w > 0.5 * wprev:
            status = 2
            best = (xprev, wprev) if w > wprev else (x, w)
            break
        if iters >= max_iters:
            status, best = 1, (x, w)
            break
        wprev = w
        cycles += 1
        d, k, s = _cycle(resid, solve, r, beta, min(restart, max_iters - iters), restart)
        iters += k
        solves += s
        if d is not None:
            xprev = x
            x = x + d
        it += 1
    x, w = best
    return x, dict(iterations=iters, cycles=cycles, status=status, solves=solves, omega0=omega0, omega=w, omegas=omegas)


def plain_ir(resid, solve, b, max_solves, tol=EPS):
    """Iterative refinement x += F \\ r with the same residual, max_solves solves in all; returns (x, omega, omegas)."""
    x = solve(b)
    r, w = resid(b, x)
    omegas = [w]
    for _ in range(max_solves - 1):
        if w <= tol:
            break
        x = x + solve(r)
        r, w = resid(b, x)
        omegas.append(w)
    return x, w, omegas
