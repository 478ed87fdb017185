"""numpy restatement of the condition estimator of condest.hip / api_condest.cpp: Higham and Tisseur's block 1-norm
estimator (Algorithm 2.4) applied to F^-1 (or diag(f) F^-1), with the same fixed generator, the same replacement of parallel sign
columns and the same tie rules.  `solve(B)` returns F^-1 B for an n x t block; the tests drive it with exact dense solves."""
import numpy as np

ITMAX = 5
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(z):
    """splitmix64's finaliser on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def gen_column(draw, cls, n):
    """The +-1 column of draw `draw` and head class `cls`: rows 0 .. H-1 (H = min(n, 4)) carry the class (row 0 is +1, row r is -1
    when bit r-1 of cls is set), the other rows the sign bit of splitmix64((draw << 32) ^ i)."""
    i = np.arange(n, dtype=np.uint64)
    z = _mix((np.uint64(draw) << np.uint64(32)) ^ i)
    s = np.where((z >> np.uint64(63)) != 0, -1.0, 1.0)
    H = min(n, 4)
    for r in range(H):
        s[r] = 1.0 if (r == 0 or not (cls >> (r - 1)) & 1) else -1.0
    return s


def _cls(col, H):
    c = 0
    for r in range(1, H):
        if col[r] != col[0]:
            c |= 1 << (r - 1)
    return c


def estimate(solve, n, t=2, f=None):
    """The estimate of ||op||_1, op = diag(f) F^-1 (f None: F^-1).  Returns dict(est, iterations, solves, status, indices)."""
    t = 2 if t <= 0 else min(t, 4)
    t = min(t, n)
    H = min(n, 4)
    w = np.ones(n) if f is None else np.asarray(f, dtype=np.float64)
    X = np.empty((n, t))
    X[:, 0] = 1.0 / n
    for j in range(1, t):
        X[:, j] = gen_column(j, j, n) / n
    hist = []
    est = est_old = 0.0
    ind_best = -1
    ind = [-1] * t
    S_old = None
    cls_old = [0] * t
    next_draw = t
    solves = iters = 0
    status = 1
    k = 0
    while True:
        k += 1
        Y = solve(X) * w[:, None]
        solves += 1
        if not np.all(np.isfinite(Y)):
            status, est = 3, np.inf
            break
        norms = np.abs(Y).sum(axis=0)
        jb = int(np.argmax(norms))        # the first maximum: the lowest column
        e = float(norms[jb])
        if (e > est_old or k == 2) and k >= 2:
            ind_best = ind[jb]
        if k >= 2 and e <= est_old:
            est, status = est_old, 0
            break
        est = est_old = e
        if k > ITMAX:
            status = 1
            break
        S = np.where(Y >= 0.0, 1.0, -1.0)
        has_old = S_old is not None
        SO = S.T @ S_old if has_old else None
        SS = S.T @ S

        def par_old(a):
            return has_old and any(abs(SO[a, c]) == n for c in range(t))
        if has_old and all(par_old(a) for a in range(t)):
            status = 0
            break
        cls = [_cls(S[:, a], H) for a in range(t)]
        repl = [False] * t
        if t > 1:
            for a in range(t):
                par = par_old(a) or any(not repl[b] and abs(SS[a, b]) == n for b in range(a))
                if not par:
                    continue
                for c in range(1 << (H - 1)):
                    if any((b != a and cls[b] == c) or (has_old and cls_old[b] == c) for b in range(t)):
                        continue
                    S[:, a] = gen_column(next_draw, c, n)
                    next_draw += 1
                    cls[a] = c
                    repl[a] = True
                    break
        cls_old = list(cls)
        Z = solve(S * w[:, None])
        solves += 1
        iters += 1
        if not np.all(np.isfinite(Z)):
            status, est = 3, np.inf
            break
        h = np.abs(Z).max(axis=1)
        order = np.lexsort((np.arange(n), -h))       # h descending, then the lower row
        if k >= 2 and h[order[0]] == h[ind_best]:
            status = 0
            break
        if t > 1:
            used = set(hist)
            if all(int(i) in used for i in order[:t]):
                status = 0
                break
            fresh = [int(i) for i in order if int(i) not in used][:t]
            if len(fresh) < t:
                status = 0
                break
            ind = fresh
        else:
            ind = [int(order[0])]
        X = np.zeros((n, t))
        for a, i in enumerate(ind):
            X[i, a] = 1.0
        hist.extend(ind)
        S_old = S
    return dict(est=est, iterations=iters, solves=solves, status=status, indices=hist)


def condest(F, t=2):
    """(||F||_1, estimate of ||F^-1||_1, result dict) for a dense symmetric F, by exact dense solves."""
    import scipy.linalg as sl
    F = np.asarray(F, dtype=np.float64)
    lu = sl.lu_factor(F)
    r = estimate(lambda B: sl.lu_solve(lu, B), F.shape[0], t)
    return float(np.abs(F).sum(axis=0).max()), r["est"], r


def dense_symmetric(A, shift=None):
    """The dense symmetric matrix of a lower-triangle CSC (upper entries ignored, duplicates summed) plus diag(shift)."""
    import scipy.sparse as sp
    L = sp.tril(sp.csc_matrix(A)).toarray()
    F = L + np.tril(L, -1).T
    if shift is not None:
        F[np.diag_indices_from(F)] += shift
    return F
