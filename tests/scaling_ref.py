"""numpy restatement of the symmetric equilibration of okkt_set_scaling (include/okkt.h), and the small
matrices the scaling tests share.

A is the full symmetric matrix of a square CSC input: lower triangle read, upper entries ignored, duplicates summed in input order.
s starts at 1; a sweep takes r_i = max_j ((|a_ij| * s_i) * s_j) over the finite entries of every row from the old s and sets
s_i <- s_i / sqrt(r_i) where r_i is positive and finite; after the last sweep s_i = m 2^e (1/2 <= m < 1) becomes 2^(e-1) when
m < fl(sqrt(1/2)) and 2^e otherwise, the exponent clamped to [-510, 510]."""
import numpy as np
import scipy.sparse as sp

SQRT_HALF = float(np.sqrt(0.5))      # 0x1.6a09e667f3bcdp-1
EXP_MAX = 510


def arrays(A):
    """(dim, colptr, rowval, nzval) 0-based of a scipy matrix (brought to sorted CSC, as linear_system_solvers.csc_arrays does) or of
    a (dim, colptr, rowval, nzval, base) tuple taken as it is (duplicates and order kept)."""
    if isinstance(A, tuple):
        dim, colptr, rowval, nzval, base = A
        return int(dim), np.asarray(colptr, dtype=np.int64) - base, np.asarray(rowval, dtype=np.int64) - base, np.asarray(nzval, dtype=np.float64)
    A = sp.csc_matrix(A)
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)


def symmetric_entries(A, shift=None):
    """(row, col, value) of every entry of the full symmetric matrix, each (i, j) pair once per side; shift[i] is added to a stored a_ii"""
    dim, colptr, rowval, nzval = arrays(A)
    col = np.repeat(np.arange(dim, dtype=np.int64), np.diff(colptr))
    keep = rowval >= col
    r, c, v = rowval[keep], col[keep], nzval[keep]
    uniq, inv = np.unique(c * dim + r, return_inverse=True)
    sums = np.zeros(len(uniq))
    np.add.at(sums, inv, v)              # unbuffered: the duplicates of a pair are added in input order, from 0
    r, c = uniq % dim, uniq // dim
    if shift is not None:
        dg = r == c
        sums[dg] = sums[dg] + np.asarray(shift, dtype=np.float64)[r[dg]]
    off = r != c
    return dim, np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([sums, sums[off]])


def row_maxima(n, R, Cc, V, s):
    """r_i = max_j (|a_ij| s_i) s_j over the finite entries (0 for a row without any)"""
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (np.abs(V) * s[R]) * s[Cc]
    prod[~np.isfinite(V)] = 0.0
    out = np.zeros(n)
    np.maximum.at(out, R, prod)
    return out


def round_pow2(s):
    """(rounded s, exponents)"""
    ok = (s > 0) & np.isfinite(s)
    m, e = np.frexp(np.where(ok, s, 1.0))
    e = np.where(m < SQRT_HALF, e - 1, e)
    e = np.clip(np.where(ok, e, 0), -EXP_MAX, EXP_MAX).astype(np.int64)
    return np.ldexp(1.0, e), e


def ruiz_unrounded(A, sweeps=10, shift=None):
    n, R, Cc, V = symmetric_entries(A, shift)
    s = np.ones(n)
    for _ in range(sweeps):
        r = row_maxima(n, R, Cc, V, s)
        upd = (r > 0) & np.isfinite(r)
        s = np.where(upd, s / np.sqrt(np.where(upd, r, 1.0)), s)
    return s


def info_of(A, s, shift=None):
    """rowmax_min, rowmax_max over the non-zero rows of |S A S| (0, 0 without any) and the number of zero rows"""
    n, R, Cc, V = symmetric_entries(A, shift)
    r = row_maxima(n, R, Cc, V, s)
    nz = r > 0
    return dict(rowmax_min=float(r[nz].min()) if nz.any() else 0.0, rowmax_max=float(r.max()) if n else 0.0,
                zero_rows=int((~nz).sum()), rowmax=r)


def ruiz(A, sweeps=10, shift=None):
    """(s, exponents, info) as okkt_get_scaling returns them after a OKKT_SCALE_RUIZ factorisation"""
    s, e = round_pow2(ruiz_unrounded(A, sweeps, shift))
    return s, e, info_of(A, s, shift)


def mantissa_margin(A, sweeps=10, shift=None):
    """min_i |m_i - sqrt(1/2)| over the unrounded s_i = m_i 2^e: how far the input keeps every rounding from its threshold"""
    m, _ = np.frexp(ruiz_unrounded(A, sweeps, shift))
    return float(np.min(np.abs(m - SQRT_HALF))) if len(m) else 1.0


def prescaled(A, s):
    """the same CSC pattern and entry order with the values (s_row * v) * s_col: a scipy matrix for a scipy matrix, a tuple for a tuple"""
    dim, colptr, rowval, nzval = arrays(A)
    col = np.repeat(np.arange(dim, dtype=np.int64), np.diff(colptr))
    v = (s[rowval] * nzval) * s[col]
    if isinstance(A, tuple):
        return (dim, colptr.copy(), rowval.copy(), v, 0)
    return sp.csc_matrix((v, rowval.copy(), colptr.copy()), shape=(dim, dim))


# ---- the small matrices of the tests ---------------------------------------------------------------------------------------------

def random_symmetric(n, seed, per_row=5, off_decades=12, diag_decades=15):
    """lower CSC: off-diagonal entries over 10^+-off_decades, the diagonal over 10^+-diag_decades, random signs"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, n, size=n * per_row)
    c = rng.integers(0, n, size=n * per_row)
    keep = r > c
    v = rng.choice([-1.0, 1.0], size=keep.sum()) * 10.0 ** rng.uniform(-off_decades, off_decades, size=keep.sum())
    d = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-diag_decades, diag_decades, size=n)
    A = sp.coo_matrix((np.concatenate([v, d]), (np.concatenate([r[keep], np.arange(n)]), np.concatenate([c[keep], np.arange(n)]))),
                      shape=(n, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return A


def arrow(n=300, seed=3):
    """lower CSC of an arrow matrix: a diagonal over 10^+-6 and a full last row (more than 256 entries: the long-row kernel) beside
    rows of two entries"""
    rng = np.random.default_rng(seed)
    d = 10.0 ** rng.uniform(-6, 6, size=n)
    last = rng.normal(size=n - 1) * 10.0 ** rng.uniform(-3, 3, size=n - 1)
    rows = np.concatenate([np.arange(n), np.full(n - 1, n - 1)])
    cols = np.concatenate([np.arange(n), np.arange(n - 1)])
    A = sp.coo_matrix((np.concatenate([d, last]), (rows, cols)), shape=(n, n)).tocsc()
    A.sort_indices()
    return A


def with_duplicates_and_upper(n=67, seed=5):
    """a (dim, colptr, rowval, nzval, base) tuple, 1-based: a banded symmetric matrix whose lower entries are partly listed twice (the
    copies sum to the entry) and whose upper triangle holds entries that must be ignored"""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(n):
        ent = []
        if j >= 2:
            ent.append((j - 2, 1e30 * rng.normal()))            # upper triangle: ignored
        ent.append((j, (4.0 + rng.random()) * 10.0 ** rng.uniform(-5, 5)))
        for i in (j + 1, j + 3):
            if i < n:
                v = rng.normal() * 10.0 ** rng.uniform(-4, 4)
                if rng.random() < 0.5:
                    ent.append((i, 0.25 * v)); ent.append((i, 0.75 * v))
                else:
                    ent.append((i, v))
        cols.append(ent)
    colptr = np.cumsum([0] + [len(e) for e in cols]) + 1
    rowval = np.array([i for e in cols for i, _ in e], dtype=np.int64) + 1
    nzval = np.array([v for e in cols for _, v in e])
    return (n, colptr.astype(np.int64), rowval, nzval, 1)


def with_zero_row(n=40, seed=7, z=11):
    """lower CSC, tridiagonal, except that row and column z hold nothing but a stored zero on the diagonal"""
    rng = np.random.default_rng(seed)
    d = (2.0 + rng.random(n)) * 10.0 ** rng.uniform(-4, 4, size=n)
    o = rng.normal(size=n - 1)
    d[z] = 0.0
    o[z - 1] = 0.0
    o[z] = 0.0
    keep = np.ones(n - 1, dtype=bool)
    keep[[z - 1, z]] = False
    A = sp.coo_matrix((np.concatenate([d, o[keep]]), (np.concatenate([np.arange(n), np.arange(1, n)[keep]]),
                                                      np.concatenate([np.arange(n), np.arange(n - 1)[keep]]))), shape=(n, n)).tocsc()
    A.sort_indices()
    return A


def tridiagonal(n, seed):
    rng = np.random.default_rng(seed)
    d = (2.0 + rng.random(n)) * 10.0 ** rng.uniform(-5, 5, size=n)
    o = rng.normal(size=max(n - 1, 0)) * 10.0 ** rng.uniform(-3, 3, size=max(n - 1, 0))
    A = sp.coo_matrix((np.concatenate([d, o]), (np.concatenate([np.arange(n), np.arange(1, n)]),
                                                np.concatenate([np.arange(n), np.arange(n - 1)]))), shape=(n, n)).tocsc()
    A.sort_indices()
    return A


def inertia_counts(A):
    """(positive, negative) eigenvalue counts of the full symmetric matrix, from the prescaled matrix (the counts are those of A:
    Sylvester) so that the eigenvalue solver sees a well-scaled one"""
    s, _, _ = ruiz(A, 10)
    n, R, Cc, V = symmetric_entries(prescaled(A, s))
    w = np.linalg.eigvalsh(sp.coo_matrix((V, (R, Cc)), shape=(n, n)).toarray())
    return int((w > 0).sum()), int((w < 0).sum())


def small_cases():
    """name -> input (scipy lower CSC or a 1-based tuple): what the kernels can get wrong at small sizes"""
    return {
        "arrow-300": arrow(),
        "dups-upper-67": with_duplicates_and_upper(),
        "zero-row-40": with_zero_row(),
        "n1": sp.csc_matrix(np.array([[3.0e-7]])),
        "tridiagonal-67": tridiagonal(67, 9),
    }
