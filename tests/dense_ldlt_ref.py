"""NumPy restatement of the dense Bunch-Kaufman factorisation of csrc/dense_ldlt.hip, the designed inputs of
its tests and the LAPACK-side yardsticks.

bunch_kaufman(S) makes the pivot choices of LAPACK's dsytf2 / dlasyf, lower variant: alpha = (1 + sqrt 17) / 8, the same three
comparisons in the same order, the first largest entry on a tie.  It is unblocked and right-looking (the blocked device code computes
the same numbers in another order), and it reports for every comparison that decided something the relative margin |a - b| / max(|a|,
|b|) between its two sides -- for the search of the largest entry the margin between the largest and the runner-up, recorded only where
the index is used.  A device run can be asked to reproduce ipiv exactly only where the smallest margin is far above rounding."""
import numpy as np

ALPHA = (1.0 + np.sqrt(17.0)) / 8.0


def _margin(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else np.inf


def bunch_kaufman(S):
    """P S P' = L D L'.  Returns dict(L, D, perm, ipiv, inertia=(pos, neg, zero), margin): L unit lower triangular with every
    interchange applied to every column, D block diagonal (dense array), perm with (P S P')[i, j] = S[perm[i], perm[j]], ipiv in
    dsytrf's convention (1-based, negative pairs), margin the smallest relative margin of the deciding comparisons."""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    A = np.tril(A) + np.tril(A, -1).T
    L = np.eye(n)
    D = np.zeros((n, n))
    perm = np.arange(n)
    ipiv = np.zeros(n, dtype=np.int32)
    pos = neg = zero = 0
    margin = np.inf
    k = 0
    while k < n:
        absakk = abs(A[k, k])
        if k + 1 < n:
            col = np.abs(A[k + 1:, k])
            imax = k + 1 + int(np.argmax(col))
            colmax = col[imax - k - 1]
        else:
            imax, colmax = k, 0.0
        kstep, kp, is_zero = 1, k, False
        if max(absakk, colmax) == 0.0:
            is_zero = True
        else:
            margin = min(margin, _margin(absakk, ALPHA * colmax))
            if not absakk >= ALPHA * colmax:
                if col.size > 1:
                    second = np.partition(col, -2)[-2]
                    margin = min(margin, _margin(colmax, second))
                row = np.abs(A[imax, k:]).copy()
                row[imax - k] = 0.0
                rowmax = row.max()
                margin = min(margin, _margin(absakk, ALPHA * colmax * (colmax / rowmax)))
                if absakk >= ALPHA * colmax * (colmax / rowmax):
                    kp = k
                else:
                    margin = min(margin, _margin(abs(A[imax, imax]), ALPHA * rowmax))
                    kp = imax
                    if not abs(A[imax, imax]) >= ALPHA * rowmax:
                        kstep = 2
        kk = k + kstep - 1
        if kp != kk:
            A[[kk, kp], :] = A[[kp, kk], :]
            A[:, [kk, kp]] = A[:, [kp, kk]]
            L[[kk, kp], :k] = L[[kp, kk], :k]
            perm[[kk, kp]] = perm[[kp, kk]]
        if kstep == 1:
            d = A[k, k]
            D[k, k] = d
            ipiv[k] = kp + 1
            if is_zero:
                zero += 1
            else:
                pos += d > 0
                neg += d < 0
                l = A[k + 1:, k] / d
                L[k + 1:, k] = l
                A[k + 1:, k + 1:] -= np.outer(l, A[k + 1:, k])
        else:
            Dk = A[k:k + 2, k:k + 2].copy()
            D[k:k + 2, k:k + 2] = Dk
            ipiv[k] = ipiv[k + 1] = -(kp + 1)
            pos += 1
            neg += 1
            W = A[k + 2:, k:k + 2].copy()
            d21 = Dk[1, 0]
            d11, d22 = Dk[1, 1] / d21, Dk[0, 0] / d21
            t = (1.0 / (d11 * d22 - 1.0)) / d21
            l = np.stack([t * (d11 * W[:, 0] - W[:, 1]), t * (d22 * W[:, 1] - W[:, 0])], axis=1)      # W D^-1 as dlasyf forms it
            L[k + 2:, k:k + 2] = l
            A[k + 2:, k + 2:] -= l @ W.T
        k += kstep
    return dict(L=L, D=D, perm=perm, ipiv=ipiv, inertia=(int(pos), int(neg), int(zero)), margin=margin)


def unpack_lapack(LD, ipiv):
    """(L, D, perm) with S[perm][:, perm] = L D L' from dsytrf's lower layout (what okkt_schur_get_factor and scipy's dsytrf return):
    column k of the stored L carries the interchanges made up to its own step only, so the later ones are applied here."""
    n = LD.shape[0]
    L = np.tril(LD, -1) + np.eye(n)
    D = np.diag(np.diag(LD)).astype(np.float64)
    perm = np.arange(n)
    k = 0
    while k < n:
        if ipiv[k] > 0:
            kk, kp, step = k, ipiv[k] - 1, 1
        else:
            kk, kp, step = k + 1, -ipiv[k] - 1, 2
            D[k + 1, k] = D[k, k + 1] = LD[k + 1, k]
            L[k + 1, k] = 0.0
        if kp != kk:
            L[[kk, kp], :k] = L[[kp, kk], :k]
            perm[[kk, kp]] = perm[[kp, kk]]
        k += step
    return L, D, perm


def reconstruction_error(S, L, D, perm):
    S = np.tril(S) + np.tril(S, -1).T
    return float(np.max(np.abs(S[np.ix_(perm, perm)] - L @ D @ L.T)))


def scipy_reconstruction_error(S):
    """max |P S P' - L D L'| of LAPACK's own dsytrf on S (scipy.linalg.ldl drives it and hands back the permuted factor)"""
    import scipy.linalg
    S = np.tril(S) + np.tril(S, -1).T
    lu, d, p = scipy.linalg.ldl(S, lower=True)
    return float(np.max(np.abs(S - lu @ d @ lu.T)))


def omega(S, x, b):
    """componentwise backward error max_i |b - S x|_i / (|S| |x| + |b|)_i"""
    r = np.abs(b - S @ x)
    den = np.abs(S) @ np.abs(x) + np.abs(b)
    return float(np.max(np.where(den > 0, r / np.where(den > 0, den, 1.0), 0.0)))


def inertia_eig(S, drop=0):
    """(pos, neg, zero) from eigvalsh; drop: the number of eigenvalues known to be exactly zero (the smallest in magnitude)"""
    w = np.linalg.eigvalsh(np.tril(S) + np.tril(S, -1).T)
    if drop:
        w = w[np.argsort(np.abs(w))[drop:]]
    return int((w > 0).sum()), int((w < 0).sum()), int(drop)


# ---- designed inputs -------------------------------------------------------------------------------------------------------------
def antidiagonal(n):
    """zero diagonal, unit anti-diagonal pairs: every pivot is 2 x 2 (an odd order keeps a -1 in the middle)"""
    S = np.zeros((n, n))
    for i in range(n):
        S[i, n - 1 - i] = 1.0
    if n % 2:
        S[n // 2, n // 2] = -1.0
    return S


def definite(n, seed=0):
    """strictly diagonally dominant and positive: every pivot is 1 x 1 and stays in place"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-1.0, 1.0, (n, n))
    return (E + E.T) / 2 + (n + 1.0) * np.eye(n)


def heavy_tail(n, seed=0):
    """S[i, j] = s_i s_j E[i, j] with s growing tenfold towards the last rows and a weak diagonal: the largest entry of a column sits
    in the last rows, far beyond the panel, and the diagonal there cannot serve either -- the steps interchange across the panels"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(0.5, 1.0, (n, n)) * rng.choice([-1.0, 1.0], (n, n))
    E = np.tril(E, -1) + np.tril(E, -1).T + np.diag(0.3 * rng.choice([-1.0, 1.0], n))
    s = 1.0 + 9.0 * np.arange(n) / max(n - 1, 1)
    return E * np.outer(s, s)


def pair_at(n, p, seed=0):
    """definite(n) with the rows and columns p, p + 1 cut loose and replaced by [[0.1, 1], [1, -0.1]]: a 2 x 2 pivot on exactly these
    columns, 1 x 1 pivots in place everywhere else (so the panels end where the width says)"""
    S = definite(n, seed)
    S[[p, p + 1], :] = 0.0
    S[:, [p, p + 1]] = 0.0
    S[p, p], S[p + 1, p], S[p, p + 1], S[p + 1, p + 1] = 0.1, 1.0, 1.0, -0.1
    return S


def spectrum(n, seed=0):
    """random symmetric indefinite with prescribed eigenvalues, |lambda| log-uniform in [1e-3, 1], both signs"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = 10.0 ** rng.uniform(-3.0, 0.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    lam[0] = 1.0
    S = (Q * lam) @ Q.T
    return (S + S.T) / 2


def singular(n, seed=0):
    """spectrum(n) with row and column n // 3 set to zero: exactly one zero pivot"""
    S = spectrum(n, seed)
    z = n // 3
    S[z, :] = 0.0
    S[:, z] = 0.0
    return S
