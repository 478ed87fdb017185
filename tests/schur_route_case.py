"""Shared by test_schur_route_host.py and test_gpu_schur_route.py: the NumPy restatement of the block
recurrence of csrc/dense_ldlt.hip's inverse, the designed dense inputs of its GPU cases, and the tolerance rules.

block_inverse(S) takes the factor of dense_ldlt_ref.bunch_kaufman (unit L with every interchange applied, block diagonal D, perm) as
one front with f = k = ns and r = 0 and walks its blocks of B columns from the last to the first:
    W_j = L_Bj L_jj^-1,   Z_Bj = - Z_BB W_j,   Z_jj = L_jj^-T D_j^-1 L_jj^-1 - W_j' Z_Bj,
then Z[perm[i], perm[j]] = Zt[i, j].  A block ends one column early rather than split a 2 x 2 pivot.

Tolerances.  The dense inverse is held to selinv_case.tolerance's rule, max(1e-8, 100 eps g cond(S)) relative to max |S^-1|, with the
growth g = max(|L| |D| |L'|) / max |S| of the factor the device hands out (schur_get_factor): Bunch-Kaufman bounds g, it does not make
it 1.  The whole-matrix Z through the route uses the same rule with the growth of both factors."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import dense_ldlt_ref as ref

B = 32      # kDlIB of csrc/dense_ldlt.h
EPS = np.finfo(float).eps


def blocks(D, width=B):
    """[c0, .., n]: where the blocks begin, first to last"""
    n = D.shape[0]
    out, c = [], 0
    while c < n:
        out.append(c)
        e = min(n, c + width)
        if e < n and D[e, e - 1] != 0.0:      # (e - 1, e) is a 2 x 2 pivot: it opens the next block
            e -= 1
        c = e
    return out + [n]


def block_inverse(S, width=B):
    r = ref.bunch_kaufman(S)
    L, D, perm = r["L"], r["D"], r["perm"]
    n = D.shape[0]
    Zt = np.zeros((n, n))
    bl = blocks(D, width)
    for j in range(len(bl) - 2, -1, -1):
        c0, j1 = bl[j], bl[j + 1]
        w = j1 - c0
        Li = scipy.linalg.solve_triangular(L[c0:j1, c0:j1], np.eye(w), lower=True, unit_diagonal=True)
        Dj = D[c0:j1, c0:j1]
        Dinv = np.zeros((w, w))
        k = 0
        while k < w:
            if k + 1 < w and Dj[k + 1, k] != 0.0:
                Dinv[k:k + 2, k:k + 2] = np.linalg.inv(Dj[k:k + 2, k:k + 2])
                k += 2
            else:
                Dinv[k, k] = 1.0 / Dj[k, k]
                k += 1
        W = L[j1:, c0:j1] @ Li
        ZB = -Zt[j1:, j1:] @ W
        Zt[j1:, c0:j1] = ZB
        Zt[c0:j1, j1:] = ZB.T
        Zjj = Li.T @ Dinv @ Li - W.T @ ZB
        Zt[c0:j1, c0:j1] = np.tril(Zjj) + np.tril(Zjj, -1).T
    Z = np.zeros((n, n))
    Z[np.ix_(perm, perm)] = Zt
    return Z, r


def full(S):
    return np.tril(S) + np.tril(S, -1).T


# the dense cases of the GPU test: (id, ns, builder).  pair_at puts a 2 x 2 pivot on each edge of the blocks of B columns
SIZES = [2, 3, B - 1, B, B + 1, 2 * B + 1, 257]
PAIR_N = 129
PAIRS = [B - 2, B - 1, B, 2 * B - 1]


def dense_cases():
    out = []
    for ns in SIZES:
        out.append((f"definite-{ns}", ns, lambda ns=ns: ref.definite(ns)))
        out.append((f"antidiagonal-{ns}", ns, lambda ns=ns: ref.antidiagonal(ns)))
        out.append((f"heavy_tail-{ns}", ns, lambda ns=ns: ref.heavy_tail(ns)))
        out.append((f"spectrum-{ns}", ns, lambda ns=ns: ref.spectrum(ns)))
    for p in PAIRS:
        out.append((f"pair_at-{PAIR_N}-{p}", PAIR_N, lambda p=p: ref.pair_at(PAIR_N, p)))
    out.append(("heavy_tail-2049", 2049, lambda: ref.heavy_tail(2049)))
    return out


def dense_growth(LD, ipiv, S):
    """max(|L| |D| |L'|) / max |S| of the factor schur_get_factor hands out"""
    Lf, Df, _ = ref.unpack_lapack(LD, ipiv)
    G = np.abs(Lf) @ np.abs(Df) @ np.abs(Lf).T
    return max(1.0, float(G.max()) / float(np.max(np.abs(S))))


def dense_tolerance(S, g):
    return max(1e-8, 100.0 * EPS * g * np.linalg.cond(full(S)))


def whole_growth(h, A):
    """the growth of the two factors of the Schur route taken as one factor of the permuted A: unit L = [L11 0; L21 L_S] with the
    interior's L (factor_csc) and the dense L of P S P', D = diag(D1, D_S)"""
    n = A.shape[0]
    LD, ipiv = h.schur_get_factor()
    Ls, Ds, perm = ref.unpack_lapack(LD, ipiv)
    ns = LD.shape[0]
    n1 = n - ns
    Lf = sp.lil_matrix(abs(h.factor_csc()))
    L21 = Lf[n1:, :n1].toarray()[perm, :]
    Lw = np.zeros((n, n))
    Lw[:n1, :n1] = Lf[:n1, :n1].toarray() + np.eye(n1)
    Lw[n1:, :n1] = L21
    Lw[n1:, n1:] = np.abs(Ls)
    Dw = np.zeros((n, n))
    Dw[:n1, :n1] = np.diag(np.abs(h.diag()[:n1]))
    Dw[n1:, n1:] = np.abs(Ds)
    G = Lw @ Dw @ Lw.T
    return max(1.0, float(G.max()) / float(np.max(np.abs(A))))
