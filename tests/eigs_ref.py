"""numpy restatement of the block shift-invert Krylov-Schur method of okkt_eigs (include/okkt.h) and the designs
its tests run: the same hashed start block (splitmix64 of (seed, column, row), bit for bit), the same two classical Gram-Schmidt passes
(the block against the basis, then column by column inside the block), the same drop rule (2^-33 of the norm before), the same two
restart rules (the next block is taken against the whole basis before the compression; a block is never truncated) and the same
returned vectors v = F^-1 E' x.  The projected problem is solved by numpy.linalg.eigh here and by cyclic Jacobi in the library, and the
sums run in another order, so the two agree to rounding, not bit for bit; only the start block is compared bitwise.

Designs.  Quasi-definite KKT matrices K = [[H, J'], [J, -inv(Sigma)]] (H positive definite, Sigma over six decades), which a static-pivot
L D L' factors stably in any order; the pencil designs take the x-block as the leading block, so their (2,2) block -inv(Sigma) is
nonsingular.  Orders sit around the constants of the kernels: 1, 2, 3, 5 (below and just above the block width), 63 / 64 / 65 (a wave),
255 / 256 / 257 (a workgroup), 1029 (just past twice the 512 rows one workgroup of a reduction covers: three workgroups).  A design with
|lambda_1| / ||A|| ~ 1e-12, three identical diagonal blocks plus well-separated extra eigenvalues, and a tree of the front_trees
catalogue.  Every (design, nev) has a relative gap >= 1.005 between |lambda_nev| and |lambda_nev+1| -- the seed is the first that
gives one -- and the gap is part of the case id."""
import functools

import numpy as np
import scipy.sparse as sp

import front_trees as FT

MASK = (1 << 64) - 1
DROP = 2.0 ** -33
MIN_GAP = 1.005


# ---- the start block ----------------------------------------------------------------------------------------------------------------
def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def hashed_column(seed, col, n):
    sc = mix((mix(seed & MASK) + col) & MASK)
    out = np.empty(n)
    for i in range(n):
        h = mix((sc + i) & MASK)
        out[i] = (float(h >> 11) * 2.0 ** -52 - 1.0) + 2.0 ** -53
    return out


# ---- the method ---------------------------------------------------------------------------------------------------------------------
def default_basis(n, nev, block):
    floor = 2 * nev + 3 * block
    return max(floor, min(max(48, floor), 128, n))


def sort_ritz(theta, S):
    """|theta| descending, of equal moduli the positive one first."""
    order = sorted(range(len(theta)), key=lambda i: (-abs(theta[i]), -theta[i]))
    return theta[order], S[:, order]


def finish(v, nlead):
    """Unit 2-norm of the leading part, its entry of largest modulus (lowest index among ties) positive."""
    lead = v[:nlead]
    i = int(np.argmax(np.abs(lead)))
    return v * ((-1.0 if lead[i] < 0 else 1.0) / np.linalg.norm(lead))


def reference_eigs(F, nev, block=4, max_basis=0, max_restarts=20, tol=0.0, nlead=0, seed=1):
    """(lam, V, info) of the scheme on the dense symmetric F; V has one full-length vector per row."""
    dim = F.shape[0]
    pencil = 0 < nlead < dim
    n = nlead if pencil else dim
    Finv = np.linalg.inv(F)
    Op = Finv[:n, :n]
    tol = tol if tol > 0 else 2.0 ** -26
    mb = max_basis if max_basis else default_basis(n, nev, block)
    assert 1 <= nev <= min(32, n) and 1 <= block <= 4 and 2 * nev + 3 * block <= mb <= 128
    info = dict(status=1, nconv=0, sweeps=0, solves=0, restarts=0, basis=mb, fresh_blocks=0, dropped_columns=0)
    V, OV = np.zeros((n, 0)), np.zeros((n, 0))
    G = np.zeros((0, 0))
    state = dict(next_col=0)

    def orth_block(Q):
        norm0 = np.linalg.norm(Q, axis=0)
        if V.shape[1]:
            for _ in range(2):
                Q = Q - V @ (V.T @ Q)
        kept = []
        for j in range(Q.shape[1]):
            w = Q[:, j]
            if kept:
                B = np.column_stack(kept)
                for _ in range(2):
                    w = w - B @ (B.T @ w)
            nrm = np.linalg.norm(w)
            if nrm > 0 and nrm >= DROP * norm0[j]:
                kept.append(w / nrm)
            else:
                info["dropped_columns"] += 1
        return np.column_stack(kept) if kept else np.zeros((n, 0))

    def fresh():
        Q = np.column_stack([hashed_column(seed, state["next_col"] + c, n) for c in range(block)])
        state["next_col"] += block
        return orth_block(Q)

    Q = fresh()
    theta, S, rel = np.zeros(0), np.zeros((0, 0)), np.zeros(0)
    while Q.shape[1]:
        q = Q.shape[1]
        W = Op @ Q
        info["sweeps"] += 1
        info["solves"] += q
        V, OV = np.column_stack([V, Q]), np.column_stack([OV, W])
        m = V.shape[1]
        C = V.T @ W
        if not np.all(np.isfinite(C)):
            info["status"] = 3
            return np.full(nev, np.nan), None, info
        Gn = np.zeros((m, m))
        Gn[: m - q, : m - q] = G
        for c in range(q):
            j = m - q + c
            Gn[: j + 1, j] = C[: j + 1, c]
            Gn[j, : j + 1] = C[: j + 1, c]
        G = Gn
        theta, S = sort_ritz(*np.linalg.eigh(G))
        k = min(nev, m)
        rel = np.array([np.linalg.norm(OV @ S[:, j] - theta[j] * (V @ S[:, j])) / abs(theta[j]) for j in range(k)])
        ok = rel <= tol
        info["nconv"] = int(k if ok.all() else np.argmin(ok))
        if m == n:
            info["status"] = 2
            break
        if k == nev and info["nconv"] == nev:
            info["status"] = 0
            break
        Q = orth_block(W.copy())
        tries = 0
        while Q.shape[1] == 0 and tries < 4:
            info["fresh_blocks"] += 1
            Q = fresh()
            tries += 1
        if Q.shape[1] == 0:
            break
        if m + Q.shape[1] > mb:
            if info["restarts"] >= max_restarts:
                break
            keep = min(m, nev + block)
            V, OV = V @ S[:, :keep], OV @ S[:, :keep]
            G = np.diag(theta[:keep])
            info["restarts"] += 1
    k = min(nev, V.shape[1])
    lam = 1.0 / theta[:k]
    X = V @ S[:, :k]
    vecs = np.zeros((k, dim))
    for j in range(k):
        vecs[j] = finish(Finv[:, :n] @ X[:, j], n)
    if pencil:
        info["solves"] += k
    info["rel"] = rel
    return lam, vecs, info


# ---- the designs ---------------------------------------------------------------------------------------------------------------------
def kkt_block(n, seed):
    """A quasi-definite K of order n: the x-block (the leading ceil(3 n / 5) indices) positive definite, Sigma over six decades."""
    rng = np.random.default_rng(1000 * n + seed)
    nx = max(1, (3 * n + 4) // 5)
    m = n - nx
    h = 10.0 ** rng.uniform(-1.0, 1.0, size=nx)
    c = 0.3 * np.sqrt(h[:-1] * h[1:]) * rng.uniform(-1.0, 1.0, size=max(nx - 1, 0))
    H = sp.diags([h, c, c], [0, -1, 1]) if nx > 1 else sp.csc_matrix(np.array([[h[0]]]))
    if m == 0:
        return sp.csc_matrix(H), nx
    rows = np.repeat(np.arange(m), 3)
    cols = rng.integers(0, nx, size=3 * m)
    J = sp.csc_matrix((rng.normal(size=3 * m), (rows, cols)), shape=(m, nx))
    sigma = 10.0 ** rng.uniform(-3.0, 3.0, size=m)
    return sp.bmat([[H, J.T], [J, -sp.diags(1.0 / sigma)]], format="csc"), nx


def tiny_design(n=100):
    """A positive definite tridiagonal-plus matrix shifted until its smallest eigenvalue is 1e-12 of its norm."""
    K, _ = kkt_block(n, 7)
    H = K.toarray()
    H = np.abs(H) * np.sign(np.eye(n) - 0.5) * -1.0 + 2.0 * np.diag(np.abs(H).sum(axis=1))     # dominant: positive definite
    H = 0.5 * (H + H.T)
    w = np.linalg.eigvalsh(H)
    A = H - (w[0] - 1e-12 * w[-1]) * np.eye(n)
    return sp.csc_matrix(A), 0


def repeated_design():
    """Three copies of one block and three extra eigenvalues, well separated from the two innermost of the block."""
    B, _ = kkt_block(40, 3)
    w = np.linalg.eigvalsh(B.toarray())
    w = w[np.argsort(np.abs(w))]
    extra = sp.diags([abs(w[1]) * 3.0, -abs(w[1]) * 5.0, abs(w[1]) * 9.0])
    return sp.block_diag([B, B, B, extra], format="csc"), 0


def tree_design():
    """The small-front classes of the front_trees catalogue (order 372, mixed signs)."""
    roots = FT.DESIGNS["small-classes-f32-33-64-65-128-129"][0]
    b = FT.build(roots, values="plain", seed=0)
    return sp.csc_matrix(FT.full_csr(b.A)), 0


class Case:
    """One design with its options: F dense, A its lower triangle (CSC), the true spectrum and the gap behind |lambda_nev|."""

    def __init__(self, name, A, nlead, nev, block=4, max_basis=0, tol=1e-8, seed=1):
        A = sp.csc_matrix(A)
        self.F = A.toarray()
        self.F = 0.5 * (self.F + self.F.T)
        self.A = sp.csc_matrix(sp.tril(sp.csc_matrix(self.F)))
        self.A.sort_indices()
        self.dim = self.F.shape[0]
        self.pencil = 0 < nlead < self.dim
        self.nlead, self.n = nlead, (nlead if self.pencil else self.dim)
        self.nev, self.block, self.max_basis, self.tol, self.seed = nev, block, max_basis, tol, seed
        if self.pencil:
            k = nlead
            self.S = self.F[:k, :k] - self.F[:k, k:] @ np.linalg.solve(self.F[k:, k:], self.F[k:, :k])
            self.S = 0.5 * (self.S + self.S.T)
        else:
            self.S = self.F
        w, U = np.linalg.eigh(self.S)
        order = np.argsort(np.abs(w), kind="stable")
        self.w, self.U = w[order], U[:, order]
        self.gap = abs(self.w[nev]) / abs(self.w[nev - 1]) if nev < self.n else np.inf
        wF = np.linalg.eigvalsh(self.F)
        self.norm2 = float(np.max(np.abs(wF)))
        self.npos = int(np.sum(wF > 0))                      # the inertia the factorisation is asked for
        self.snorm2 = float(np.max(np.abs(self.w)))          # of the matrix eigh ran on (the Schur complement in pencil mode)
        self.name = name
        self.id = f"{name}-nev{nev}-b{block}-mb{max_basis}-gap{self.gap:.4g}"

    def opts(self):
        return dict(block=self.block, max_basis=self.max_basis, tol=self.tol, nlead=self.nlead, seed=self.seed)


def _first_with_gap(make):
    for seed in range(40):
        c = make(seed)
        if c.gap >= MIN_GAP:
            return c
    raise AssertionError("no seed gives the gap")


SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1029]
PENCIL_SIZES = [5, 65, 257, 1029]


@functools.lru_cache(maxsize=None)
def cases():
    """Every case the GPU tests run, by id."""
    out = []
    for n in SIZES:
        nev = min(n, 6 if n >= 63 else 3)
        out.append(_first_with_gap(lambda s, n=n, nev=nev: Case(f"kkt{n}", kkt_block(n, s)[0], 0, nev)))
    for n in PENCIL_SIZES:
        def make(s, n=n):
            K, nx = kkt_block(n, s)
            return Case(f"pencil{n}", K, nx, min(nx, 6 if n >= 63 else 2))
        out.append(_first_with_gap(make))
    # block widths below four, one eigenvalue, twelve eigenvalues
    out.append(_first_with_gap(lambda s: Case("kkt257", kkt_block(257, s)[0], 0, 1, block=1)))
    out.append(_first_with_gap(lambda s: Case("kkt257", kkt_block(257, s)[0], 0, 6, block=2)))
    out.append(_first_with_gap(lambda s: Case("kkt257", kkt_block(257, s)[0], 0, 12, block=3)))
    # the basis at its floor (restarts happen) and at its cap
    # (at the floor a restart leaves room for three blocks: the reference needs 5 to 7 restarts on these, 10 on kkt1029 with nev = 6)
    out.append(_first_with_gap(lambda s: Case("kkt257", kkt_block(257, s)[0], 0, 6, max_basis=24)))
    out.append(_first_with_gap(lambda s: Case("pencil257", kkt_block(257, s)[0], kkt_block(257, s)[1], 6, max_basis=24)))
    out.append(_first_with_gap(lambda s: Case("kkt1029", kkt_block(1029, s)[0], 0, 2, max_basis=16)))
    out.append(_first_with_gap(lambda s: Case("kkt1029", kkt_block(1029, s)[0], 0, 6, max_basis=128)))
    out.append(Case("tiny100", tiny_design()[0], 0, 1))
    out.append(Case("repeated3x40", repeated_design()[0], 0, 6))
    out.append(Case("tree372", tree_design()[0], 0, 4))
    for c in out:
        assert c.gap >= MIN_GAP, c.id
    return {c.id: c for c in out}
