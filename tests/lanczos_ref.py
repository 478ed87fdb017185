"""NumPy / SciPy restatement of what okkt_kkt_min_eig and okkt_kkt_ipopt_strategy_eig promise, and the designed
systems of tests/test_gpu_delta_eig.py.  No GPU and no library call in here.

  dense_q(it)            Q(0) = H_sym + J' diag(y ./ s) J as a dense double matrix (H is stored as its lower triangle)
  scaled_q(Q, sd)        D Q D with d_i = 1 / sqrt(|sd_i|), 1 where sd_i is 0 or not finite
  rayleigh_ld(it, v)     (rho, resid, rho_abs, |Q||v| norm) of v in long double
  delta_sequence(...)    the attempts of ipopt_strategy! (delta_strategy.jl:37-114) as a list of (delta, eligible): eligible attempts are
                         the ones after the first failed attempt, i.e. the ones a Lanczos bound could skip
  exact_skips(...)       how many attempts an exact lambda_min would skip
"""
import math

import numpy as np
import scipy.sparse as sp

LD = np.longdouble


def _parts(it):
    Hl = sp.csc_matrix(it.H).toarray()
    Hs = Hl + Hl.T - np.diag(np.diag(Hl))
    J = sp.csc_matrix(it.J).toarray().reshape(len(it.s), len(it.x))
    return Hs, J


def dense_q(it):
    Hs, J = _parts(it)
    sig = np.asarray(it.y, float) / np.asarray(it.s, float)
    return Hs + J.T @ (sig[:, None] * J)


def scaling_vector(sd):
    sd = np.asarray(sd, float)
    d = np.ones_like(sd)
    ok = np.isfinite(sd) & (sd != 0.0)
    d[ok] = 1.0 / np.sqrt(np.abs(sd[ok]))
    return d


def scaled_q(Q, sd):
    d = scaling_vector(sd)
    return d[:, None] * Q * d[None, :]


def rayleigh_ld(it, v):
    """Long double: rho = v'Qv / v'v, resid = ||Qv - rho v|| / ||v||, rho_abs = (|v|'|H||v| + sum sigma (|J||v|)^2) / v'v and
    || |Q| |v| ||_2 / ||v||_2 with |Q| = |H| + |J|' Sigma |J| (the scale of the rounding of Q v)."""
    Hs, J = _parts(it)
    Hs, J, v = Hs.astype(LD), J.astype(LD), np.asarray(v).astype(LD)
    sig = np.asarray(it.y).astype(LD) / np.asarray(it.s).astype(LD)
    vv = v @ v
    Jv = J @ v
    qv = Hs @ v + J.T @ (sig * Jv)
    rho = (v @ qv) / vv
    resid = np.sqrt(((qv - rho * v) ** 2).sum() / vv)
    av = np.abs(v)
    aJv = np.abs(J) @ av
    aq = np.abs(Hs) @ av + np.abs(J).T @ (sig * aJv)
    rho_abs = (av @ aq) / vv
    return float(rho), float(resid), float(rho_abs), float(np.sqrt((aq ** 2).sum() / vv))


def delta_sequence(diag_min, delta_prev, d, count=80):
    """[(delta, eligible)]: the attempts of ipopt_strategy! in order, as long as every one fails, `count` loop attempts at most.  d has
    start, min, inc, dec, zero (Class_delta_parameters).  The first attempt is never eligible: Lanczos runs after it has failed."""
    out = []
    tau = 1.5 * diag_min
    if tau > 0.0:
        tau = 0.0
        out.append((d.zero, False))
    delta = d.zero
    for i in range(1, count + 1):
        if i == 1:
            delta = max(d.min - tau, delta_prev * d.dec) if delta_prev != 0.0 else d.start - tau
        else:
            delta = delta * d.inc
        out.append((delta, len(out) > 0))
    return out


def exact_skips(seq, lam_min, delta_max):
    """The eligible attempts before the first one that succeeds (delta > -lam_min) that an exact lam_min certifies to fail."""
    n = 0
    for delta, eligible in seq:
        if delta > -lam_min:
            break
        if eligible and delta <= delta_max:
            n += 1
    return n


def attempts_until_success(seq, lam_min):
    n = 0
    for delta, _ in seq:
        n += 1
        if delta > -lam_min:
            return n, delta
    raise AssertionError("the sequence never passes -lam_min")


def margin_from_grid(seq, lam_min):
    """min over the sequence of |delta_i / (-lam_min) - 1|: the tests require 0.1 at least (no attempt within 10 % of -lam_min)."""
    return min(abs(delta / (-lam_min) - 1.0) for delta, _ in seq if delta != 0.0)


# ---- designed systems ---------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257)     # lpr - 1, lpr, lpr + 1 for every lanes-per-row


def _iterate(Iterate, H, J, s, y, rng):
    m, n = J.shape
    return Iterate(x=np.zeros(n), y=y, s=s, mu=0.1, J=J, H=H, grad=rng.normal(size=n), cons=rng.normal(size=m))


def _lower(n, rng, density, empty_col):
    """A lower-triangular pattern with a full diagonal except column `empty_col`, which is empty, and (n > 2) random entries below."""
    rows, cols, vals = [], [], []
    for j in range(n):
        if j == empty_col:
            continue
        rows.append(j); cols.append(j); vals.append(rng.uniform(-2.0, 3.0))
        for i in range(j + 1, n):
            if i != empty_col and rng.random() < density:
                rows.append(i); cols.append(j); vals.append(rng.normal())
    H = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    H.sum_duplicates()
    return H


def operator_design(Iterate, n, variant, seed=0):
    """variant: 'full' (H with an empty column, J with rows of every edge length, one full row, an empty column, sigma from 1e-8 to
    1e8), 'm0' (no constraints), 'h0' (nnz(H) = 0)."""
    rng = np.random.default_rng(1000 * n + seed)
    empty_col = n - 1 if n > 2 else -1
    H = sp.csc_matrix((n, n)) if variant == "h0" else _lower(n, rng, min(1.0, 3.0 / n), empty_col)
    if variant == "m0":
        J = sp.csc_matrix((0, n))
    else:
        lens = sorted({min(v, n) for v in ROW_LENGTHS} | {n})
        lens += [min(3, n)] * max(0, min(n, 40) - len(lens))          # a tail of ordinary rows
        jempty = 0 if n > 2 else -1                                   # an empty column of J (the full row skips it too: n - 1 entries)
        rows, cols, vals = [], [], []
        avail = np.array([c for c in range(n) if c != jempty])
        for i, ln in enumerate(lens):
            ln = min(ln, len(avail))
            for c in np.sort(rng.choice(avail, size=ln, replace=False)):
                rows.append(i); cols.append(int(c)); vals.append(rng.normal())
        J = sp.csc_matrix((vals, (rows, cols)), shape=(len(lens), n))
        J.sum_duplicates()
    m = J.shape[0]
    sig = 10.0 ** np.linspace(-8.0, 8.0, m) if m else np.zeros(0)
    rng.shuffle(sig)
    return _iterate(Iterate, H, J, np.ones(m), sig, rng)


def indefinite_design(Iterate, n, lam, seed=0, cluster=1):
    """Q(0) with positive diagonal and `cluster` lowest eigenvalues near lam < 0 (cluster = 1: lam itself, isolated): coordinates
    (2c, 2c + 1) carry the block [[1, b_c], [b_c, 1]] with 1 - b_c = lam (1 + 1e-3 c) and touch nothing else; the other coordinates
    carry a spread diagonal in [1, 4] with a weak sparse coupling plus J' Sigma J of three-entry rows, sigma in [0.5, 2]: positive
    definite with its spectrum above 0.5."""
    rng = np.random.default_rng(7 * n + seed)
    nb = 2 * cluster
    assert n >= nb
    rows, cols, vals = [], [], []
    for c in range(cluster):
        b = 1.0 - lam * (1.0 + 1e-3 * c)
        rows += [2 * c, 2 * c + 1, 2 * c + 1]; cols += [2 * c, 2 * c, 2 * c + 1]; vals += [1.0, b, 1.0]
    rest = np.arange(nb, n)
    for j in rest:
        rows.append(j); cols.append(j); vals.append(rng.uniform(1.0, 4.0))
        if j + 3 < n and rng.random() < 0.5:
            rows.append(j + 3); cols.append(j); vals.append(rng.uniform(-0.1, 0.1))
    H = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    H.sum_duplicates()
    m = len(rest) // 2
    jr, jc, jv = [], [], []
    for i in range(m):
        for c in np.sort(rng.choice(rest, size=min(3, len(rest)), replace=False)):
            jr.append(i); jc.append(int(c)); jv.append(rng.uniform(-0.5, 0.5))
    J = sp.csc_matrix((jv, (jr, jc)), shape=(m, n))
    J.sum_duplicates()
    y = rng.uniform(0.5, 2.0, size=m)
    return _iterate(Iterate, H, J, np.ones(m), y, rng)


def convex_design(Iterate, n, seed=0):
    rng = np.random.default_rng(11 * n + seed)
    H = sp.diags(rng.uniform(1.0, 4.0, size=n), format="csc")
    m = n // 2
    J = sp.random(m, n, density=min(1.0, 3.0 / n), random_state=np.random.RandomState(seed), format="csc")
    return _iterate(Iterate, H, J, np.ones(m), rng.uniform(0.5, 2.0, size=m), rng)


def pick_lpr(nnz, rows):
    """The lanes-per-row rule of okkt_kkt_set_structure (csrc/kkt.hip)."""
    avg = nnz / rows if rows > 0 else 1.0
    return 4 if avg <= 5.0 else 8 if avg <= 10.0 else 16 if avg <= 24.0 else 32 if avg <= 56.0 else 64


def numpy_lanczos(Q, steps, start):
    """Lanczos with full reorthogonalisation on the dense Q: (theta_min, Ritz vector) after `steps` steps (CPU planning aid)."""
    n = Q.shape[0]
    V = np.zeros((n, 0))
    v = start / np.linalg.norm(start)
    al, be = [], []
    for _ in range(min(steps, n)):
        V = np.column_stack([V, v])
        w = Q @ v
        for _ in range(2):
            w = w - V @ (V.T @ w)
        al.append(v @ Q @ v)
        b = np.linalg.norm(w)
        if b <= 2.0 ** -44 * max(abs(a) for a in al):
            break
        be.append(b)
        v = w / b
    k = len(al)
    T = np.diag(al) + np.diag(be[: k - 1], 1) + np.diag(be[: k - 1], -1)
    w, S = np.linalg.eigh(T)
    return w[0], V[:, :k] @ S[:, 0]
