"""Designed inputs of the KKT layer (csrc/kkt.hip): seeded (H lower, J, s, y) whose shapes put every launch route of the assembly and
of the segmented row kernels to work.  Each design says which route and which edge it exists for; `routes` restates the rules that
pick the routes, so tests/test_kkt_designs.py can check that every design still lands where it claims (host only).

Values: magnitudes in [0.5, 2] with random signs, s and y in [0.2, 5] -- every term of every sum is then far above the rounding
bound of kkt_exact, so a dropped or doubled term cannot pass a check."""
import math
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp


# ---- the rules of okkt_kkt_set_structure, restated -----------------------------------------------------------------------------
def pick_lpr(nnz, rows):
    """Lanes per row of the segmented products (kkt.hip, pick_lpr)."""
    avg = nnz / rows if rows > 0 else 1.0
    return 4 if avg <= 5.0 else (8 if avg <= 10.0 else (16 if avg <= 24.0 else (32 if avg <= 56.0 else 64)))


def schur_groups(maxcol, cap=16):
    """Column groups per workgroup of k_assemble_schur_lds (0: the contribution-list kernel k_assemble_schur), kkt.hip
    okkt_kkt_set_structure: G from the longest column of Q, capped by OKKT_SCHUR_GROUPS."""
    g = 16 if maxcol <= 512 else (8 if maxcol <= 1024 else (4 if maxcol <= 2048 else 0))
    return min(g, cap)


def dense_rows(J, opt):
    """Rows of J that border the Schur system (okkt_opts.schur_dense_rows: 0 off, > 0 threshold, -1 max(64, 10 sqrt(n)))."""
    if opt == 0:
        return np.zeros(0, dtype=np.int64)
    n = J.shape[1]
    thr = float(opt) if opt > 0 else max(64.0, 10.0 * math.sqrt(n))
    return np.nonzero(np.diff(J.tocsr().indptr) > thr)[0].astype(np.int64)


def q_pattern(H, J, drows):
    """Lower pattern of Q_s = J_s' S J_s + H with its diagonal (boolean CSC, sorted) and, per column, the border entries of the
    dense rows: the layout okkt_kkt_set_structure gives the Schur kinds."""
    n = J.shape[1]
    keep = np.ones(J.shape[0], bool)
    keep[drows] = False
    Js = abs(J.tocsr()[keep]).astype(bool).astype(np.int64)
    P = sp.tril(Js.T @ Js + abs(H).astype(bool).astype(np.int64) + sp.identity(n, dtype=np.int64, format="csc")).tocsc()
    P.sort_indices()
    nb = np.asarray(abs(J.tocsr()[drows]).astype(bool).sum(axis=0)).ravel() if len(drows) else np.zeros(n, np.int64)
    return P, nb


def routes(d):
    """Where okkt_kkt_set_structure sends design d: longest column of Q (border included), G, lanes per row of the three families."""
    drows = dense_rows(d.J, d.dense)
    P, nb = q_pattern(d.H, d.J, drows)
    maxcol = int(max(1, (np.diff(P.indptr) + nb).max())) if d.n else 1
    return dict(maxcol=maxcol, G=schur_groups(maxcol), kd=len(drows), lprJr=pick_lpr(d.J.nnz, d.m), lprJc=pick_lpr(d.J.nnz, d.n),
                lprH=pick_lpr(d.H.nnz, d.n))


# ---- designs -----------------------------------------------------------------------------------------------------------------
@dataclass
class Design:
    name: str
    why: str
    H: sp.csc_matrix          # n x n, lower triangle
    J: sp.csc_matrix          # m x n
    s: np.ndarray
    y: np.ndarray
    dense: int = 0            # okkt_opts.schur_dense_rows for the Schur kinds
    expect: dict = field(default_factory=dict)   # what routes(d) must give
    factor: bool = True       # directions are computed (False: the matrices only)

    @property
    def n(self):
        return self.J.shape[1]

    @property
    def m(self):
        return self.J.shape[0]


def _vals(rng, k):
    return rng.uniform(0.5, 2.0, size=k) * rng.choice([-1.0, 1.0], size=k)


def _from_rows(rng, n, rows):
    """J (m x n CSC, canonical) from the column lists of its rows."""
    m = len(rows)
    ri = np.concatenate([np.full(len(c), i, np.int64) for i, c in enumerate(rows)] + [np.zeros(0, np.int64)])
    ci = np.concatenate([np.asarray(c, np.int64) for c in rows] + [np.zeros(0, np.int64)])
    J = sp.csc_matrix((_vals(rng, len(ri)), (ri, ci)), shape=(m, n))
    J.sum_duplicates()
    return J


def _h(rng, n, per_col, no_diag=0.2, extra=()):
    """Lower-triangular H with about per_col entries per column: the diagonal (missing on a fraction no_diag of the columns) and
    random rows below it; `extra`: (row, col) entries to add."""
    ri, ci = [], []
    for j in range(n):
        below = n - j - 1
        k = min(below, max(0, int(round(rng.uniform(0.5, 1.5) * per_col)) - 1))
        rows = list(j + 1 + rng.choice(below, size=k, replace=False)) if k else []
        if rng.random() >= no_diag:
            rows.append(j)
        ri += rows
        ci += [j] * len(rows)
    for a, b in extra:
        ri.append(max(a, b)); ci.append(min(a, b))
    H = sp.csc_matrix((np.ones(len(ri)), (np.asarray(ri, np.int64), np.asarray(ci, np.int64))), shape=(n, n))
    H.sum_duplicates()
    H.data = _vals(rng, H.nnz)
    return H


def _sy(rng, m):
    return rng.uniform(0.2, 5.0, size=m), rng.uniform(0.2, 5.0, size=m)


def _random_rows(rng, n, m, r, empty_rows=0, lens=None):
    """m rows of about r distinct columns each (lens: explicit lengths), the last `empty_rows` of them empty."""
    rows = []
    for i in range(m):
        k = lens[i] if lens is not None else int(np.clip(round(rng.uniform(0.6, 1.4) * r), 1, n))
        rows.append(np.sort(rng.choice(n, size=k, replace=False)) if i < m - empty_rows else [])
    return rows


def star(L, seed, n_extra=3, border=0, dense=0):
    """The longest column of Q at exactly L entries from a 'star': column 0 in short rows that each hold 3 - 5 distinct higher
    columns (1 .. L-1 once each), so a row gives 10 - 20 terms.  Extra columns: one empty, two in short rows of their own; one
    empty row; H entries (a, 0) in a few star columns (J and H terms in one slot).  border > 0: that many dense rows of 300
    columns, column 0 among them, bordering the system (dense > 0 is their threshold)."""
    rng = np.random.default_rng(seed)
    n = L + n_extra
    rows, c = [], 1
    while c < L:
        k = min(int(rng.integers(3, 6)), L - c)
        rows.append([0] + list(range(c, c + k)))
        c += k
    rows += [[L, L + 1], [L + 1], []]
    for _ in range(border):
        rows.append(np.unique(np.concatenate([[0], rng.choice(np.arange(1, L), size=299, replace=False)])))
    J = _from_rows(rng, n, rows)
    H = _h(rng, n, 1.5, extra=[(a, 0) for a in rng.choice(np.arange(1, L), size=max(1, L // 20), replace=False)])
    s, y = _sy(rng, J.shape[0])
    return J, H, s, y


def _design_list():
    out = []

    def add(name, why, J, H, s, y, dense=0, factor=True, **expect):
        out.append(Design(name, why, H.tocsc(), J.tocsc(), s, y, dense, expect, factor))

    # -- the four Schur assembly routes, at both sides of every boundary of the G rule
    for L, G in ((512, 16), (513, 8), (1024, 8), (1025, 4), (2048, 4), (2049, 0)):
        J, H, s, y = star(L, seed=L)
        add(f"star{L}", f"longest column of Q = {L}: G = {G}", J, H, s, y, maxcol=L, G=G)
    J, H, s, y = star(512, seed=7, border=1)
    add("border513", "Q_s has a column of 512, the border entry of a dense row makes it 513: G = 8", J, H, s, y, dense=200,
        maxcol=513, G=8, kd=1)
    rng = np.random.default_rng(21)
    n = 2140
    rows = [np.arange(2100)] + [np.arange(c, min(c + 4, n)) for c in range(2100, n, 4)]     # disjoint: one J term per entry of Q
    J = _from_rows(rng, n, rows)
    H = _h(rng, n, 1.2, extra=[(a, b) for a, b in rng.choice(2100, size=(40, 2))])
    add("long_row", "one J row of 2100 entries, dense rows off: the contribution-list kernel is the only route", J, H, *_sy(rng, J.shape[0]),
        factor=False, maxcol=2100, G=0)
    # -- the bordered system
    rng = np.random.default_rng(22)
    n, m = 300, 160
    rows = _random_rows(rng, n, m, 5) + [np.sort(rng.choice(n, size=k, replace=False)) for k in (200, 240, 281)]
    J = _from_rows(rng, n, rows)
    add("border3", "three dense rows (automatic threshold) border Q_s", J, _h(rng, n, 4), *_sy(rng, J.shape[0]), dense=-1, kd=3)

    # -- lanes per row: every band of every family, counts that are not multiples of 256 / LPR, empty rows and columns
    def band(name, why, n, m, r, h, seed, empty_rows=0, empty_cols=0, no_diag=0.2, **expect):
        rng = np.random.default_rng(seed)
        live = np.sort(rng.choice(n, size=n - empty_cols, replace=False))
        rows = [live[c] for c in _random_rows(rng, n - empty_cols, m, r, empty_rows)]
        J = _from_rows(rng, n, rows)
        H = _h(rng, n, h, no_diag=no_diag) if h else sp.csc_matrix((n, n))
        add(name, why, J, H, *_sy(rng, m), **expect)

    band("b4", "4 lanes everywhere; 7 empty rows, 11 empty columns", 301, 130, 3.5, 3, 31, empty_rows=7, empty_cols=11,
         lprJr=4, lprJc=4, lprH=4)
    band("b8", "8 lanes everywhere; empty rows and columns", 203, 211, 8, 7, 32, empty_rows=3, empty_cols=5, lprJr=8, lprJc=8, lprH=8)
    band("b16", "16 lanes everywhere", 157, 141, 18, 15, 33, empty_rows=2, empty_cols=2, lprJr=16, lprJc=16, lprH=16)
    band("b32", "32 lanes everywhere", 131, 97, 40, 40, 34, empty_cols=1, lprJr=32, lprJc=32, lprH=32)
    band("b64", "64 lanes over the rows of J and the columns of H (n = 170: the last workgroup holds 2 of 4 rows)", 170, 60, 80, 75, 35,
         lprJr=64, lprJc=32, lprH=64)
    band("jc64", "64 lanes over the columns of J (n = 37)", 37, 400, 6, 2, 36, lprJr=8, lprJc=64, lprH=4)
    band("h_empty", "nnz(H) = 0", 90, 70, 6, 0, 37, lprJr=8, lprJc=4, lprH=4)
    band("h_nodiag", "no H column has its diagonal", 120, 90, 4, 3, 38, no_diag=1.0, lprJr=4, lprJc=4, lprH=4)
    # one partial workgroup: n or m below 256 / LPR
    band("tiny8", "m = 17 < 32, n = 20 < 32 at 8 lanes", 20, 17, 8, 7, 41, no_diag=0.3, lprJr=8, lprJc=8, lprH=8)
    band("tiny16", "m = 13 < 16, n = 15 < 16 at 16 lanes", 15, 13, 12, 3, 42, lprJr=16, lprJc=16)
    band("tiny32r", "m = 7 < 8 at 32 lanes over the rows", 60, 7, 40, 3, 43, lprJr=32, lprJc=8)
    band("tiny32c", "n = 7 < 8 at 32 lanes over the columns", 7, 50, 5, 2, 44, lprJr=4, lprJc=32)
    rng = np.random.default_rng(45)
    J = _from_rows(rng, 250, [np.sort(rng.choice(250, size=120, replace=False)), [], np.sort(rng.choice(250, size=200, replace=False))])
    add("jr64_tiny", "m = 3 < 4 at 64 lanes over the rows, one of them empty", J, _h(rng, 250, 2), *_sy(rng, 3), lprJr=64, lprJc=4)
    rng = np.random.default_rng(46)
    J = _from_rows(rng, 3, [np.sort(rng.choice(3, size=int(rng.integers(2, 4)), replace=False)) for _ in range(300)])
    H = sp.csc_matrix(np.tril(np.ones((3, 3))))
    H.data = _vals(rng, H.nnz)
    add("jc64_tiny", "n = 3 < 4 at 64 lanes over the columns", J, H, *_sy(rng, 300), lprJr=4, lprJc=64, lprH=4)
    rng = np.random.default_rng(47)
    J = sp.csc_matrix(np.array([[_vals(rng, 1)[0]]]))
    H = sp.csc_matrix(np.array([[_vals(rng, 1)[0]]]))
    add("n1m1", "n = 1, m = 1", J, H, *_sy(rng, 1), lprJr=4, lprJc=4, lprH=4)
    rng = np.random.default_rng(48)
    add("m0", "m = 0: Q = H", sp.csc_matrix((0, 40)), _h(rng, 40, 3), np.zeros(0), np.zeros(0), lprJc=4)
    rng = np.random.default_rng(49)
    rows = _random_rows(rng, 400, 200, 3, lens=[2] * 120 + [360] + [3] * 79)
    for i in range(0, 150):
        rows[i] = np.unique(np.concatenate([rows[i], [0]]))
    J = _from_rows(rng, 400, rows)
    add("outlier", "one row 100 times longer than the others, one column in 150 of 200 rows", J, _h(rng, 400, 3), *_sy(rng, 200),
        lprJr=4, lprJc=4)
    return out


DESIGNS = {d.name: d for d in _design_list()}


def shift(d):
    """A delta that makes Q + delta I (H + delta I for the symmetric kind) positive definite: 1 + the largest absolute row sum of
    the symmetric H (J' S J is semidefinite)."""
    if d.n == 0 or d.H.nnz == 0:
        return 1.0
    Hs = abs(d.H) + abs(sp.tril(d.H, -1)).T
    return 1.0 + float(np.asarray(Hs.sum(axis=1)).max())


def point(d, seed=0):
    """x, grad, cons, mu of an iterate at design d (s, y its own)."""
    rng = np.random.default_rng(seed + 1000)
    return dict(x=rng.normal(size=d.n), grad=_vals(rng, d.n), cons=d.s + 0.5 * _vals(rng, d.m), mu=0.1)


def moved(d, seed=0, last=0.0):
    """A current iterate different from the factor iterate (one_phase.jl:262-279): new Jacobian values, s, y.  last > 0: the last
    column of J moves by that fraction, the last row by ten times it, s and y of the last row by factors 3 and 1/3 (the residual of
    the direct kind's N err peaks there)."""
    rng = np.random.default_rng(seed + 2000)
    J2 = d.J.copy()
    J2.data = J2.data * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=J2.nnz))
    s2, y2 = d.s * rng.uniform(0.7, 1.4, size=d.m), d.y * rng.uniform(0.7, 1.4, size=d.m)
    if last and d.m:
        J2 = J2.tolil()
        J2[:, d.n - 1] = J2[:, d.n - 1] * (1.0 + last)
        J2[d.m - 1, :] = J2[d.m - 1, :] * (1.0 + 10.0 * last)
        J2 = J2.tocsc()
        J2.sort_indices()
        s2[-1] *= 3.0
        y2[-1] /= 3.0
    return J2, s2, y2


# ---- designs of the clever-symmetric kind: rows of J that are exact multiples of each other -------------------------------------
@dataclass
class CleverDesign(Design):
    """A Design plus what compute_indicies (clever_symmetric.jl:200-260) has to find in its J: groups = [(members in ls order,
    their ratios to the leader)], sorted by leader (= members[0], the group's first row in the sorted order of the rescaled rows)."""
    groups: list = field(default_factory=list)

    @property
    def m_new(self):
        return len(self.groups)


def _three_pair(rng, k):
    """Values v of a k-entry row such that the rows v and 3 v (a) differ after rescaling by their first value, so the sort -- not
    the row number -- decides which of them leads, and (b) still merge under columns_are_same's 1e-16 test (clever_symmetric.jl:63-88,
    107-155 restated; tests/test_kkt_clever_designs.py pins what the oracle itself decides).  Returns (v, 3 v, True if 3 v leads)."""
    for _ in range(10000):
        a = _vals(rng, k)
        b = 3.0 * a
        ra, rb = a / a[0], b / b[0]
        if np.array_equal(ra, rb):
            continue
        p = int(np.nonzero(ra != rb)[0][0])
        three_leads = bool(rb[p] < ra[p])
        lead, other = (b, a) if three_leads else (a, b)
        if np.sqrt(np.sum((lead - other * (lead[0] / other[0])) ** 2)) < 1e-16:
            return a, b, three_leads
    raise AssertionError("no merging ratio-3 pair found")


def clever_family(name, why, n, seed, singles=0, pow2=(), three=0, near=0, pattern=0, empty=0, empty_cols=0, h=3.0, no_diag=0.2, r=4):
    """A clever design from families of rows, scattered through the row order by a random permutation:
    singles: rows of their own; pow2: one group per entry, its members the given power-of-two multiples (both signs) of one base row
    -- their rescaled rows are bitwise equal, the lowest row leads; three: pairs (v, 3 v) whose leader is the HIGHER row (_three_pair);
    near: pairs (v, v with one entry off by a relative 1e-12) that must not merge; pattern: pairs with one pattern and unrelated
    values; empty: empty rows (one group).  Every non-empty row has at least two entries and every family a pattern of its own."""
    rng = np.random.default_rng(seed)
    live = np.sort(rng.choice(n, size=n - empty_cols, replace=False))
    seen = set()

    def pat():
        while True:
            k = int(np.clip(round(rng.uniform(0.6, 1.4) * r), 2, len(live)))
            c = tuple(np.sort(rng.choice(live, size=k, replace=False)))
            if c not in seen:
                seen.add(c)
                return np.array(c, np.int64)

    rows, fams = [], []           # rows: (cols, vals); fams: [(row ids of a family, kind, data)]
    for _ in range(singles):
        c = pat(); rows.append((c, _vals(rng, len(c)))); fams.append(([len(rows) - 1], "group", [1.0]))
    for fac in pow2:
        c = pat(); v = _vals(rng, len(c))
        ids = []
        for f in fac:
            rows.append((c, f * v)); ids.append(len(rows) - 1)
        fams.append((ids, "group", list(fac)))
    for _ in range(three):
        c = pat(); a, b, three_leads = _three_pair(rng, 2)
        c = c[:2]
        rows.append((c, a)); rows.append((c, b))
        fams.append(([len(rows) - 2, len(rows) - 1], "three", three_leads))
    for _ in range(near):
        c = pat(); v = _vals(rng, len(c)); w = v.copy(); w[-1] *= 1.0 + 1e-12
        rows.append((c, v)); rows.append((c, 2.0 * w))
        fams.append(([len(rows) - 2], "group", [1.0])); fams.append(([len(rows) - 1], "group", [1.0]))
    for _ in range(pattern):
        c = pat()
        for _ in range(2):
            rows.append((c, _vals(rng, len(c)))); fams.append(([len(rows) - 1], "group", [1.0]))
    ids = []
    for _ in range(empty):
        rows.append((np.zeros(0, np.int64), np.zeros(0))); ids.append(len(rows) - 1)
    if ids:
        fams.append((ids, "group", [1.0] * len(ids)))
    m = len(rows)
    place = rng.permutation(m)                      # row t of the list above becomes row place[t] of J
    groups = []
    for ids, kind, data in fams:
        at = [int(place[t]) for t in ids]
        if kind == "three":                         # the leader takes the higher of the two places
            lead = 1 if data else 0
            hi, lo = max(at), min(at)
            place[ids[lead]], place[ids[1 - lead]] = hi, lo
            vl, vo = rows[ids[lead]][1], rows[ids[1 - lead]][1]
            groups.append(([hi, lo], [1.0, float(vo[0] / vl[0])]))
        else:
            order = np.argsort(at)                  # equal rescaled rows: the sort falls back on the row number
            groups.append(([at[i] for i in order], [float(data[i] / data[order[0]]) for i in order]))
    groups.sort(key=lambda g: g[0][0])
    ri = np.concatenate([np.full(len(c), place[t], np.int64) for t, (c, _) in enumerate(rows)] + [np.zeros(0, np.int64)])
    ci = np.concatenate([c for c, _ in rows] + [np.zeros(0, np.int64)])
    vv = np.concatenate([v for _, v in rows] + [np.zeros(0)])
    J = sp.csc_matrix((vv, (ri, ci)), shape=(m, n))
    J.sum_duplicates()
    H = _h(rng, n, h, no_diag=no_diag) if h else sp.csc_matrix((n, n))
    s, y = _sy(rng, m)
    return CleverDesign(name, why, H.tocsc(), J, s, y, groups=groups)


def singleton_groups(d):
    """The grouping of a design whose non-empty rows are pairwise non-parallel: every row its own group, the empty rows one group led
    by the lowest of them."""
    empty = [int(i) for i in np.nonzero(np.diff(d.J.tocsr().indptr) == 0)[0]]
    g = [([i], [1.0]) for i in range(d.m) if i not in set(empty)]
    if empty:
        g.append((empty, [1.0] * len(empty)))
    return sorted(g, key=lambda t: t[0][0])


def _clever_list():
    P = lambda *e: tuple(2.0 ** k * sg for k, sg in e)     # (exponent, sign) -> factor
    out = [
        clever_family("cg_mix", "groups of 1, 2, 3, 5 and 7 scattered through 293 rows, both signs, a ratio-3 pair led by its higher row, a "
                      "near-parallel pair, a same-pattern pair, 5 empty rows, 7 empty columns; m_new = 210 < 256 < m", 211, 61, singles=150,
                      pow2=[P((0, 1), (e, sg)) for e, sg in zip([1, -1, 2, -3, 5, -6, 10, -10] * 5, [1, -1] * 20)]
                      + [P((0, 1), (1, -1), (-2, 1)), P((0, -1), (3, 1), (-1, -1)), P((2, 1), (0, 1), (-2, -1))] * 3 + [P((1, 1), (0, -1), (4, 1))]
                      + [P((0, 1), (1, 1), (-1, -1), (2, -1), (-3, 1))] * 3 + [P((0, 1), (-1, -1), (1, 1), (-2, 1), (2, -1), (3, 1), (-4, -1))],
                      three=1, near=1, pattern=1, empty=5, empty_cols=7, h=3.0, no_diag=0.3),
        clever_family("cg_big", "m_new = 283 > 256 (two workgroups of groups, the second partial), no H column has its diagonal", 150, 62,
                      singles=240, pow2=[P((0, 1), (1, -1))] * 15 + [P((-1, 1), (2, 1))] * 15 + [P((0, -1), (1, 1), (-1, 1))] * 10
                      + [P((0, 1), (1, -1), (2, 1), (-1, -1), (-2, 1), (3, -1))] * 2, empty=3, h=3.0, no_diag=1.0, r=5),
        clever_family("cg_h0", "nnz(H) = 0", 60, 63, singles=20, pow2=[P((0, 1), (-1, -1))] * 5 + [P((1, 1), (0, -1), (-1, 1))] * 2
                      + [P((0, 1), (1, 1), (2, -1), (-1, 1), (-2, -1))], empty=2, empty_cols=3, h=0),
    ]
    rng = np.random.default_rng(64)
    a = _vals(rng, 1)[0]
    out.append(CleverDesign("cg_n1m2", "n = 1, m = 2, the two rows parallel: m_new = 1", sp.csc_matrix(np.array([[_vals(rng, 1)[0]]])),
                            sp.csc_matrix(np.array([[a], [-2.0 * a]])), *_sy(rng, 2), groups=[([0, 1], [1.0, -2.0])]))
    # the existing designs, as they are: random rows, so every group is a singleton (the empty rows of b8 merge); m = 0
    for name in ("b8", "b64", "jc64_tiny", "m0"):
        d = DESIGNS[name]
        out.append(CleverDesign(name, d.why, d.H, d.J, d.s, d.y, groups=singleton_groups(d)))
    return out


CLEVER_DESIGNS = {d.name: d for d in _clever_list()}
RESCALES = ("none", "u_only", "u_and_x")
