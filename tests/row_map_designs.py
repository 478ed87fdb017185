"""Designed inputs of the row-map kernels (csrc/refine.hip k_resid_*, csrc/scaling.hip k_scale_*, csrc/condest.hip k_cd_rowsum_*;
DESIGN.md section 5) at the edges of the partition they share.  No GPU and no library call in here; test_row_map_designs_host.py checks
what is claimed below, test_gpu_row_map_edges.py runs the kernels on it.

The partition, restated from refine_map_build: the full symmetric rows of the lower CSC input (upper entries ignored, a pair listed more
than once summed in input order from 0), nnz entries in n rows; lpr = pick_lanes(nnz, n) lanes per short row; long_min = max(256, 8 lpr);
a row of more than long_min entries is long and takes a workgroup of 256 threads (entry p on thread (p - p0) mod 256, wave thread / 64); the
others take lpr lanes each (entry p on lane (p - p0) mod lpr), g = 256 / lpr rows per workgroup, nb_short = ceil(n lpr / 256) workgroups,
threads past row n - 1 clamped to it; the partials of the long rows stand behind the nb_short short ones and one workgroup of 256 threads
folds them all, partial i on thread i mod 256.

A pattern is a band of half-width w (BAND_W picks the lpr), rows of prescribed length ("arrow" rows, filled with evenly spread columns, and
short rows cut or filled to length) and optionally empty rows.  The rows of prescribed length never neighbour each other, so every
length is exact.  catalogue() names the designs:
  lpr{4,8,16,32,64}-full / -one   n = 0 / 1 (mod g): the last workgroup full / owning one row with 255 threads clamped.  Arrow rows of
                                  long_min - 1, long_min, long_min + 1 and 2 * 256 + 1 entries (long_min + 256 + 1 for lpr 64: 769), one of
                                  them row n - 1, one the first row of a workgroup; short rows of 1, lpr - 1, lpr, lpr + 1, 2 lpr + 1.
  lpr8-dups                       lpr8-full with pairs of the arrow rows listed twice, upper-triangle entries that nobody may read and
                                  the rows of every column in descending order (ndup > 0 on the long route)
  lpr8-empty                      lpr8-one with an empty row (no diagonal, no entries) in its last full workgroup: residual only
  lpr16-nodiag                    lpr16-full whose 513-entry row stores no diagonal (condest's `hasd` branch); that row is ordered last
  zero-last                       tridiagonal, n = 129: row 128, alone in the last workgroup, holds only a stored 0.0
  avg{5,10,24,56}-on / -over      the smallest band-like patterns with nnz / n exactly on a boundary of pick_lanes and one off-diagonal
                                  pair above it (n = 8, 16, 32 and, because nnz / n <= n, 64 for the boundary 56)
  n1, n2-empty                    one row; two rows of which the second is empty (residual only)
  tridiag-16385                   lpr 4, nb_short = 257: row 16384 is alone in workgroup 256, the one partial the final kernels of
                                  refine.hip and condest.hip reach on the second trip of their strided loop

Values (all from fixed seeds):
  base        off-diagonal entries +-[0.5, 2), a_ii = 1 + sum_j |a_ij|: strictly diagonally dominant, positive diagonal
  plain       base; x = +-[0.5, 2); b = fl(A x) + e with e_i = 2^-20 (|A||x| + |A x|)_i u_i, u_i in [0.1, 0.4] and u = 1 in one planted row: x is
              no solution, and the planted row holds the unique maximal ratio |r_i| / (|A||x| + |b|)_i by a factor of two at least
  cancelling  base, except that the diagonal of every edge row is chosen so that sum_j a_ij x_j = 2^-40 sum_j |a_ij||x_j| to within a
              rounding, and b_i there is of that size: no longer dominant, used for the residual alone
  planted max base, except entry p of an edge row r, in column c: |a_rc| = P >= 16 max of the other entries of row r, and
              a_cc = 4 P^2 (1 + sum_k |a_ck|), so that D^-1 A D^-1 with D_c = 2 P is still strictly diagonally dominant and A positive
              definite (for the diagonal entry: a_rr times a power of two).  Entry p decides the row maximum of the first sweep, losing it
              moves s_r by two binades, and after one sweep row r holds the smallest row maximum (a_rr / P <= 1 / 16 against 1 elsewhere)
  norm1       base with the diagonal of one edge row raised until its row sum is at least twice every other (the row without a diagonal:
              its entries times 8 and the other diagonals rebuilt)
"""
import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np

LPRS = (4, 8, 16, 32, 64)
BAND_W = {4: 0, 8: 1, 16: 6, 32: 17, 64: 30}
U = 2.0 ** -53
SHIFT = 2300            # exact sums are integers times 2^-SHIFT (products of two doubles need 2 * 1074 + 106 bits below 1 at the most)


# ---- the partition ----------------------------------------------------------------------------------------------------------------

def pick_lanes(nnz, n):
    avg = nnz / n if n > 0 else 1.0
    return 4 if avg <= 5.0 else 8 if avg <= 10.0 else 16 if avg <= 24.0 else 32 if avg <= 56.0 else 64


def long_min(lpr):
    return max(256, 8 * lpr)


def nb_short(n, lpr):
    return (n * lpr + 255) // 256 if n > 0 else 0


def row_map(n, colptr, rowval):
    """(rows, pairs): rows[i] = [(column, pair), ...] in the order of the map, pairs[m] = (i, j, [input positions]) with i >= j"""
    pairs, slot = [], {}
    for j in range(n):
        for p in range(int(colptr[j]), int(colptr[j + 1])):
            i = int(rowval[p])
            if i < j:
                continue
            m = slot.get((i, j))
            if m is None:
                slot[(i, j)] = len(pairs)
                pairs.append((i, j, [p]))
            else:
                pairs[m][2].append(p)
    rows = [[] for _ in range(n)]
    for m, (i, j, _) in enumerate(pairs):
        rows[i].append((j, m))
        if i != j:
            rows[j].append((i, m))
    return rows, pairs


@dataclasses.dataclass
class Design:
    name: str
    n: int
    colptr: np.ndarray
    rowval: np.ndarray
    rows: list
    pairs: list
    upper: list                      # input positions of the ignored upper-triangle entries
    edge: dict                       # label -> row: the rows of prescribed length and the rows at the ends of workgroups
    claim: dict                      # what the design claims of itself (lpr, long rows, ...), checked by the host test
    factorable: bool = True
    last: tuple = ()                 # rows the test orders last (a row without a diagonal)

    @functools.cached_property
    def nnz(self):
        return sum(len(r) for r in self.rows)

    @functools.cached_property
    def lpr(self):
        return pick_lanes(self.nnz, self.n)

    @property
    def g(self):
        return 256 // self.lpr

    @property
    def long_min(self):
        return long_min(self.lpr)

    @property
    def nb_short(self):
        return nb_short(self.n, self.lpr)

    @functools.cached_property
    def long_rows(self):
        return [i for i, r in enumerate(self.rows) if len(r) > self.long_min]

    @functools.cached_property
    def ndup(self):
        return sum(1 for r in self.rows for _, m in r if len(self.pairs[m][2]) > 1)

    @functools.cached_property
    def flat(self):
        """(row, column, pair) of every entry of the map as arrays"""
        R = np.repeat(np.arange(self.n, dtype=np.int64), [len(r) for r in self.rows])
        Cc = np.array([c for r in self.rows for c, _ in r], dtype=np.int64)
        M = np.array([m for r in self.rows for _, m in r], dtype=np.int64)
        return R, Cc, M

    @functools.cached_property
    def pair_index(self):
        """(first input position of every pair, the pairs listed more than once)"""
        first = np.array([pos[0] for _, _, pos in self.pairs], dtype=np.int64)
        return first, [m for m, (_, _, pos) in enumerate(self.pairs) if len(pos) > 1]

    def query(self):
        """what okkt_debug_row_map must report"""
        return (self.lpr, self.long_min, self.nb_short, len(self.long_rows), self.ndup, self.nnz)

    def is_long(self, row):
        return len(self.rows[row]) > self.long_min

    def owner(self, row, p):
        """(lane, wave) of entry p of a long row; (lane of the row's group, None) of a short one"""
        if self.is_long(row):
            return p % 256, (p % 256) // 64
        return p % self.lpr, None

    def workgroup(self, row):
        """the partial a row's result goes through: its short workgroup, or nb_short + its place among the long rows"""
        if self.is_long(row):
            return self.nb_short + self.long_rows.index(row)
        return row // self.g

    def reduce_slot(self, row):
        """(thread, trip) at which the one-workgroup final kernels read that partial"""
        w = self.workgroup(row)
        return w % 256, w // 256

    def raw(self, nz):
        return (self.n, self.colptr, self.rowval, np.asarray(nz, dtype=np.float64), 0)

    def positions(self, row):
        """the entries of a row that a lane loop can lose: first, lpr - 1, lpr, last; on the long route 0, 63, 64, 255, 256, last"""
        ln = len(self.rows[row])
        cand = (0, 63, 64, 255, 256, ln - 1) if self.is_long(row) else (0, self.lpr - 1, self.lpr, ln - 1)
        return sorted({p for p in cand if 0 <= p < ln})


# ---- patterns ---------------------------------------------------------------------------------------------------------------------

def _design(name, n, adj, edge, claim, dups=(), factorable=True, last=(), descending=False):
    """lower CSC of the symmetric pattern adj (sets, the diagonal included where stored)"""
    dups = set(dups)
    colptr, rowval, upper = [0], [], []
    for j in range(n):
        low = sorted((i for i in adj[j] if i >= j), reverse=descending)
        for i in low:
            rowval.append(i)
            if (i, j) in dups:
                rowval.append(i)
        if descending:                       # entries above the diagonal: ignored by the analysis, the map and the factorisation
            for i in sorted(c for c in adj[j] if c < j)[:3]:
                upper.append(len(rowval))
                rowval.append(i)
        colptr.append(len(rowval))
    colptr, rowval = np.array(colptr, dtype=np.int64), np.array(rowval, dtype=np.int64)
    rows, pairs = row_map(n, colptr, rowval)
    return Design(name, n, colptr, rowval, rows, pairs, upper, dict(edge), dict(claim), factorable, tuple(last))


def _band(n, w):
    return [set(range(max(0, i - w), min(n, i + w + 1))) for i in range(n)]


def _set_length(adj, r, length, special):
    """cut (farthest neighbour first) or fill (evenly spread columns that are no special row) row r to `length` entries"""
    n = len(adj)
    while len(adj[r]) > length:
        c = max((c for c in adj[r] if c != r), key=lambda c: (abs(c - r), c))
        adj[r].discard(c)
        adj[c].discard(r)
    need = length - len(adj[r])
    if need > 0:
        cand = [c for c in range(n) if c not in adj[r] and c not in special and c != r]
        if len(cand) < need:
            raise ValueError("too few columns")
        for k in range(need):
            c = cand[(k * len(cand)) // need]
            adj[r].add(c)
            adj[c].add(r)


def _edge_design(lpr, variant, n, dups=False, empty=False, nodiag=False, name=None):
    """the band design of `lpr` with n rows, or ValueError where n cannot hold it"""
    w, g, lm = BAND_W[lpr], 256 // lpr, long_min(lpr)
    big = lm + 256 + 1 if lpr == 64 else 2 * 256 + 1
    first = 2 * g                                      # first row of workgroup 2
    lengths = {"first": lm + 1, "last": lm, "a": lm - 1, "b": big} if variant == 0 else {"first": lm, "last": lm + 1, "a": big, "b": lm - 1}
    short = {"len1": 1, "lpr-1": lpr - 1, "lpr": lpr, "lpr+1": lpr + 1, "2lpr+1": 2 * lpr + 1}
    free = [r for r in range(w + 3, n - 1 - w - 1, 2 * w + 7) if abs(r - first) > w + 1]
    if empty:
        short["empty"] = 0
    if len(free) < len(short) + 2:
        raise ValueError("too few rows")
    where = {"first": first, "last": n - 1, "a": free[0], "b": free[1]}
    if empty:                                          # in the last full workgroup of the -one variant
        wg = (n - 1) // g - 1
        free = [r for r in free if r // g != wg] + []
        where["empty"] = wg * g + g // 2
        if any(abs(where["empty"] - r) <= w + 1 for r in list(where.values())[:-1] + free[2:2 + len(short)]):
            raise ValueError("the empty row has a special neighbour")
    for k, lab in enumerate(s for s in short if s != "empty"):
        where[lab] = free[2 + k]
    special = set(where.values())
    adj = _band(n, w)
    if empty:
        r = where["empty"]
        for c in list(adj[r]):
            adj[r].discard(c)
            adj[c].discard(r)
    nd = where["b" if variant == 0 else "a"] if nodiag else None
    if nd is not None:
        adj[nd].discard(nd)
    for lab, ln in short.items():
        if lab != "empty":
            _set_length(adj, where[lab], ln, special)
    for lab, ln in lengths.items():
        _set_length(adj, where[lab], ln, special)
    dup = []
    if dups:
        for lab in lengths:
            r = where[lab]
            dup += [(max(r, c), min(r, c)) for c in sorted(adj[r]) if (r + c) % 3 == 0]
    claim = dict(lpr=lpr, long=sorted(where[lab] for lab, ln in lengths.items() if ln > lm), lengths={**lengths, **short},
                 first_of_workgroup=[first], last_of_matrix=n - 1, rows_in_last_workgroup=(n - 1) % g + 1)
    name = name or f"lpr{lpr}-{'full' if variant == 0 else 'one'}"
    return _design(name, n, adj, where, claim, dups=dup, factorable=not empty, last=(nd,) if nd is not None else (), descending=dups)


def _smallest(lpr, variant, **kw):
    """the smallest n = variant (mod g) that holds the arrow rows and lands on lpr"""
    g = 256 // lpr
    n0 = (long_min(lpr) + 256 + 1 if lpr == 64 else 513)
    for n in range(n0, 4 * n0):
        if n % g != variant % g:
            continue
        try:
            d = _edge_design(lpr, variant, n, **kw)
        except ValueError:
            continue
        if d.lpr == lpr and d.long_rows == d.claim["long"]:
            return d
    raise AssertionError((lpr, variant))


def _boundary(avg, over):
    """the smallest band-like pattern with nnz = avg * n, or one off-diagonal pair more"""
    n = {5: 8, 10: 16, 24: 32, 56: 64}[avg]
    k = (avg * n - n) // 2 + (1 if over else 0)
    assert (avg * n - n) % 2 == 0
    order = sorted(((i - j, j, i) for i in range(n) for j in range(i)))[:k]
    adj = [{i} for i in range(n)]
    for _, j, i in order:
        adj[i].add(j)
        adj[j].add(i)
    lo = pick_lanes(avg * n, n)
    claim = dict(lpr=LPRS[LPRS.index(lo) + 1] if over else lo, long=[], nnz=avg * n + (2 if over else 0))
    return _design(f"avg{avg}-{'over' if over else 'on'}", n, adj, {"row0": 0, "last": n - 1}, claim)


def _tridiagonal(n, name, zero_last=False):
    adj = _band(n, 1)
    if zero_last:
        adj[n - 1].discard(n - 2)
        adj[n - 2].discard(n - 1)
    g = 64
    edge = {"row0": 0, "last-of-wg": ((n - 1) // g) * g - 1, "last": n - 1}
    return _design(name, n, adj, edge, dict(lpr=4, long=[], rows_in_last_workgroup=(n - 1) % g + 1))


@functools.lru_cache(maxsize=None)
def catalogue():
    out = {}
    for lpr in LPRS:
        for v in (0, 1):
            d = _smallest(lpr, v)
            out[d.name] = d
    out["lpr8-dups"] = _smallest(8, 0, dups=True, name="lpr8-dups")
    out["lpr8-empty"] = _smallest(8, 1, empty=True, name="lpr8-empty")
    out["lpr16-nodiag"] = _smallest(16, 0, nodiag=True, name="lpr16-nodiag")
    out["zero-last"] = _tridiagonal(129, "zero-last", zero_last=True)
    for avg in (5, 10, 24, 56):
        for over in (False, True):
            d = _boundary(avg, over)
            out[d.name] = d
    out["n1"] = _design("n1", 1, [{0}], {"row0": 0}, dict(lpr=4, long=[]))
    out["n2-empty"] = _design("n2-empty", 2, [{0}, set()], {"row0": 0, "empty": 1}, dict(lpr=4, long=[]), factorable=False)
    out["tridiag-16385"] = _tridiagonal(16385, "tridiag-16385")
    return out


BAND_DESIGNS = [f"lpr{lpr}-{v}" for lpr in LPRS for v in ("full", "one")]
BOUNDARY_DESIGNS = [f"avg{a}-{o}" for a in (5, 10, 24, 56) for o in ("on", "over")]
ALL_DESIGNS = BAND_DESIGNS + ["lpr8-dups", "lpr8-empty", "lpr16-nodiag", "zero-last"] + BOUNDARY_DESIGNS + ["n1", "n2-empty", "tridiag-16385"]
FACTORED_DESIGNS = [d for d in ALL_DESIGNS if d not in ("lpr8-empty", "n2-empty")]


def resid_edges(d):
    """the edge rows whose residual has size: those with an entry, the stored zero row of zero-last excepted"""
    return [r for r in sorted(set(d.edge.values())) if d.rows[r] and not (d.name == "zero-last" and r == d.n - 1)]


def checked_rows(d):
    """the rows whose residual is compared with exact arithmetic: all of them up to about 1 100 rows; of the large design workgroups 0,
    255 and 256 and 200 further rows from a fixed seed"""
    if d.n <= 1200:
        return list(range(d.n))
    g = d.g
    rows = set(range(g)) | set(range(255 * g, d.n))
    rows |= set(int(i) for i in np.random.default_rng(7).choice(d.n, 200, replace=False))
    return sorted(rows)


# ---- values -----------------------------------------------------------------------------------------------------------------------

def to_nz(d, pv, junk=1.0e30):
    """input values of the pair values pv: a pair listed twice as 0.25 v and 0.75 v, the upper-triangle entries junk"""
    first, multi = d.pair_index
    nz = np.zeros(len(d.rowval))
    nz[first] = pv
    for m in multi:
        pos = d.pairs[m][2]
        nz[pos[0]] = 0.25 * pv[m]
        nz[pos[1]] = 0.75 * pv[m]
    for k, p in enumerate(d.upper):
        nz[p] = junk * (1 + k % 7)
    return nz


def pair_values(d, nz):
    """the value of every pair as the gather kernels form it: one entry, or the sum of its entries in input order from 0"""
    first, multi = d.pair_index
    out = np.asarray(nz, dtype=np.float64)[first]
    for m in multi:
        out[m] = pair_values_one(d, nz, m)
    return out


def row_values(d, nz, rows=None):
    """{row: [(column, value), ...]} in the order of the map"""
    pv = pair_values(d, nz)
    return {i: [(c, float(pv[m])) for c, m in d.rows[i]] for i in (range(d.n) if rows is None else rows)}


def _dominant(d, pv):
    off = np.zeros(d.n)
    dg = {}
    for m, (i, j, _) in enumerate(d.pairs):
        if i == j:
            dg[i] = m
        else:
            off[i] += abs(pv[m])
            off[j] += abs(pv[m])
    for i, m in dg.items():
        pv[m] = 1.0 + off[i]
    return pv, off, dg


def base_pairs(d, seed=1):
    rng = np.random.default_rng(seed)
    pv = rng.choice([-1.0, 1.0], len(d.pairs)) * rng.uniform(0.5, 2.0, len(d.pairs))
    pv, _, dg = _dominant(d, pv)
    if d.name == "zero-last":
        pv[dg[d.n - 1]] = 0.0
    return pv


def base_values(d, seed=1):
    return to_nz(d, base_pairs(d, seed))


def _fexact(v):
    m, e = math.frexp(v)
    return int(m * 9007199254740992.0), e - 53


def exact_dot(row, x, absolute=False):
    """sum_j a_j x_j (or sum |a_j||x_j|) of a row [(column, value)] as a Fraction: integer arithmetic at the scale 2^-SHIFT"""
    acc = 0
    for c, v in row:
        ma, ea = _fexact(v)
        mx, ex = _fexact(float(x[c]))
        t = (ma * mx) << (ea + ex + SHIFT)
        acc += abs(t) if absolute else t
    return Fraction(acc, 1 << SHIFT)


def exact_residual(row, b_i, x):
    """(r, |A||x|) of one row, exact"""
    return Fraction(float(b_i)) - exact_dot(row, x), exact_dot(row, x, absolute=True)


def residual_bound(r_exact, ax_exact, nnz_i):
    """|r - r_exact| <= u |r_exact| + 4 nnz_i u^2 (|A||x|)_i: one rounding of the result and the double-double accumulation"""
    return Fraction(U) * abs(r_exact) + 4 * max(nnz_i, 1) * Fraction(U) * Fraction(U) * ax_exact


def plain_rhs(d, nz, seed, plant=None):
    """(x, b) of the value set "plain" on the matrix nz; the row `plant` holds the maximal ratio"""
    rng = np.random.default_rng(1000 + seed)
    x = rng.choice([-1.0, 1.0], d.n) * rng.uniform(0.5, 2.0, d.n)
    u = rng.uniform(0.1, 0.4, d.n)
    if plant is not None:
        u[plant] = 1.0
    ax, s = float_products(d, nz, x)
    b = ax + 2.0 ** -20 * (s + np.abs(ax)) * u
    return x, b


def float_products(d, nz, x):
    """(A x, |A||x|) in double, the rows summed in some fixed order: for building right-hand sides and for margins of a factor of two"""
    R, Cc, M = d.flat
    t = pair_values(d, nz)[M] * x[Cc]
    return np.bincount(R, weights=t, minlength=d.n), np.bincount(R, weights=np.abs(t), minlength=d.n)


def float_ratios(d, nz, x, b):
    """|r_i| / (|A||x| + |b|)_i in double (0 / 0 = 0)"""
    ax, s = float_products(d, nz, x)
    den = s + np.abs(b)
    return np.where(den > 0, np.abs(b - ax) / np.where(den > 0, den, 1.0), 0.0)


def cancelling(d, seed=3):
    """(nz, x, b) of the value set "cancelling": in every edge row that stores a diagonal, sum a x = 2^-40 sum |a||x| to a rounding"""
    pv = base_pairs(d)
    nz = to_nz(d, pv)
    x, b = plain_rhs(d, nz, seed)
    rng = np.random.default_rng(2000 + seed)
    done = []
    for r in sorted(set(d.edge.values())):
        dg = [m for c, m in d.rows[r] if c == r]
        if not dg or len(d.rows[r]) < 2 or len(d.pairs[dg[0]][2]) > 1:
            continue
        row = [(c, float(pair_values_one(d, nz, m))) for c, m in d.rows[r] if c != r]
        t = exact_dot(row, x)
        s = exact_dot(row, x, absolute=True)
        delta = Fraction(float(rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 2.0))) * s / (1 << 40)
        nz[d.pairs[dg[0]][2][0]] = float((delta - t) / Fraction(float(x[r])))
        b[r] = float(rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 2.0)) * float(s) * 2.0 ** -41
        done.append(r)
    return nz, x, b, done


def pair_values_one(d, nz, m):
    pos = d.pairs[m][2]
    if len(pos) == 1:
        return nz[pos[0]]
    s = 0.0
    for p in pos:
        s = s + float(nz[p])
    return s


def planted_max_sets(d):
    """[(nz, [(row, p), ...])]: the "planted max" value sets, one position of a row each, plants that cannot disturb each other sharing a
    set: distinct rows, distinct partner columns, no partner that is a planted row."""
    plants = [(r, p) for r in sorted(set(d.edge.values())) if len(d.rows[r]) >= 2 for p in d.positions(r)]
    groups = []
    for r, p in plants:
        c = d.rows[r][p][0]
        for grp in groups:
            if all(r != r2 and c != c2 and c != r2 and c2 != r for r2, _, c2 in grp):
                grp.append((r, p, c))
                break
        else:
            groups.append([(r, p, c)])
    out = []
    base = base_pairs(d)
    _, off, dg = _dominant(d, base.copy())
    for grp in groups:
        pv = base.copy()
        for r, p, c in grp:
            m = d.rows[r][p][1]
            others = max(abs(pv[k]) for q, (_, k) in enumerate(d.rows[r]) if q != p)
            big = abs(pv[m]) * 2.0 ** max(math.ceil(math.log2(16.0 * others / abs(pv[m]))), 0)
            pv[m] = math.copysign(big, pv[m])
            if c != r:
                pv[dg[c]] = 4.0 * big * big * (1.0 + off[c])
        out.append((to_nz(d, pv), [(r, p) for r, p, _ in grp]))
    return out


def norm1_set(d, row):
    """nz of the value set that makes `row` the maximal row of |A| by a factor of two at least"""
    pv = base_pairs(d)
    has_diag = any(c == row for c, _ in d.rows[row])
    if not has_diag:
        for c, m in d.rows[row]:
            pv[m] *= 8.0
        pv, _, _ = _dominant(d, pv)
        return to_nz(d, pv)
    sums = np.zeros(d.n)
    for m, (i, j, _) in enumerate(d.pairs):
        sums[i] += abs(pv[m])
        if i != j:
            sums[j] += abs(pv[m])
    other = max((sums[i] for i in range(d.n) if i != row), default=0.0)
    m = next(m for c, m in d.rows[row] if c == row)
    pv[m] = max(pv[m], math.ceil(2.0 * other + 1.0))
    return to_nz(d, pv)


def exact_row_sum(row):
    return sum((Fraction(abs(v)) for _, v in row), Fraction(0))


def norm1_bound(length, lanes):
    """gamma_k, k = ceil(len / lanes) + log2(lanes) + 3: the additions of one lane, the butterfly (on the long route six levels and three
    wave sums, which log2(256) + 3 covers), the shift added to the diagonal entry, |shift| added to a row without one, one to spare"""
    k = -(-length // lanes) + int(math.log2(lanes)) + 3
    return Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))
