"""Designed elimination trees: symmetric indefinite matrices whose supernodal fronts are chosen, not found.

A design is a forest of `Node`s.  A node has k pivot columns and a contribution block (CB) of c rows; its front has f = k + c
rows.  `build(design)` returns the lower triangle of a matrix (CSC, in a shuffled labelling), the permutation that undoes the
shuffle (perm[new] = old: pass it with `ordering = 2`) and what the symbolic phase has to find for it:

  * every node's pivot block is dense, and so is its f x k panel (pivots, then the CB rows);
  * the CB rows of a child are a strict subset of its parent's front rows that contains the parent's FIRST pivot: the child hangs
    below the parent in the elimination tree, its pivot columns stay one supernode (the parent's front is never the child's CB plus
    one column, so fundamental supernodes do not merge them), and the parent's pivots stay consecutive in the postorder;
  * without "scatter" the CB is the leading c rows of the parent's front, with it the c rows are spread evenly through the parent's
    front (a non-contiguous extend-add);
  * children are numbered by ascending CB size (stable), the postorder the analysis itself produces -- so the permutation the
    handle reports is the design's own.

Amalgamation has to be off for the fronts to be the designed ones: `NO_RELAX` (values <= 0 mean "default", hence 1 and 1e-300:
no merge is small enough, and only a merge that adds no zero -- impossible here -- has a zero fraction below 1e-300).

Values ("plain"): N(0,1) entries in every panel, diagonal +-3 sqrt(f) with a designed sign (the recipe of the dense tests).
Values ("ipm"): the shape of a late interior-point iterate.  Columns of positive sign form an H block with diagonal 3 sqrt(f); columns
of negative sign carry -s/y on the diagonal, s/y log-uniform in 1e-6 .. 1e6, and no entry between two of them (the diagonal (2,2)
block of a KKT system: the pattern stays dense, the value is 0).  The matrix is then equilibrated symmetrically (every row and column
divided by the square root of its largest entry) so that its largest entries are O(1).

`true_solution` refines the oracle's solve with long-double residuals: the reference solution of the fp64 matrix.
"""
import numpy as np
import scipy.sparse as sp

NO_RELAX = dict(relax_always=1, relax_small=1, relax_mid=1, relax_small_frac=1e-300, relax_mid_frac=1e-300, relax_any_frac=1e-300)


class Node:
    def __init__(self, k, c=0, *children, scatter=False):
        assert k >= 1 and c >= 0
        self.k, self.c, self.children, self.scatter = int(k), int(c), list(children), bool(scatter)

    @property
    def f(self):
        return self.k + self.c


def N(k, c=0, *children, scatter=False):
    return Node(k, c, *children, scatter=scatter)


class Built:
    """What `build` designs: the matrix (lower triangle, CSC, shuffled labels), perm (perm[new] = old), and per node of the design
    (in postorder) its k, f, level (height above the leaves), pivot columns and front rows in the permuted numbering."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def fronts(self):
        """(k, f, level) of every front, postorder."""
        return [(nd["k"], nd["f"], nd["level"]) for nd in self.nodes]

    def fingerprint(self):
        ks = np.array([nd["k"] for nd in self.nodes], dtype=np.int64)
        fs = np.array([nd["f"] for nd in self.nodes], dtype=np.int64)
        return dict(nsuper=len(self.nodes), max_front=int(fs.max()), nlevels=1 + max(nd["level"] for nd in self.nodes),
                    sum_rowidx=int(fs.sum()), nnzL_stored=int((fs * ks - ks * (ks - 1) // 2).sum()))

    def colcounts(self):
        """Column counts of L (diagonal included) in the permuted numbering: f - i for the i-th pivot of a front."""
        cnt = np.zeros(self.n, dtype=np.int64)
        for nd in self.nodes:
            cnt[nd["col0"]:nd["col0"] + nd["k"]] = nd["f"] - np.arange(nd["k"])
        return cnt

    def l_pattern(self):
        """Strictly lower pattern of L, permuted numbering, as a CSC matrix of ones."""
        rows, cols = [], []
        for nd in self.nodes:
            r = nd["rows"]
            for i in range(nd["k"]):
                rows.append(r[i + 1:])
                cols.append(np.full(len(r) - i - 1, nd["col0"] + i))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        M = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(self.n, self.n))
        M.sort_indices()
        return M


def _postorder(roots):
    """Nodes in the order the analysis numbers them: children by ascending CB size (stable), then the node."""
    out = []

    def visit(nd, parent, depth):
        for ch in sorted(nd.children, key=lambda x: x.c):
            visit(ch, nd, depth + 1)
        out.append((nd, parent))

    for r in roots:
        assert r.c == 0, "a root has no contribution block"
        visit(r, None, 0)
    return out


def build(roots, values="plain", seed=0):
    """seed: the values (the pattern and the labelling do not depend on it: refactorisations on one pattern)."""
    order = _postorder(roots)
    idx = {id(nd): i for i, (nd, _) in enumerate(order)}
    col0, pos = [], 0
    for nd, _ in order:
        col0.append(pos)
        pos += nd.k
    n = pos
    level = [0] * len(order)
    for i, (nd, par) in enumerate(order):
        if par is not None:
            level[idx[id(par)]] = max(level[idx[id(par)]], level[i] + 1)
    # front rows, parents first (reverse postorder)
    rows = [None] * len(order)
    for i in range(len(order) - 1, -1, -1):
        nd, par = order[i]
        piv = np.arange(col0[i], col0[i] + nd.k)
        if par is None:
            rows[i] = piv
            continue
        R = rows[idx[id(par)]]
        assert nd.c < len(R), f"the CB of a ({nd.k}, {nd.c}) front must be a strict subset of its parent's {len(R)} rows"
        assert nd.c >= 1, "a child needs a CB"
        sel = (np.arange(nd.c) * len(R)) // nd.c if nd.scatter else np.arange(nd.c)
        rows[i] = np.concatenate([piv, R[sel]])
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    fcol = np.zeros(n)
    r_all, c_all = [], []
    for i, (nd, _) in enumerate(order):
        R = rows[i]
        fcol[col0[i]:col0[i] + nd.k] = len(R)
        for j in range(nd.k):
            r_all.append(R[j:])
            c_all.append(np.full(len(R) - j, col0[i] + j))
    r_all, c_all = np.concatenate(r_all), np.concatenate(c_all)
    v = rng.normal(size=len(r_all))
    diag = r_all == c_all
    if values == "plain":
        v[diag] = sign[c_all[diag]] * 3.0 * np.sqrt(fcol[c_all[diag]])
    elif values == "ipm":
        neg = sign < 0
        v[neg[r_all] & neg[c_all] & ~diag] = 0.0
        sy = 10.0 ** rng.uniform(-6.0, 6.0, size=n)
        v[diag] = np.where(neg[c_all[diag]], -sy[c_all[diag]], 3.0 * np.sqrt(fcol[c_all[diag]]))
        big = np.zeros(n)
        np.maximum.at(big, r_all, np.abs(v))
        np.maximum.at(big, c_all, np.abs(v))
        sc = 1.0 / np.sqrt(big)
        v = v * sc[r_all] * sc[c_all]
    else:
        raise ValueError(values)
    # shuffled labels: the matrix the caller sees is P^T A P, perm[new] = old undoes it
    perm = np.random.default_rng(n).permutation(n)
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    a, b = perm[r_all], perm[c_all]
    lo, hi = np.maximum(a, b), np.minimum(a, b)
    A = sp.csc_matrix((v, (lo, hi)), shape=(n, n))
    A.sort_indices()
    npos = int((sign > 0).sum())
    nodes = [dict(k=nd.k, f=nd.f, level=level[i], col0=col0[i], rows=rows[i], parent=None if par is None else idx[id(par)])
             for i, (nd, par) in enumerate(order)]
    return Built(n=n, A=A, perm=perm.astype(np.int64), iperm=iperm, nodes=nodes, npos=npos, nneg=n - npos, values=values)


def full_csr(A):
    """The symmetric matrix of a lower triangle, CSR."""
    A = sp.csc_matrix(A)
    return (sp.tril(A) + sp.tril(A, -1).T).tocsr()


def true_solution(M, solve, b, steps=4):
    """The oracle's solution of M x = b refined with long-double residuals (M: full symmetric CSR, solve: the oracle's fp64 solve)."""
    x = solve(b)
    data = M.data.astype(np.longdouble)
    bl = b.astype(np.longdouble)
    for _ in range(steps):
        prod = data * x.astype(np.longdouble)[M.indices]
        r = (bl - np.add.reduceat(prod, M.indptr[:-1])).astype(np.float64)
        x = x + solve(r)
    return x


def rhs(n, nrhs, seed=7):
    """nrhs right-hand sides, one per row (the layout of okkt_solve's batches)."""
    return np.random.default_rng(seed).normal(size=(nrhs, n))


def fwd_err(x, xt):
    return float(np.max(np.abs(x - xt)) / np.max(np.abs(xt)))


# ---------------------------------------------------------------------------------------------------------------------------------
# The catalogue: every design the GPU file runs (and the CPU test checks the analysis of).  id -> (forest, what it is for).

def _edge(k, c):
    """A (k, c) front: the child of a root that takes its CB (root of its own tree when c = 0)."""
    return [N(k)] if c == 0 else [N(c + 1, 0, N(k, c))]


# pivot-block and CB edges of the big-front kernels (tiles of 128, 64-column solve steps, 1024-column inverses, 2048 super-blocks):
# every k and every c at least once, k mod 1024 in {1, 129} (the padded last inverse block), ragged pivot AND ragged CB tiles
EDGE_PAIRS = [(129, 700), (255, 129), (256, 0), (257, 127), (383, 63), (384, 128), (385, 1), (1023, 128), (1024, 63), (1025, 1),
              (2047, 0), (2048, 127), (2049, 129)]


def _mixed(scatter):
    """One level of five fronts: under one separator a thin (k <= 128), a mid (129 .. 384), a wide (> 384) and a small front, and
    beside them the root of a tree of its own."""
    return [N(260, 0, N(100, 200, scatter=scatter), N(300, 150, scatter=scatter), N(500, 250, scatter=scatter),
              N(24, 8, scatter=scatter)),
            N(450)]


def _fold(nmid):
    """A big front and `nmid` lone mid-size fronts (33 .. small_max rows) in one level: up to 3 join the big fronts' launch."""
    return [N(200, 0, N(200, 150), *[N(30 + 5 * i, 20 + 5 * i) for i in range(nmid)])]


def _chain_small(depth):
    nd = N(8, 16)
    for _ in range(depth - 1):
        nd = N(8, 16, nd)
    return nd


DESIGNS = {}
for _k, _c in EDGE_PAIRS:
    DESIGNS[f"edge-k{_k}-c{_c}"] = (_edge(_k, _c), "pivot / CB edge")
DESIGNS.update({
    "thin-tall-k1-2-127-128-c2100": ([N(2101, 0, N(1, 2100), N(2, 2100), N(127, 2100), N(128, 2100))],
                                     "k = 1 .. 128 fronts of 2100 CB rows: maxf > 2048 (plain and chunked assembly), fused thin sweeps"),
    "thin-k128-f2049": ([N(1922, 0, N(128, 1921))], "a thin front of just above 2048 rows"),
    "small-classes-f32-33-64-65-128-129": ([N(17, 0, *[N(f - 16, 16) for f in (32, 33, 64, 65, 128, 129)])],
                                           "small-front classes at their edges (<= 32, <= 64, <= small_max)"),
    "task-chains-under-big": ([N(300, 0, _chain_small(8), _chain_small(6), N(150, 120))], "subtrees of small fronts run as tasks"),
    "fold-lone-1": (_fold(1), "fold rule"),
    "fold-lone-3": (_fold(3), "fold rule, at its limit"),
    "fold-lone-4": (_fold(4), "fold rule, past its limit"),
    "mixed-level": (_mixed(False), "thin, mid, wide, small fronts and a separate root in one level"),
    "mixed-level-scatter": (_mixed(True), "the same with non-contiguous extend-add"),
    "forest-3-roots": ([N(500), N(1100), N(1700)], "three big roots in one level"),
    "deep-chain-6": ([N(300, 0, N(200, 290, N(160, 440, N(150, 560, N(140, 650, N(130, 740))))))],
                     "six big fronts, each CB most but not all of its parent's front"),
    "fan-in-8": ([N(400, 0, *[N(k, c, scatter=(i % 2 == 1)) for i, (k, c) in enumerate(
        [(150, 399), (200, 300), (129, 380), (260, 250), (385, 200), (300, 390), (180, 129), (230, 128)])])],
                 "eight big children whose CBs are alive together"),
})

# the designs the subprocess runs under the other routes
VARIANT_DESIGNS = ["mixed-level", "fan-in-8", "deep-chain-6", "edge-k2049-c129"]
