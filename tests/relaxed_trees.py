"""Designed elimination trees under relaxed supernode amalgamation: a model of the merge rule and a catalogue of designs at its edges.

front_trees.py designs fronts and switches amalgamation off so that the analysis finds exactly them.  Every production run factors
with amalgamation ON; this module restates the rule on a design (`merged`) so that the fronts the analysis must form from a design
under given relaxation options -- and with them the stored pattern of L, the positions of the explicit ("relaxation") zeros, the
levels and the statistics -- are known without the code under test.  Nothing here imports the library.

The rule (one pass over the fundamental supernodes s = 0 .. ns - 2 in postorder; here the designed nodes):
  * s is a candidate when its parent in the tree is s + 1 (the last child: the one with the largest contribution block);
  * with the current widths kc (of s, after earlier merges) and kp (of s + 1) and the parent's designed front order fp:
    km = kc + kp, fm = kc + fp, stored = fm km - km (km - 1) / 2, z = (stored - (truennz_s + truennz_p)) / stored;
  * merge iff km <= always, or (km <= small and z < small_frac), or (km <= mid and z < mid_frac), or z < any_frac;
  * after a merge the parent carries the summed width and true count: chains merge transitively, and a refused merge starts anew.
z is a `fractions.Fraction`; the catalogue keeps every decision at least MARGIN away from a fraction it is compared with, so the
library's fp64 z decides the same.

Schur mode (`nschur` > 0: the last nschur columns of the design are the Schur set): the Schur set is one dense supernode; a designed
node that straddles column n - nschur is split there and never re-joined; nothing merges into the Schur supernode.
"""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import front_trees as ft
from front_trees import N

# the defaults of the analysis, restated
DEFAULT_RELAX = dict(relax_always=64, relax_small=256, relax_small_frac=0.25, relax_mid=96, relax_mid_frac=0.15, relax_any_frac=0.03)
# the one set of options under which the `mid` clause decides: at the defaults mid <= small and mid_frac <= small_frac, so whatever
# the mid clause accepts the small clause accepts too
MID_RELAX = dict(relax_always=8, relax_small=40, relax_small_frac=0.10, relax_mid=24, relax_mid_frac=0.30, relax_any_frac=0.01)
MARGIN = 1e-3
SMALL_MAX = 128          # the default small_front_max: a front of more rows is a "big front"
CLAUSES = ("always", "small", "mid", "any")


def trapezoid(f, k):
    """Stored entries of the first k columns of a front of order f (diagonal included)."""
    return f * k - k * (k - 1) // 2


class Merged:
    """What `merged` derives: `fronts` (postorder; dicts of k, f, col0, rows, level, parent, members -- the design's node indices),
    `decisions` (one per candidate: s, km, fm, z, open, true, merge) and the design it came from."""

    def __init__(self, d, fronts, decisions, nnzL, nschur):
        self.d, self.n, self.fronts, self.decisions, self.nnzL, self.nschur = d, d.n, fronts, decisions, nnzL, nschur

    def fingerprint(self):
        ks = np.array([fr["k"] for fr in self.fronts], dtype=np.int64)
        fs = np.array([fr["f"] for fr in self.fronts], dtype=np.int64)
        return dict(nsuper=len(self.fronts), max_front=int(fs.max()), nlevels=1 + max(fr["level"] for fr in self.fronts),
                    sum_rowidx=int(fs.sum()), nnzL_stored=int((fs * ks - ks * (ks - 1) // 2).sum()),
                    n_big_fronts=int((fs > SMALL_MAX).sum()), nnzL=int(self.nnzL))

    @property
    def shapes(self):
        """(k, f) of every merged front, postorder."""
        return [(fr["k"], fr["f"]) for fr in self.fronts]

    def big_fronts(self):
        """(level, f, k) of every merged front of more than SMALL_MAX rows, sorted."""
        return sorted((fr["level"], fr["f"], fr["k"]) for fr in self.fronts if fr["f"] > SMALL_MAX)

    def stored_pattern(self):
        """Strictly lower stored pattern of L (permuted numbering, CSC of ones): every merged front's panel, zeros included."""
        return _pattern(self.n, self.fronts)

    def true_pattern(self):
        """Strictly lower pattern of L without amalgamation."""
        return self.d.l_pattern()

    def zero_pattern(self):
        """The relaxation zeros: stored positions that are no entry of L."""
        Z = (self.stored_pattern() - self.true_pattern()).tocsc()
        Z.eliminate_zeros()
        Z.sort_indices()
        assert Z.nnz == self.fingerprint()["nnzL_stored"] - self.nnzL and (Z.data == 1.0).all()
        return Z

    def front_of_node(self, i):
        """Index of the merged front that holds designed node i."""
        return next(j for j, fr in enumerate(self.fronts) if i in fr["members"])


def _pattern(n, fronts):
    rows, cols = [], []
    for fr in fronts:
        r = fr["rows"]
        for i in range(fr["k"]):
            rows.append(r[i + 1:])
            cols.append(np.full(len(r) - i - 1, fr["col0"] + i))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    M = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    M.sort_indices()
    return M


def _nodes(d, nschur):
    """The fundamental supernodes of the design: the designed nodes, or in Schur mode the nodes below column n1 = n - nschur (the one
    that straddles n1 cut there) and one dense supernode of the Schur set."""
    nodes = [dict(k=nd["k"], f=nd["f"], col0=nd["col0"], rows=nd["rows"], parent=nd["parent"], members=[i]) for i, nd in enumerate(d.nodes)]
    if not nschur:
        return nodes
    n1 = d.n - nschur
    assert 0 < n1 < d.n
    keep = [nd for nd in nodes if nd["col0"] < n1]
    tail = [nd for nd in nodes if nd["col0"] + nd["k"] > n1]
    first = len(nodes) - len(tail)
    for t, nd in enumerate(tail):     # the Schur set lies in the top of one chain: dense already but for the new coupling of the cut node
        assert nd is nodes[first + t] and (nd["parent"] == first + t + 1 if t + 1 < len(tail) else nd["parent"] is None)
    schur = len(keep)
    for nd in keep:
        if nd["col0"] + nd["k"] > n1:
            nd["k"] = n1 - nd["col0"]
            nd["parent"] = schur
        elif nd["parent"] is not None and nd["parent"] >= len(keep):
            nd["parent"] = schur
    keep.append(dict(k=nschur, f=nschur, col0=n1, rows=np.arange(n1, d.n), parent=None, members=[first + t for t in range(len(tail))]))
    return keep


def merged(d, opts=None, nschur=0):
    """The fronts the analysis forms from the design `d` (an ft.build result) under the relaxation options `opts`."""
    o = dict(DEFAULT_RELAX, **(opts or {}))
    width_of = dict(always=o["relax_always"], small=o["relax_small"], mid=o["relax_mid"], any=None)
    frac_of = dict(always=None, small=Fraction(o["relax_small_frac"]), mid=Fraction(o["relax_mid_frac"]), any=Fraction(o["relax_any_frac"]))
    nodes = _nodes(d, nschur)
    ns = len(nodes)
    width = [nd["k"] for nd in nodes]
    true = [trapezoid(nd["f"], nd["k"]) for nd in nodes]
    nnzL = sum(true)
    head = list(range(ns))          # first fundamental supernode of the group that ends at s
    alive = [True] * ns
    decisions = []
    for s in range(ns - 1):
        p = s + 1
        if nodes[s]["parent"] != p:
            continue
        if nschur and p == ns - 1:
            continue
        kc, kp, fp = width[s], width[p], nodes[p]["f"]
        km, fm = kc + kp, kc + fp
        stored = trapezoid(fm, km)
        tn = true[s] + true[p]
        z = Fraction(stored - tn, stored)
        is_open = {c for c in CLAUSES if width_of[c] is None or km <= width_of[c]}
        holds = {c for c in is_open if frac_of[c] is None or z < frac_of[c]}
        decisions.append(dict(s=s, km=km, fm=fm, z=z, open=is_open, true=holds, merge=bool(holds),
                              margin=min([abs(z - frac_of[c]) for c in is_open if frac_of[c] is not None])))
        if not holds:
            continue
        alive[s] = False
        head[p], width[p], true[p] = head[s], km, tn
    fronts, front_of = [], {}
    for s in range(ns):
        if not alive[s]:
            continue
        top, lo = nodes[s], nodes[head[s]]
        rows = np.concatenate([np.arange(lo["col0"], top["col0"]), top["rows"]])
        for t in range(head[s], s + 1):
            front_of[t] = len(fronts)
        fronts.append(dict(k=width[s], f=len(rows), col0=lo["col0"], rows=rows, level=0, top=s,
                           members=[i for t in range(head[s], s + 1) for i in nodes[t]["members"]]))
        assert fronts[-1]["f"] == fronts[-1]["k"] + top["f"] - top["k"]
    for j, fr in enumerate(fronts):      # postorder: children before parents
        par = nodes[fr.pop("top")]["parent"]
        fr["parent"] = None if par is None else front_of[par]
        if par is not None:
            fronts[fr["parent"]]["level"] = max(fronts[fr["parent"]]["level"], fr["level"] + 1)
    return Merged(d, fronts, decisions, nnzL, nschur)


# ---------------------------------------------------------------------------------------------------------------------------------
# The catalogue: id -> (forest, relaxation options, what it is for).  The merging child of a node is its last one (largest CB).

def _chain(shapes, *top_children):
    """A chain from (k, c) pairs written leaf to root; `top_children` hang beside the chain under its last node."""
    nd = None
    for i, (k, c) in enumerate(shapes):
        kids = ([] if nd is None else [nd]) + (list(top_children) if i == len(shapes) - 1 else [])
        nd = N(k, c, *kids)
    return nd


def _from_ft(name, purpose):
    return (ft.DESIGNS[name][0], DEFAULT_RELAX, purpose)


_UNDER_SEP = _chain([(20, 66), (20, 62), (20, 58), (20, 54), (20, 50), (31, 40)])

DESIGNS = {
    "mixed-level": _from_ft("mixed-level", "the 500 / 750 child merges into the 260 separator: (760, 760), three other children extend-add into it"),
    "mixed-level-scatter": _from_ft("mixed-level-scatter", "the same with non-contiguous extend-add behind 500 merged columns"),
    "fan-in-8": _from_ft("fan-in-8", "the last of eight children merges into the root: (550, 550)"),
    "deep-chain-6": _from_ft("deep-chain-6", "only the top pair merges: (500, 500)"),
    "edge-k385-c1": _from_ft("edge-k385-c1", "one (387, 387) front: just past the 384-column route boundary by amalgamation"),
    "edge-k1023-c128": _from_ft("edge-k1023-c128", "one (1152, 1152) front, a zero row under the child's 1023 columns: a padded second inverse block"),
    "small-classes-f32-33-64-65-128-129": _from_ft("small-classes-f32-33-64-65-128-129", "the last small front merges into the root: a (130, 130) big front"),
    "task-chains-under-big": _from_ft("task-chains-under-big", "chains of 8-column fronts collapse to (64, 80) and (48, 64)"),
    "forest-3-roots": _from_ft("forest-3-roots", "nothing merges across roots"),
    "always-64-65": ([N(40, 0, N(24, 10)), N(41, 0, N(24, 10))], DEFAULT_RELAX, "always clause: km = 64 merges at z = 0.346, km = 65 does not"),
    "small-frac-under-over": ([N(120, 0, N(120, 60)), N(72, 0, N(110, 34))], DEFAULT_RELAX,
                              "small clause, fraction edge: z = 0.2490 merges to (240, 240), z = 0.2510 does not"),
    "small-width-256-257": ([N(128, 0, N(128, 100)), N(129, 0, N(128, 101))], DEFAULT_RELAX,
                            "small clause, width edge: km = 256 merges at z = 0.109, km = 257 does not"),
    "any-frac-under-over": ([N(380, 0, N(250, 357)), N(320, 0, N(200, 299))], DEFAULT_RELAX,
                            "any clause: z = 0.0289 merges to (630, 630), the explicit-inverse route; z = 0.0310 does not"),
    "chain-6x20": ([_chain([(20, 110), (20, 105), (20, 100), (20, 95), (20, 90), (91, 0)])], DEFAULT_RELAX,
                   "five transitive merges through widths 40 .. 100 to one (191, 191) big front made of small fronts"),
    "chain-under-sep": ([N(70, 0, N(12, 9, scatter=True), N(30, 20), _UNDER_SEP)], DEFAULT_RELAX,
                        "the chain merges to 60 columns, is refused at 80 (z = 0.254), restarts, merges to 71, is refused into the separator"),
    "mid-clause": ([N(12, 0, N(12, 6)), N(13, 0, N(12, 6)), N(20, 0, N(20, 17)), N(10, 0, N(4, 3)), N(10, 0, N(30, 9))], MID_RELAX,
                   "options of its own so that the mid clause decides: width edge 24 | 25"),
    "mid-frac-over": ([N(12, 0, N(8, 2))], MID_RELAX, "mid clause open (km = 20) and refused at z = 0.381: the far side of mid_frac"),
    "task-chains-only": ([N(17, 0, ft._chain_small(6), ft._chain_small(8))], DEFAULT_RELAX,
                         "the chain subtrees of task-chains-under-big alone: all fronts small after merging (batches)"),
}

# which designs the GPU file runs where.  mid-frac-over is in the catalogue for its one refused decision (the analysis, on the host):
# two fronts of 10 and 12 rows, nothing merged, n = 20 -- nothing for the numeric phase that mid-clause does not have
GPU_DESIGNS = [name for name in DESIGNS if name != "mid-frac-over"]
EXPLICIT_INVERSE = ["mixed-level", "mixed-level-scatter", "fan-in-8", "deep-chain-6", "edge-k385-c1", "edge-k1023-c128", "any-frac-under-over"]
PROMISE_DESIGNS = ["mixed-level-scatter", "chain-under-sep", "chain-6x20", "small-frac-under-over", "edge-k385-c1"]
BATCH_DESIGNS = ["always-64-65", "mid-clause", "task-chains-only"]
VARIANT_DESIGNS = ["mixed-level", "fan-in-8", "edge-k1023-c128", "chain-under-sep"]
SCHUR_DESIGN, SCHUR_SIZES = "deep-chain-6", (100, 300, 310)
# a leaf (k, c) of a merged chain per design: where the sparse right-hand sides sit
CHAIN_LEAF = {"mixed-level-scatter": (500, 250), "chain-under-sep": (20, 66), "chain-6x20": (20, 110), "small-frac-under-over": (120, 60),
              "edge-k385-c1": (385, 1), "deep-chain-6": (200, 290), "task-chains-under-big": (8, 16)}


def design(name, values="plain", seed=0):
    """(ft.build result, the handle's relaxation options, model) of a catalogue entry.  A design at the defaults gives the handle no
    option: the library's own defaults are then part of what is tested against the model's DEFAULT_RELAX."""
    roots, opts, _ = DESIGNS[name]
    d = ft.build(roots, values=values, seed=seed)
    return d, ({} if opts is DEFAULT_RELAX else dict(opts)), merged(d, opts)
