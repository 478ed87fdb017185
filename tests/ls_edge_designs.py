"""Designed inputs of the step-side vector kernels (csrc/ls_device.h, linesearch.hip, ls_batch.hip) at the sizes
where a map-reduce goes wrong.  No GPU and no library call in here; test_ls_edge_designs_host.py checks what is claimed below.

Structure W(N): n = m = N, H diagonal, row i of J holds one entry, in column i.  K of the symmetric kind is N independent 2 x 2 blocks, Q
of the Schur kind is diagonal; J dx, J'w and H dx are one product per entry.

The partition of a launch over `len` entries: nb = min(256, ceil(len / 1024)) workgroups of 256 threads, thread t of workgroup b takes
the entries b * 256 + t + j * (nb * 256), j = 0, 1, ...; partial row b of nb; one workgroup folds the rows.

Two tiers of values:
  random   N in RANDOM_N: s, y in [0.5, 2], dx, dy, ds, grad normal (clipped to +-4, no exact zero in dy), fractions in [0.05, 0.3], J
           and H entries in +-[0.5, 2].  Sums are compared within a rounding bound (ls_exact.py).
  dyadic   N in DYADIC_N: 261121 = 255 * 1024 + 1 is the first length with 256 workgroups, 262144 gives every thread exactly four
           entries, 262145 gives one thread a fifth, 600001 is ragged in the third stride.  s, the penalty parameter, the step sizes, the
           scales and the entries of J are powers of two; y, mu, dx, dy, ds, grad, H, s_cand, y_cand are small integers over 8 or 16:
           every product and every partial sum in any order is exact (ls_exact.Dy proves it in integer arithmetic), so the sums are
           compared as bits.

Planted entries, one position at a time (positions(N)): every plant is a unique deciding entry whose runner-up is at least a factor of
two away, so a launch that loses the entry reports something unmistakably different.  Plants that touch different inputs share a case:
  group "a": ratio_s    ds = -64 s            the ratio that decides max_step_primal (the others stay below 12)
             s_bound    s_new = half its bound the single row that fails s_bound_ok
             lb         dy = 1/2, y_cand = -1  the only positive candidate of dual_bounds' lower bound (about 2; the start is 0)
             dx         2 max|dx|              the unique maximum of |dx|
             comp       y = 32                 the unique maximum of |comp| (at least 15.6; the others stay below 4)
  group "b": ub         dy = -1/2, y_cand = -1 the only negative candidate of dual_bounds' upper bound (about -2; the others are positive)
             comp_pred  ds = 512               the unique maximum of |comp_predicted| (at least 44; the others stay below 20.5)
  group "c": lb_y       dy = -64 y_cand        the ratio that decides simple_max_step(y_cand, dy, lb_y) (the others stay below 27)
  reset      dy = 0 (or -0.0), y_cand = -1 at the position: dual_bounds' interval restarts at (0, -1).  Two rows before it hold candidates
             that must not count (lb about 4, ub about -4), two rows behind it candidates that must (lb about 2, ub about -2).
  NaN        group "n1": ds and y_cand, "n2": y, "n3": dy, "n4": dx -- every channel that propagates NaN sees one at the position.
"""
import dataclasses
import functools
import math

import numpy as np
import scipy.sparse as sp

RANDOM_N = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
DYADIC_N = (261121, 262144, 262145, 600001)
GROUPS = {"a": ("ratio_s", "s_bound", "lb", "dx", "comp"), "b": ("ub", "comp_pred"), "c": ("lb_y",)}
NAN_GROUPS = {"n1": ("ds", "y_cand"), "n2": ("y",), "n3": ("dy",), "n4": ("dx",)}
COMP_FEAS = 0.01
EX = 0.5
PER_ENTRY = ("H", "J", "s", "y", "grad", "dx", "dy", "ds", "frac_predict", "frac", "s_new", "s_cand", "y_cand", "grad_cand", "J_cand")


def nb(length):
    """Workgroups of a map-reduce launch over `length` entries."""
    return min(256, -(-length // 1024))


def stride(length):
    return nb(length) * 256


def serial_adds(length):
    """The most entries one thread folds: ceil(length / (nb * 256))."""
    return -(-length // stride(length))


def positions(N):
    """0 and N - 1; the last entry of the first stride and the first of the second; the largest multiple of the stride below N and the
    entry before it; 262144 (the first entry any thread takes in a fifth iteration) -- where they lie inside 0 .. N - 1."""
    st = stride(N)
    last = ((N - 1) // st) * st
    cand = [0, N - 1, st - 1, st, last, last - 1, 262144]
    return sorted({p for p in cand if 0 <= p < N})


@dataclasses.dataclass
class Case:
    """One iterate on W(N), one direction and the inputs of one round of the five step-side functions."""
    tier: str
    N: int
    H: np.ndarray            # the diagonal of H
    J: np.ndarray            # entry (i, i) of J
    s: np.ndarray
    y: np.ndarray
    mu: float
    pen: float
    grad: np.ndarray
    dx: np.ndarray
    dy: np.ndarray
    ds: np.ndarray
    dmu: float
    frac_predict: np.ndarray
    frac: np.ndarray
    s_new: np.ndarray        # s_bound_ok's candidate
    s_cand: np.ndarray       # dual_step_range's and dual_step's candidate
    y_cand: np.ndarray
    mu_cand: float
    grad_cand: np.ndarray
    J_cand: np.ndarray
    scale_D: float
    scale_mu: float
    steps: tuple             # the step sizes of predicted_reduction
    planted: tuple = ()      # (what, position)

    def copy(self, **kw):
        c = dataclasses.replace(self, **kw)
        for f in PER_ENTRY:
            setattr(c, f, getattr(c, f).copy())
        return c


@functools.lru_cache(maxsize=None)
def _pattern(N):
    return np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32)


def diag_matrix(N, data):
    """An N x N CSC matrix with `data` on its diagonal: H (lower-stored) and J of W(N).  The index arrays are one object per N."""
    ptr, idx = _pattern(N)
    return sp.csc_matrix((np.ascontiguousarray(data, dtype=float), idx, ptr), shape=(N, N))


def iterate(c, Iterate):
    return Iterate(x=np.zeros(c.N), y=c.y, s=c.s, mu=c.mu, J=diag_matrix(c.N, c.J), H=diag_matrix(c.N, c.H), grad=c.grad, cons=c.s.copy(),
                   a_norm_penalty_par=c.pen)


def _signs(rng, N):
    return rng.integers(0, 2, size=N) * 2.0 - 1.0


def base_random(N, big_dx, seed=0):
    """The random tier's case; big_dx: norm(dx, Inf) = 2.5, else 0.6 (the two branches of min(1, |dx|_inf))."""
    rng = np.random.default_rng(10 * N + seed)
    u = lambda lo, hi: rng.uniform(lo, hi, size=N)
    normal = lambda: np.clip(rng.normal(size=N), -4.0, 4.0)
    s, y = u(0.5, 2.0), u(0.5, 2.0)
    dx = normal()
    dx = dx / np.max(np.abs(dx)) * (2.5 if big_dx else 0.6)
    dy = normal()
    dy[np.abs(dy) < 1e-3] = 0.5
    grad = normal()
    J = _signs(rng, N) * u(0.5, 2.0)
    return Case(tier="random", N=N, H=_signs(rng, N) * u(0.5, 2.0), J=J, s=s, y=y, mu=0.137 + 0.01 * seed, pen=1.3e-4, grad=grad, dx=dx, dy=dy, ds=normal(),
                dmu=-0.05, frac_predict=u(0.05, 0.3), frac=u(0.05, 0.3), s_new=s * u(0.6, 1.5), s_cand=s * u(0.6, 1.5), y_cand=y * u(0.6, 1.5),
                mu_cand=0.09, grad_cand=grad + 0.03, J_cand=J * 1.02, scale_D=0.7, scale_mu=1.3, steps=(1.0, 0.37))


def base_dyadic(N, item=0):
    """The dyadic tier's case; `item` changes the values (the three items of the batch test)."""
    rng = np.random.default_rng(7 * N + item)
    ints = lambda lo, hi: rng.integers(lo, hi + 1, size=N).astype(float)
    pow2 = lambda: 2.0 ** rng.integers(-1, 2, size=N)
    s = pow2()
    dy = _signs(rng, N) * ints(1, 16) / 8.0
    grad = ints(-16, 16) / 8.0
    J = _signs(rng, N) * pow2()
    s_cand = ints(4, 16) / 8.0
    return Case(tier="dyadic", N=N, H=_signs(rng, N) * ints(4, 16) / 8.0, J=J, s=s, y=ints(4, 16) / 8.0, mu=(3.0 + item) / 8.0, pen=0.125, grad=grad,
                dx=ints(-16, 16) / 8.0 / (1.0 if item % 2 == 0 else 4.0), dy=dy, ds=ints(-16, 16) / 8.0, dmu=-0.125, frac_predict=2.0 ** rng.integers(-3, -1, size=N),
                frac=2.0 ** rng.integers(-3, -1, size=N), s_new=s_cand.copy(), s_cand=s_cand, y_cand=ints(8, 16) / 8.0, mu_cand=(5.0 + item) / 16.0,
                grad_cand=grad + 0.25, J_cand=_signs(rng, N) * pow2(), scale_D=0.5, scale_mu=2.0, steps=(1.0, 0.25))


def thres(c):
    """lb_s_thres's scalar norm(dx, Inf) * norm(dx, Inf)^ex (NaN propagates)."""
    nx = float(np.max(np.abs(c.dx))) if not np.isnan(c.dx).any() else math.nan
    return nx * math.pow(nx, EX)


def _plant_one(c, what, p):
    if what == "ratio_s":
        c.ds[p] = -64.0 * c.s[p]
    elif what == "s_bound":
        pass                                           # after dx: the bound depends on norm(dx, Inf)
    elif what == "lb":
        c.dy[p], c.y_cand[p] = 0.5, -1.0
    elif what == "ub":
        c.dy[p], c.y_cand[p] = -0.5, -1.0
    elif what == "lb_y":
        c.dy[p] = -64.0 * c.y_cand[p]
    elif what == "dx":
        c.dx[p] = -2.0 * np.max(np.abs(c.dx))
    elif what == "comp":
        c.y[p] = 32.0
    elif what == "comp_pred":
        c.ds[p] = 512.0
    else:
        raise KeyError(what)


def plant(base, group, p):
    """The plants of GROUPS[group] at position p of a copy of `base`."""
    c = base.copy(planted=tuple((w, p) for w in GROUPS[group]))
    for w in GROUPS[group]:
        _plant_one(c, w, p)
    if "s_bound" in GROUPS[group]:
        c.s_new[p] = 0.5 * (c.frac[p] * min(c.s[p], thres(c)))
    return c


def plant_reset(base, p, negative_zero=False):
    """A reset row at p; candidates that must not count at p - 2 (ub) and p - 1 (lb), candidates that must at p + 1 (lb) and p + 2 (ub)."""
    c = base.copy(planted=(("reset", p),))
    N = c.N
    for q, d, in ((p - 2, -0.25), (p - 1, 0.25), (p + 1, 0.5), (p + 2, -0.5)):
        if 0 <= q < N:
            c.dy[q], c.y_cand[q] = d, -1.0
    c.dy[p], c.y_cand[p] = (-0.0 if negative_zero else 0.0), -1.0
    return c


def plant_nan(base, group, p):
    c = base.copy(planted=tuple(("nan_" + f, p) for f in NAN_GROUPS[group]))
    for f in NAN_GROUPS[group]:
        getattr(c, f)[p] = math.nan
    return c


def without(c, p):
    """The case without entry p (length N - 1): what a launch that loses the entry computes."""
    d = dataclasses.replace(c, N=c.N - 1, planted=())
    for f in PER_ENTRY:
        setattr(d, f, np.delete(getattr(c, f), p))
    return d


def edge_cases(base):
    """Every planted case of a base case: [(label, case)]."""
    out = []
    for p in positions(base.N):
        out += [(f"{g}@{p}", plant(base, g, p)) for g in GROUPS]
        out.append((f"reset@{p}", plant_reset(base, p)))
        out += [(f"{g}@{p}", plant_nan(base, g, p)) for g in NAN_GROUPS]
    out.append((f"reset-0.0@{base.N - 1}", plant_reset(base, base.N - 1, negative_zero=True)))
    return out
