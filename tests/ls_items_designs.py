"""The designed batches of the line-search batch tests (okkt_kkt_items_max_step_primal ...): item families on one
structure, designed directions whose dual_bounds reset in some items and not in others, and the inputs of one line-search round.  No GPU
and no library call in here; test_ls_items_host.py checks what is claimed below with numpy and the oracle.

Families (every one holds items that differ in s, y, mu, grad, the penalty parameter and the direction):
  d37     lanczos_ref.indefinite_design(37, lam): n = 37, m = 17 -- fewer entries than one workgroup; H differs from item to item
  banded  tridiagonal H, row i of J with three consecutive columns from floor(i (n - 2) / m); n = 1100, m = 2100: two workgroups per
          item for the sums over n, three for those over m; H and J are one object for every item (they go in with stride 0)
  chain   synth.hanging_chain(N_h = 520): m = 1046, n = 1042, two workgroups of which the second is almost empty (symmetric kind only)
"""
import dataclasses
import functools
import math

import numpy as np
import scipy.sparse as sp

import lanczos_ref as R
from onephase_jl_amd import synth

LAMS37 = (0.5, -4e-4, -3.7, -2.0)
# the shift every item of a family is factorised with (a direction exists whatever the inertia, as in the reference)
DELTA = {"d37": 5.0, "banded": 0.5, "chain": 1.0}
KINDS = {"d37": ("schur", "symmetric"), "banded": ("schur", "symmetric"), "chain": ("symmetric",)}
SIZES = {"d37": (37, 17), "banded": (1100, 2100), "chain": (1042, 1046)}
# what the designed direction of item b does (b modulo the length)
ROLES = ("plain", "reset_mid", "reset_last", "nan_ds", "nonfinite", "plain")


@functools.lru_cache(maxsize=None)
def _banded():
    n, m = SIZES["banded"]
    rng = np.random.default_rng(41)
    H = sp.diags([rng.uniform(2.0, 4.0, size=n), rng.uniform(-0.5, 0.5, size=n - 1)], [0, -1], format="csc")
    rows, cols = [], []
    for i in range(m):
        c0 = (i * (n - 2)) // m
        rows += [i, i, i]; cols += [c0, c0 + 1, c0 + 2]
    J = sp.csc_matrix((rng.uniform(-0.5, 0.5, size=3 * m), (rows, cols)), shape=(m, n))
    J.sort_indices()
    return H, J, rng.uniform(0.5, 2.0, size=m), rng.uniform(0.5, 2.0, size=m), 0.1


@functools.lru_cache(maxsize=None)
def _chain():
    p = synth.hanging_chain(N_h=520)
    assert (p["n"], p["m"]) == SIZES["chain"]
    return p["H"], p["J"], p["s"], p["y"], p["mu"]


def family(name, Iterate, B):
    """B iterates of the family on one structure."""
    its = []
    for b in range(B):
        rng = np.random.default_rng(1000 + b)
        if name == "d37":
            base = R.indefinite_design(Iterate, 37, LAMS37[b % 4])
            H, J, s0, y0, mu0 = base.H, base.J, base.s, base.y, base.mu
        else:
            H, J, s0, y0, mu0 = _banded() if name == "banded" else _chain()
        m, n = J.shape
        s = s0 * rng.uniform(0.5, 2.0, size=m)
        y = y0 * rng.uniform(0.5, 2.0, size=m)
        its.append(Iterate(x=np.zeros(n), y=y, s=s, mu=mu0 * (1.0 + 0.25 * b), J=J, H=H, grad=rng.normal(size=n) * (1.0 + b), cons=s + 0.1 * rng.normal(size=m),
                           a_norm_penalty_par=1e-4 * (1.0 + b)))
    return its


def reset_rows(role, m):
    """Rows with dy == 0 and y_cand < 0 (they reset dual_bounds' interval), and rows with dy == 0 and y_cand > 0 (NaN bounds: skipped)."""
    if role == "reset_mid":
        return [m // 3, (2 * m) // 3], [1, m // 2]
    if role == "reset_last":
        return [m // 4, m - 1], []
    return [], []


def designed_directions(its, Point):
    """(directions, y_cand) for okkt_kkt_items_set_direction, item b in the role ROLES[b % 6]:
      plain       no exact zero in dy
      reset_mid   two rows reset the interval in the middle of the vector, two more rows with dy == 0 do not (y_cand > 0 there)
      reset_last  the last reset sits at the final index (a -0.0 in dy)
      nan_ds      a NaN in ds (the primal step and |comp_predicted| are NaN, the dual range is not)
      nonfinite   y_cand = +Inf on a row with dy > 0: the bounds come out non-finite and fall back to (0, -1)
    norm(dx, Inf) is below 1 in the even items and above 1 in the odd ones (min(1, |dx|) takes both branches)."""
    dirs, ycands = [], []
    for b, it in enumerate(its):
        rng = np.random.default_rng(2000 + b)
        n, m = it.dim(), it.ncon()
        role = ROLES[b % len(ROLES)]
        dx = rng.uniform(-1.0, 1.0, size=n) * (0.3 if b % 2 == 0 else 2.5)
        dy = rng.normal(size=m)
        dy[np.abs(dy) < 1e-3] = 0.5
        ds = rng.normal(size=m)
        yc = it.y.copy()
        resets, skipped = reset_rows(role, m)
        for r in resets:
            dy[r] = 0.0
            yc[r] = -1.0 - 0.5 * b
        for r in skipped:
            dy[r] = 0.0
        if role == "reset_last":
            dy[m - 1] = -0.0
        if role == "nan_ds":
            ds[m // 2] = math.nan
        if role == "nonfinite":
            dy[m // 5] = abs(dy[m // 5]) + 0.1
            yc[m // 5] = math.inf
        dirs.append(Point(dx, dy, ds, mu=-0.5 * it.mu * (b + 1) / len(its)))
        ycands.append(yc)
    return dirs, ycands


@dataclasses.dataclass
class Round:
    """The inputs of one line-search round of item b that do not depend on an earlier output."""
    frac_predict: np.ndarray
    frac: np.ndarray
    alpha: float
    s_cand: np.ndarray
    y_cand: np.ndarray
    mu_cand: float
    grad_cand: np.ndarray
    J_scale: float
    scale_D: float
    scale_mu: float


def round_inputs(b, it, d, y_cand=None, alpha=None):
    """Item b's inputs at the step alpha: candidates s + alpha ds (kept positive, NaN stays NaN), y_cand (the iterate's y unless
    designed), mu + alpha dmu, a moved gradient, a Jacobian scaled by J_scale, and scales that differ from item to item."""
    rng = np.random.default_rng(3000 + b)
    m = it.ncon()
    alpha = 0.3 / (b + 1) if alpha is None else alpha
    s_cand = np.abs(it.s + alpha * d.s) + 1e-3
    return Round(frac_predict=rng.uniform(0.05, 0.3, size=m), frac=rng.uniform(0.05, 0.3, size=m), alpha=alpha, s_cand=s_cand,
                 y_cand=it.y.copy() if y_cand is None else y_cand, mu_cand=it.mu + alpha * d.mu, grad_cand=it.grad + 0.1 * alpha, J_scale=1.0 + 0.01 * (b + 1),
                 scale_D=0.7 + 0.1 * b, scale_mu=1.3 - 0.05 * b)
