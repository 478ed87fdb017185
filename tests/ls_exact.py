"""Exact references of the step-side vector kernels (csrc/ls_device.h, linesearch.hip, ls_batch.hip, ls_finish.h) on the cases of
ls_edge_designs.py, with the rounding bound each device sum must meet.  Conventions of kkt_exact.py: err / bound per value, a value
passes at <= 1.

Max / min channels and the 0 / 1 test: every entry is a few IEEE operations on the inputs, written here operation by operation as the map
is (the kernels are compiled with -ffp-contract=off), so numpy gives the device's bits; the reduction is Julia's: a NaN anywhere gives
NaN, otherwise the maximum / minimum with the channel's start value.  Compared as bits (same_bits: any NaN equals any NaN).

Sum channels: the exact value is the sum of the exact terms of the double inputs -- fractions.Fraction in the random tier, integers in
the dyadic tier (Dy: int64 numerators over one power of two; every intermediate and len * max|term| stay below 2^53, so every product,
quotient and partial sum in any order is a double and the device's sum is the exact one, bit for bit).

Bound of a sum channel in the random tier: gamma(k) * sum |pieces|, pieces = the un-cancelled pieces of the terms, k = the roundings on
the longest path from an input to the result:
    k = (roundings of the map, derived next to each channel below) + reduce_roundings(len)
    reduce_roundings(len) = ceil(len / (nb * 256))   serial additions of a thread (the first, to 0.0, is exact but counted)
                          + 8                        tree levels in the workgroup
                          + ceil(nb / 256) + 8       the final pass: one serial addition per thread, 8 tree levels
"""
import dataclasses
import math
from fractions import Fraction

import numpy as np

import ls_edge_designs as D
from kkt_exact import SLACK, U, F, _ratio, assert_within, gamma  # noqa: F401

NAN = math.nan


def same_bits(a, b):
    """a and b are the same double (NaN: both NaN; zeros: the same sign)."""
    a, b = float(a), float(b)
    if a != a or b != b:
        return a != a and b != b
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


def reduce_roundings(length):
    return D.serial_adds(length) + 8 + -(-D.nb(length) // 256) + 8


# ---- Julia's reductions -----------------------------------------------------------------------------------------------------------------
def jl_max(init, v):
    if len(v) == 0:
        return init
    return NAN if np.isnan(v).any() or init != init else max(init, float(np.max(v)))


def jl_min(init, v):
    if len(v) == 0:
        return init
    return NAN if np.isnan(v).any() or init != init else min(init, float(np.min(v)))


def _jmin2(a, b):
    return NAN if (a != a or b != b) else min(a, b)


def _quiet():
    return np.errstate(divide="ignore", invalid="ignore", over="ignore")


# ---- max / min channels -----------------------------------------------------------------------------------------------------------------
def dx_norm(c):
    return jl_max(0.0, np.abs(c.dx))                                  # MapAbs


def thres_scalar(nx):
    return nx * math.pow(nx, D.EX)                                    # ls_finish.h: the host's libm pow


def primal_ratio(c):
    """maximum([1; -ds ./ (s - frac .* min.(s, thr))]) (MapRatioS)."""
    thr = thres_scalar(dx_norm(c))
    with _quiet():
        lb = c.frac_predict * np.minimum(c.s, thr)
        return jl_max(1.0, -c.ds / (c.s - lb))


def max_step_primal(c):
    """(step_size_P, norm(dx, Inf))."""
    with _quiet():
        return float(np.float64(1.0) / np.float64(primal_ratio(c))), dx_norm(c)


def s_bound_ok(c):
    thr = thres_scalar(dx_norm(c))
    with _quiet():
        return bool(np.all(c.s_new >= c.frac * np.minimum(c.s, thr)))     # MapSBound, reduced with min: NaN compares false


def dual_channels(c):
    """(lb, ub, last reset or -1, ratio of lb_y) as the launches of okkt_kkt_dual_step_range leave them (MapDualBounds), before
    dual_range_finish: the candidates of the rows behind the last reset, the ratio over all rows."""
    s, d, yc = c.s_cand, c.dy, c.y_cand
    nxmin = _jmin2(1.0, dx_norm(c))
    with _quiet():
        ub_dy = c.mu_cand / (D.COMP_FEAS * s * d) - yc / d
        lb_dy = c.mu_cand * D.COMP_FEAS / (s * d) - yc / d
        a = np.where(d > 0.0, lb_dy * 1.001 + 0.0, np.where(d < 0.0, ub_dy * 1.001 + 0.0, -np.inf))
        b = np.where(d > 0.0, ub_dy / 1.001 - 0.0, np.where(d < 0.0, lb_dy / 1.001 - 0.0, np.inf))
        reset = np.nonzero((d == 0.0) & ((lb_dy >= 0.0) | (ub_dy <= 0.0)))[0]
        ratio = jl_max(1.0, -d / (yc - c.frac * c.y * nxmin))
    after = int(reset[-1]) if len(reset) else -1
    return jl_max(0.0, a[after + 1:]), jl_min(-1.0 if after >= 0 else 1.0, b[after + 1:]), after, ratio


def dual_step_range(c):
    lb, ub, _, ratio = dual_channels(c)
    if not (math.isfinite(lb) and math.isfinite(ub)):
        lb, ub = 0.0, -1.0
    with _quiet():
        return lb, _jmin2(ub, float(np.float64(1.0) / np.float64(ratio)))


def comp_norms(c, step):
    """(|comp|_inf, |comp_predicted|_inf) (MapPredM channels 1, 2)."""
    mu_new = c.mu + c.dmu * step
    with _quiet():
        C_k = jl_max(0.0, np.abs(c.s * c.y - c.mu))
        P_k = jl_max(0.0, np.abs(c.s * c.y + c.dy * c.s * step + c.ds * c.y * step - mu_new))
    return C_k, P_k


# ---- the sum channels in an exact arithmetic -------------------------------------------------------------------------------------------
class Dy:
    """num * 2^-exp with integer num (an int64 array or a Python int): the dyadic tier's exact arithmetic.  Every value built stays below
    2^53 in magnitude, i.e. is a double."""
    LIMIT = 2 ** 53

    def __init__(self, num, exp):
        self.num, self.exp = num, exp
        assert self.peak() < Dy.LIMIT, "not representable as a double"

    def peak(self):
        return int(np.max(np.abs(self.num))) if np.size(self.num) else 0

    @staticmethod
    def of(x):
        x = np.asarray(x, dtype=float)
        for e in range(0, 40):
            v = x * 2.0 ** e
            if np.all(v == np.rint(v)):
                return Dy(v.astype(np.int64) if x.ndim else int(v), e)
        raise AssertionError("not a small dyadic number")

    @staticmethod
    def recip(x):
        m, _ = np.frexp(np.asarray(x, dtype=float))
        assert np.all(m == 0.5), "a quotient by something that is no power of two"
        return Dy.of(1.0 / np.asarray(x, dtype=float))

    def _align(self, o):
        e = max(self.exp, o.exp)
        return self.num * 2 ** (e - self.exp), o.num * 2 ** (e - o.exp), e

    def __add__(self, o):
        a, b, e = self._align(o)
        return Dy(a + b, e)

    def __sub__(self, o):
        a, b, e = self._align(o)
        return Dy(a - b, e)

    def __mul__(self, o):
        assert self.peak() < 2 ** 26 and o.peak() < 2 ** 26          # no int64 overflow before the check of the product
        return Dy(self.num * o.num, self.exp + o.exp)

    def __neg__(self):
        return Dy(-self.num, self.exp)

    def __abs__(self):
        return Dy(np.abs(self.num), self.exp)

    def total(self):
        """The exact sum, with the proof that every partial sum in any order is a double: len * max|term| < 2^53."""
        assert np.size(self.num) * self.peak() < Dy.LIMIT
        return Fraction(int(np.sum(self.num)), 2 ** self.exp)


class _FracArith:
    @staticmethod
    def lift(x):
        x = np.asarray(x, dtype=float)
        return np.array([Fraction(v) for v in x.tolist()], dtype=object) if x.ndim else Fraction(float(x))

    @staticmethod
    def recip(x):
        return np.array([1 / Fraction(v) for v in np.asarray(x, dtype=float).tolist()], dtype=object)

    @staticmethod
    def total(t):
        return sum(t.tolist(), Fraction(0))


class _DyArith:
    lift = staticmethod(Dy.of)
    recip = staticmethod(Dy.recip)

    @staticmethod
    def total(t):
        return t.total()


# roundings of the maps, per channel (the longest path from an input to the term):
#   pred_m0 = v v (y / s), v = J dx:       v carries 1 and enters twice (2), v v (1), y / s (1), the product (1)                       = 5
#   pred_n0 = dx (grad - J'w):             w = mu / s + (-(mu pen)): the division or the product mu pen (1), the addition (1);
#                                          J'w one product (1); grad - J'w (1); dx (.) (1)                                          = 5
#   pred_n1 = dx (H dx):                   H dx = (v1 + v2) - diag x with v1 = v2 = fl(h x): exactly fl(h x) when evaluated as written,
#                                          fl(2 fl(h x) - h x) when the compiler fuses the last product (kkt.hip is compiled with
#                                          contraction on): at most 3; dx (.) (1)                                                   = 4
#   dual_n0 = res q:                       q = scale_D (Jc'dy): 2.  res = scale_D (grad - Jc'(y_cand + (-(mu pen)))): mu pen (1),
#                                          the addition (1), Jc'(.) (1), grad - (.) (1), scale_D (.) (1): 5.  res q (1)              = 8
#   dual_n1 = q q:                         2 + 2 + 1                                                                              = 5
#   dual_m0 = res q:                       q = (scale_mu s_cand) dy: 2.  res = -scale_mu (s_cand y_cand - mu): 3.  res q (1)       = 6
#   dual_m1 = q q:                         2 + 2 + 1                                                                              = 5
MAP_ROUNDINGS = {"pred_m0": 5, "pred_n0": 5, "pred_n1": 4, "dual_n0": 8, "dual_n1": 5, "dual_m0": 6, "dual_m1": 5}


def _terms(c, A):
    """channel -> (terms, pieces) in the arithmetic A; pieces are the un-cancelled pieces: |dx| (|grad| + |J'w|), not |dx| |grad - J'w|."""
    clean = lambda v: np.nan_to_num(np.asarray(v, dtype=float), nan=0.0)
    L = lambda v: A.lift(clean(v))
    rs = A.recip(clean(c.s))
    J, H, y, dx, dy, grad = L(c.J), L(c.H), L(c.y), L(c.dx), L(c.dy), L(c.grad)
    mu, pen = L(c.mu), L(c.pen)
    out = {}
    v = J * dx
    t = v * v * (y * rs)
    out["pred_m0"] = (t, abs(t))
    w_pieces = abs(mu * rs) + abs(mu * pen)
    out["pred_n0"] = (dx * (grad - J * (mu * rs - mu * pen)), abs(dx) * (abs(grad) + abs(J) * w_pieces))
    t = dx * (H * dx)
    out["pred_n1"] = (t, abs(t))
    Jc, yc, sc, gc = L(c.J_cand), L(c.y_cand), L(c.s_cand), L(c.grad_cand)
    muc, sD, sM = L(c.mu_cand), L(c.scale_D), L(c.scale_mu)
    q = sD * (Jc * dy)
    res = sD * (gc - Jc * (yc - muc * pen))
    out["dual_n0"] = (res * q, abs(q) * (abs(sD) * (abs(gc) + abs(Jc) * (abs(yc) + abs(muc * pen)))))
    out["dual_n1"] = (q * q, q * q)
    qm = sM * sc * dy
    resm = -(sM * (sc * yc - muc))
    out["dual_m0"] = (resm * qm, abs(qm) * (abs(sM) * (abs(sc * yc) + abs(muc))))
    out["dual_m1"] = (qm * qm, qm * qm)
    return out


def _float_nan(c):
    """The channels whose sum is NaN (a NaN input reaches them), from a plain numpy evaluation."""
    with _quiet():
        q = c.scale_D * (c.J_cand * c.dy)
        res = c.scale_D * (c.grad_cand - c.J_cand * (c.y_cand - c.mu_cand * c.pen))
        qm = c.scale_mu * c.s_cand * c.dy
        resm = -c.scale_mu * (c.s_cand * c.y_cand - c.mu_cand)
        v = c.J * c.dx
        t = {"pred_m0": v * v * (c.y / c.s), "pred_n0": c.dx * (c.grad - c.J * (c.mu / c.s - c.mu * c.pen)), "pred_n1": c.dx * (c.H * c.dx),
             "dual_n0": res * q, "dual_n1": q * q, "dual_m0": resm * qm, "dual_m1": qm * qm}
    return {k for k, a in t.items() if not np.isfinite(a).all()}


def _restrict(c, idx):
    d = dataclasses.replace(c, N=len(idx))
    for f in D.PER_ENTRY:
        setattr(d, f, getattr(c, f)[idx])
    return d


def _totals(c, A):
    """channel -> (sum of the terms, sum of the pieces, (max |numerator|, exponent) in the dyadic tier)."""
    out = {}
    for name, (t, p) in _terms(c, A).items():
        out[name] = (A.total(t), A.total(p), (t.peak(), t.exp) if A is _DyArith else None)
    return out


def sums(c, near=None):
    """channel -> (exact sum or None where the sum is NaN, sum |pieces|, k): Fraction in the random tier, integers in the dyadic tier
    (every assertion of Dy holds on the way: that is the proof of exactness).  near = (case, its sums): a case of the same scalars that
    differs from c in a few entries -- only those entries are evaluated again, and their terms replace the other case's in its sums."""
    A = _DyArith if c.tier == "dyadic" else _FracArith
    ks = {name: MAP_ROUNDINGS[name] + reduce_roundings(c.N) for name in MAP_ROUNDINGS}
    if near is None:
        assert not _float_nan(c), "a NaN case needs the case it was planted in"
        tot = _totals(c, A)
        out = {name: (tot[name][0], tot[name][1], ks[name]) for name in ks}
        out["_proof"] = {name: tot[name][2] for name in ks}
    else:
        b, Sb = near
        assert (b.tier, b.N, b.mu, b.pen, b.mu_cand, b.scale_D, b.scale_mu) == (c.tier, c.N, c.mu, c.pen, c.mu_cand, c.scale_D, c.scale_mu)
        diff = np.zeros(c.N, dtype=bool)
        for f in D.PER_ENTRY:
            u, v = getattr(c, f), getattr(b, f)
            diff |= ~((u == v) | ((u != u) & (v != v)))
        idx = np.nonzero(diff)[0]
        cs, bs = _restrict(c, idx), _restrict(b, idx)
        nan = _float_nan(cs)
        new, old = _totals(cs, A), _totals(bs, A)
        out = {"_proof": {}}
        for name in ks:
            out[name] = (None, None, ks[name]) if name in nan else (Sb[name][0] - old[name][0] + new[name][0], Sb[name][1] - old[name][1] + new[name][1], ks[name])
            if A is _DyArith:
                (p0, e0), (p1, e1) = Sb["_proof"][name], new[name][2]
                e = max(e0, e1)
                out["_proof"][name] = (max(p0 * 2 ** (e - e0), p1 * 2 ** (e - e1)), e)
    if A is _DyArith:          # every partial sum in any order is a double: len * max|term| < 2^53 in units of the finest term
        assert all(c.N * peak < Dy.LIMIT for peak, _ in out["_proof"].values())
    return out


# ---- ls_finish.h in exact arithmetic -------------------------------------------------------------------------------------------------
def predicted(c, step, S=None):
    """okkt_kkt_predicted_reduction at `step`: dict(C_k, P_k: doubles, compared as bits; phi, merit: (exact Fraction or None for NaN,
    bound)).  phi = step rn0 + step step 0.5 (rn1 + rm0): the path of rn0 takes 2 more roundings (the product, the last addition), that
    of rn1 and rm0 5 (their sum, step step, times 0.5, the product, the last addition).  merit = phi + (P^3 - C^3) / mu^2 from the exact
    channel values C, P: the cubes (2), the difference (1), mu mu or the quotient (1 + 1 on one path: the denominator's roundings count
    on every piece), the last addition (1): 6 on |P|^3 + |C|^3 over mu^2, one more on phi's pieces."""
    S = S or sums(c)
    C_k, P_k = comp_norms(c, step)
    st = Fraction(step)
    parts = [S["pred_n0"], S["pred_n1"], S["pred_m0"]]
    if any(p[0] is None for p in parts):
        phi, phi_b, merit, merit_b = None, None, None, None
    else:
        (n0, pn0, k0), (n1, pn1, k1), (m0, pm0, km) = parts
        phi = st * n0 + st * st / 2 * (n1 + m0)
        k = max(k0 + 2, max(k1, km) + 5)
        pieces = abs(st) * pn0 + st * st / 2 * (pn1 + pm0)
        phi_b = gamma(k) * float(pieces)
        if C_k != C_k or P_k != P_k:
            merit, merit_b = None, None
        else:
            cubes = (F(P_k) ** 3 - F(C_k) ** 3) / F(c.mu) ** 2
            merit = phi + cubes
            merit_b = gamma(k + 1) * float(pieces) + gamma(6) * float((F(P_k) ** 3 + F(C_k) ** 3) / F(c.mu) ** 2)
    return dict(C_k=C_k, P_k=P_k, phi=(phi, phi_b), merit=(merit, merit_b))


def dual_step(c, lb, ub, step_size_P, dual_ls, S=None):
    """step_size_D of okkt_kkt_dual_step: (exact value or None for NaN, bound).  dual_ls outside (1, 3): ub itself, bound 0.
    sd = (rn0 + rm0) / (rn1 + rm1), then min with ub and max with the small step.  Every piece of the numerator passes its own k roundings
    and the addition of the two sums (1); the denominator's terms are squares, so its computed value is the exact one times
    (1 + theta) with at most max(k) + 1 roundings, which reach every piece of the quotient; the division (1): gamma(k_num + k_den + 3)
    on sum |pieces of the numerator| over the exact denominator.  The clamps select, they do not round, and do not widen a difference.
    The four raw sums are no output of the entry point: with the clamps open (lb = step_size_P = -Inf, ub = Inf) the quotient itself comes
    back, and with scale_mu = 0 or scale_D = 0 the quotient of the two n sums or of the two m sums alone."""
    small = max(lb, min(ub, step_size_P))
    if dual_ls not in (1, 3):
        return F(ub), 0.0
    S = S or sums(c)
    (n0, pn0, k0), (n1, _, k1), (m0, pm0, k2), (m1, _, k3) = S["dual_n0"], S["dual_n1"], S["dual_m0"], S["dual_m1"]
    if any(v is None for v in (n0, n1, m0, m1)) or n1 + m1 == 0:
        return None, None
    den = n1 + m1
    sd = (n0 + m0) / den
    bound = gamma(max(k0, k2) + max(k1, k3) + 3) * float((pn0 + pm0) / den)
    if math.isfinite(ub):
        sd = min(sd, F(ub))                    # jl_min(sd, ub), then jl_max(., small_step): ls_finish.h's order
    if math.isfinite(small):
        sd = max(sd, F(small))
    return sd, bound


def exactly(fr):
    """The double that equals the Fraction (the dyadic tier: the value must be representable)."""
    v = float(fr)
    assert Fraction(v) == fr, "the exact value is not a double"
    return v
