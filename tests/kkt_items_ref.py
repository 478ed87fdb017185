"""The designed batches of the KKT-batch tests (okkt_kkt_items_*) and what the delta loop over their items must
return, predicted from the spectrum: no GPU and no library call in here.

The family is lanczos_ref.indefinite_design(Iterate, 37, lam) with the default seed: the generator draws nothing that depends on lam, so
every lam gives the same sparsity structure (and the same J, s, y, grad, cons); lam moves one entry of H, and with it lambda_min(Q(0)) = lam
for lam < 0.5.  lam = +0.5 is the convex item (Q(0) positive definite: one attempt at delta = 0), the negative ones need more and more
attempts.  An item's prediction is (status, num_fac, delta) from the attempt sequence of lanczos_ref.delta_sequence, the batch's
`launches` the largest num_fac of its items.
"""
import dataclasses
import functools

import numpy as np

import lanczos_ref as R

N = 37
LAMS = (0.5, -4e-4, -3.7, -900.0)
# delta_max below what item 3 (lam = -900) needs and above what the others need (lam = -3.7 succeeds at 16.78): item 3 alone ends with
# status 0.  With every previous delta 0 it does so in the last round (its attempt 134.2 > 100 is the eleventh); with the previous delta
# of DELTA_MAX_PREVS it passes delta_max at its fifth attempt (0, 0.637, 5.09, 40.7, 325.9) and leaves with its failed factor in its slot
# while item 2 goes on alone over a shorter item list and succeeds in round 10
DELTA_MAX_LOW = 100.0
DELTA_MAX_PREVS = (0.0, 0.0, 0.0, 2.0)


@functools.lru_cache(maxsize=None)
def spectrum(lam):
    """(diag_min, lambda_min) of Q(0) of the design."""
    Q = R.dense_q(R.indefinite_design(_Plain, N, lam))
    return float(np.min(np.diag(Q))), float(np.linalg.eigvalsh(Q)[0])


@dataclasses.dataclass
class _Plain:
    x: np.ndarray
    y: np.ndarray
    s: np.ndarray
    mu: float
    J: object
    H: object
    grad: np.ndarray
    cons: np.ndarray


def item(Iterate, lam, delta_prev=0.0):
    it = R.indefinite_design(Iterate, N, lam)
    it.delta = delta_prev
    return it


def batch(Iterate, lams, prevs=None):
    prevs = prevs if prevs is not None else [0.0] * len(lams)
    return [item(Iterate, lam, p) for lam, p in zip(lams, prevs)]


def sixteen():
    """B = 16: the four designs in a cycle, a nonzero delta_prev on half the items, alternating from cycle to cycle so that every design
    occurs with and without one."""
    lams = [LAMS[b % 4] for b in range(16)]
    prevs = [0.0 if (b + b // 4) % 2 == 0 else (2.0 if b % 4 in (1, 2) else 3e-5) for b in range(16)]
    return lams, prevs


def sequence(lam, delta_prev, d):
    dmin, _ = spectrum(lam)
    return R.delta_sequence(dmin, delta_prev, d)


def predict(lam, delta_prev, d):
    """(status, num_fac, delta) of ipopt_strategy! on the design: the first attempt with delta > -lambda_min succeeds; an attempt of
    the loop (every one but a first attempt at delta_zero, which exists when diag_min > 0) beyond d.max ends it as a failure."""
    dmin, lmin = spectrum(lam)
    seq = sequence(lam, delta_prev, d)
    for i, (delta, _) in enumerate(seq):
        if delta > -lmin:
            return "success", i + 1, delta
        in_loop = not (i == 0 and 1.5 * dmin > 0.0)
        if in_loop and delta > d.max:
            return "failure", i + 1, delta
    raise AssertionError("the sequence never ends")


def margin(lam, delta_prev, d):
    """The distance of the attempts from -lambda_min, relative (lanczos_ref.margin_from_grid): a prediction is only as good as this."""
    return R.margin_from_grid(sequence(lam, delta_prev, d), spectrum(lam)[1])
