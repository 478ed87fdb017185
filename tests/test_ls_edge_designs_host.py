"""The designs of ls_edge_designs.py hold what they claim, and ls_exact.py agrees with oracle/line_search_oracle.py on every one of them:
bit for bit on the max / min results and the 0 / 1 test, within the rounding bound on the sums (bit for bit in the dyadic tier, where
every order of summation is exact).  No GPU."""
import functools
import hashlib
import math
import time

import numpy as np
import pytest

import ls_edge_designs as D
import ls_exact as X
from oracle import kkt_oracle as KO
from oracle import line_search_oracle as LO


@functools.lru_cache(maxsize=None)
def base(N):
    return D.base_random(N, big_dx=(N % 2 == 0)) if N in D.RANDOM_N else D.base_dyadic(N)


# ---- 1. the partition -----------------------------------------------------------------------------------------------------------------
def test_partition_facts():
    assert [D.nb(N) for N in D.RANDOM_N] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3]
    assert [D.nb(N) for N in D.DYADIC_N] == [256, 256, 256, 256]
    assert D.nb(261120) == 255 and D.stride(261121) == 65536
    assert [D.serial_adds(N) for N in D.DYADIC_N] == [4, 4, 5, 10]
    assert [D.serial_adds(N) for N in (255, 256, 257, 1024, 1025, 2048, 2049)] == [1, 1, 2, 4, 3, 4, 3]
    assert D.positions(1) == [0] and D.positions(2) == [0, 1] and D.positions(256) == [0, 255] and D.positions(257) == [0, 255, 256]
    assert D.positions(1025) == [0, 511, 512, 1023, 1024] and D.positions(2049) == [0, 767, 768, 1535, 1536, 2048]
    assert D.positions(262144) == [0, 65535, 65536, 196607, 196608, 262143]
    assert D.positions(262145) == [0, 65535, 65536, 262143, 262144]                      # 262144: the only entry of a fifth iteration
    assert D.positions(600001) == [0, 65535, 65536, 262144, 589823, 589824, 600000]
    for N in D.RANDOM_N + D.DYADIC_N:
        st = D.stride(N)
        for p in D.positions(N):
            assert 0 <= p < N
        # who takes an entry: workgroup (p mod stride) / 256, iteration p / stride -- the last position sits in the last iteration
        assert (N - 1) // st == D.serial_adds(N) - 1
    # 600001 = 2 * 262144 + 75713 is ragged in its third block of 256 * 1024; the last of its ten strides holds 10177 entries: 39 full
    # workgroups and 193 threads of the fortieth
    assert 600001 - 9 * 65536 == 10177 and 10177 // 256 == 39 and 10177 % 256 == 193
    assert X.reduce_roundings(600001) == 10 + 8 + 1 + 8 and X.reduce_roundings(1) == 1 + 8 + 1 + 8


# ---- 2. every plant decides alone, with a factor of two to the runner-up ------------------------------------------------------------------
def channel(c, what):
    """The number the plant `what` decides (for s_bound: the verdict)."""
    if what == "ratio_s":
        return X.primal_ratio(c)
    if what == "s_bound":
        return X.s_bound_ok(c)
    if what in ("lb", "ub", "lb_y"):
        return X.dual_channels(c)[{"lb": 0, "ub": 1, "lb_y": 3}[what]]
    if what == "dx":
        return X.dx_norm(c)
    return X.comp_norms(c, c.steps[-1])[0 if what == "comp" else 1]


@pytest.mark.parametrize("N", D.RANDOM_N + D.DYADIC_N)
def test_planted_entries_decide_alone(N):
    b = base(N)
    assert not np.any(b.dy == 0.0) and X.s_bound_ok(b) and X.dual_channels(b)[2] == -1
    for p in D.positions(N):
        for g, whats in D.GROUPS.items():
            c = D.plant(b, g, p)
            lost = D.without(c, p)
            for w in whats:
                with_, without = channel(c, w), channel(lost, w)
                if w == "s_bound":
                    assert with_ is False and without is True, (N, p, w)
                elif w == "ub":
                    assert with_ <= -1.9 and without > 0.0, (N, p, w, with_, without)       # the only negative candidate
                elif w == "lb":
                    assert with_ >= 1.9 and without == 0.0, (N, p, w, with_, without)       # the only positive one: the runner-up is the start
                else:
                    assert with_ >= 2.0 * without >= 0.0 and with_ > 0.0, (N, p, w, with_, without)
            if g == "c":        # the lb_y ratio, not dual_bounds, gives the upper end of the range
                r = X.dual_channels(c)
                assert X.dual_step_range(c)[1] == 1.0 / r[3] < r[1]
        # the reset: behind it (0, -1) and the two rows that follow; the rows before it do not count
        c = D.plant_reset(b, p)
        lb, ub, after, _ = X.dual_channels(c)
        assert after == p
        assert (lb >= 1.9 and lb < 2.1) if p + 1 < N else lb == 0.0
        assert (ub <= -1.9 and ub > -2.1) if p + 2 < N else ub == -1.0
        if p >= 1:
            head = D.without(c, p)      # without the reset row the earlier candidates count
            assert X.dual_channels(head)[0] >= 3.9 and (p < 2 or X.dual_channels(head)[1] <= -3.9)
    c = D.plant_reset(b, N - 1, negative_zero=True)
    assert math.copysign(1.0, c.dy[N - 1]) < 0 and X.dual_channels(c)[:3] == (0.0, -1.0, N - 1)
    for g, fields in D.NAN_GROUPS.items():
        c = D.plant_nan(b, g, D.positions(N)[-1])
        assert all(np.isnan(getattr(c, f)).sum() == 1 for f in fields)
        step_P, nx = X.max_step_primal(c)
        lb, ub = X.dual_step_range(c)
        C_k, P_k = X.comp_norms(c, 1.0)
        got = dict(step_P=step_P, nx=nx, ub=ub, C_k=C_k, P_k=P_k)
        want_nan = {"n1": {"step_P", "ub", "P_k"}, "n2": {"ub", "C_k", "P_k"}, "n3": {"ub", "P_k"}, "n4": {"step_P", "nx", "ub"}}[g]
        assert {k for k, v in got.items() if v != v} == want_nan, (N, g, got)


# ---- 3. the dyadic tier is exact in integer arithmetic ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", D.DYADIC_N)
def test_dyadic_tier_is_integer_exact(N):
    """sums() runs in Dy: every intermediate below 2^53, len * max|term| < 2^53 per channel (its assertions); the finished numbers are
    doubles too."""
    for item in range(3):
        b = D.base_dyadic(N, item)
        for f in ("s", "pen", "scale_D", "scale_mu", "J", "J_cand"):
            m, _ = np.frexp(np.abs(np.asarray(getattr(b, f), dtype=float)))
            assert np.all(m == 0.5), f                                                    # powers of two
        assert all(np.frexp(st)[0] == 0.5 for st in b.steps)
        S = X.sums(b)
        assert all(S[name][0] is not None for name in X.MAP_ROUNDINGS)
        for step in b.steps:
            X.exactly(X.predicted(b, step, S)["phi"][0])
    b = base(N)
    near = (b, X.sums(b))
    for label, c in D.edge_cases(b):
        S = X.sums(c, near)
        if label.startswith(("a@", "b@", "c@", "reset")):
            assert all(S[name][0] is not None for name in X.MAP_ROUNDINGS), label
            for step in c.steps:
                X.exactly(X.predicted(c, step, S)["phi"][0])
    # the sums of a planted case from the base case's are those of the whole case
    c = D.plant(b, "a", D.positions(N)[-2])
    full = X.sums(c)
    assert all(full[name] == X.sums(c, near)[name] for name in X.MAP_ROUNDINGS)


def test_a_case_that_is_not_dyadic_is_refused():
    c = D.base_dyadic(261121).copy()
    c.s[5] = 1.5
    with pytest.raises(AssertionError):
        X.sums(c)
    c = D.base_dyadic(261121).copy()
    c.y[7] = 2.0 ** 30 + 1.0
    with pytest.raises(AssertionError):
        X.sums(c)


# ---- 4. ls_exact against the oracle ----------------------------------------------------------------------------------------------------------
_DUAL_MEMO = {}


def oracle_dual_range(oit, od, c):
    """LO.dual_step_range, its Python loop run once per distinct input."""
    h = hashlib.blake2b(digest_size=16)
    for a in (c.s_cand, c.y_cand, c.dy, c.frac, c.y, np.array([c.mu_cand, X.dx_norm(c)])):
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.digest()
    if key not in _DUAL_MEMO:
        _DUAL_MEMO[key] = LO.dual_step_range(oit, od, c.s_cand, c.y_cand, c.mu_cand, D.COMP_FEAS, c.frac)
    return _DUAL_MEMO[key]


def any_order(S, name, N, extra=2):
    """The bound of a sum of N terms in ANY order (numpy's pairwise sum, a BLAS dot): the map's roundings, `extra` for the oracle's own
    arrangement of the map, N - 1 additions."""
    exact, pieces, k = S[name]
    return X.gamma(k - X.reduce_roundings(N) + extra + N) * float(pieces)


def check_against_oracle(label, c, near=None):
    oit = D.iterate(c, KO.Iterate)
    od = KO.Direction(c.dx, c.dy, c.ds, mu=c.dmu)
    tag = (c.N, label)
    step_P, nx = X.max_step_primal(c)
    assert X.same_bits(nx, LO._norm_inf(od.x)), tag
    assert X.same_bits(step_P, LO.simple_max_step(oit.s, od.s, LO.lb_s_predict(oit, od, c.frac_predict, D.EX))), tag
    assert X.s_bound_ok(c) == LO.s_bound_ok(oit, od, c.s_new, c.frac, D.EX), tag
    lb, ub = X.dual_step_range(c)
    olb, oub = oracle_dual_range(oit, od, c)
    assert X.same_bits(lb, olb) and X.same_bits(ub, oub), (tag, lb, ub, olb, oub)
    S = X.sums(c, near)
    for step in (c.steps if near is None else c.steps[1:]):
        ex = X.predicted(c, step, S)
        o = LO.predicted_reduction_terms(oit, od, step)
        assert X.same_bits(ex["C_k"], o[1]) and X.same_bits(ex["P_k"], o[2]), tag
        phi, phi_b = ex["phi"]
        if phi is None:
            assert o[0] != o[0] and o[3] != o[3], tag
            continue
        merit, merit_b = ex["merit"]
        if c.tier == "dyadic":
            assert X.same_bits(o[0], X.exactly(phi)), tag
        else:
            b = abs(step) * any_order(S, "pred_n0", c.N) + step * step / 2 * (any_order(S, "pred_n1", c.N) + any_order(S, "pred_m0", c.N))
            assert X._ratio(o[0], phi, b * (1 + 8 * X.U)) <= 1.0, tag
            phi_b = b * (1 + 8 * X.U)
        if merit is None:
            assert o[3] != o[3], tag
        else:
            assert X._ratio(o[3], merit, merit_b + phi_b) <= 1.0, tag
    ocand = KO.Iterate(x=oit.x, y=c.y_cand, s=c.s_cand, mu=c.mu_cand, J=D.diag_matrix(c.N, c.J_cand), H=oit.H, grad=c.grad_cand, cons=oit.cons,
                       a_norm_penalty_par=c.pen)
    inf = math.inf
    for bounds in ((-inf, inf, -inf), (0.1, 0.6, 0.3)):
        sd, sd_b = X.dual_step(c, *bounds, 1, S)
        with np.errstate(invalid="ignore"):
            o = LO.move_dual_step(ocand, od, bounds[2], bounds[0], bounds[1], 1, c.scale_D, c.scale_mu)
        if sd is None:
            assert o != o, tag
        elif c.tier == "dyadic":
            assert X.same_bits(o, float(sd)), tag
        else:
            den = S["dual_n1"][0] + S["dual_m1"][0]
            b = X.gamma(8 + 5 + 3 + 2 * c.N) * float((S["dual_n0"][1] + S["dual_m0"][1]) / den)
            assert X._ratio(o, sd, b) <= 1.0, tag
    assert LO.move_dual_step(ocand, od, 0.3, 0.1, 0.6, 0, c.scale_D, c.scale_mu) == X.dual_step(c, 0.1, 0.6, 0.3, 0, S)[0] == 0.6


@pytest.mark.parametrize("N", D.RANDOM_N + D.DYADIC_N)
def test_ls_exact_agrees_with_the_oracle_on_every_design(N):
    near = (base(N), X.sums(base(N)))
    check_against_oracle("base", base(N))
    for label, c in D.edge_cases(base(N)):           # the planted cases: the sums from the base case's, one step size
        check_against_oracle(label, c, near)
    if N in D.RANDOM_N:
        other = D.base_random(N, big_dx=(N % 2 == 1))
        assert (X.dx_norm(other) > 1.0) != (X.dx_norm(base(N)) > 1.0)
        check_against_oracle("other branch of min(1, |dx|)", other)


def test_the_oracle_loop_finishes_in_seconds_at_the_largest_size():
    c = D.plant_reset(base(600001), 262144)
    t0 = time.perf_counter()
    got = LO.dual_bounds(c.s_cand, c.mu_cand, c.y_cand, c.dy, D.COMP_FEAS)
    dt = time.perf_counter() - t0
    lb, ub, _, _ = X.dual_channels(c)
    assert got == (lb, ub)
    assert dt < 5.0, dt
