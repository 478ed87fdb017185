"""The step-side vector kernels (csrc/ls_device.h, linesearch.hip, ls_batch.hip) against exact arithmetic at the edges of their
partition: all five functions of onephase_jl_amd.line_search on the designs of ls_edge_designs.py against ls_exact.py.  Every max / min
/ flag output is compared as bits; every sum either as bits (dyadic tier: integers) or by err / bound <= 1 with the gamma bound derived
in ls_exact.py (random tier, merit_red).  No free tolerance.  test_ls_edge_designs_host.py checks the designs and the reference on the host."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest

import ls_edge_designs as D
import ls_exact as X
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import line_search as LS

pytestmark = pytest.mark.gpu

PARS = LS.Class_ls_parameters(fraction_to_boundary_predict_exp=D.EX, comp_feas=D.COMP_FEAS)
INF = math.inf
i32p = C.POINTER(C.c_int32)
# okkt_kkt_dual_step: (dual_ls, lb, ub, step_size_P, scales).  Open clamps return the quotient of the sums itself; one scale at zero
# leaves the two n sums or the two m sums alone; the closed clamps and dual_ls = 0 exercise ls_finish.h's selection
OPEN = (1, -INF, INF, -INF, "both")
DUAL = (OPEN, (3, -INF, INF, -INF, "n"), (1, -INF, INF, -INF, "m"), (3, 0.1, 0.6, 0.3, "both"), (0, 0.1, 0.6, 0.3, "both"))


def scaled(c, which):
    return c if which == "both" else dataclasses.replace(c, scale_mu=0.0) if which == "n" else dataclasses.replace(c, scale_D=0.0)


@functools.lru_cache(maxsize=None)
def base_case(N, variant=0):
    """Random tier: variant = big_dx; dyadic tier: variant = the item."""
    return D.base_random(N, big_dx=bool(variant)) if N in D.RANDOM_N else D.base_dyadic(N, variant)


@functools.lru_cache(maxsize=None)
def base_sums(N, variant, which):
    """The exact sums of a base case, computed once: the planted cases' sums come from them (ls_exact.sums, near)."""
    b = scaled(base_case(N, variant), which)
    return b, X.sums(b)


def device_round(k, c, steps, dual):
    """One round of the five functions on solver k (structure W(N)) at the case's iterate and direction."""
    it = D.iterate(c, KS.Class_iterate)
    k.form_system_b(it)
    LS.set_direction(k, KS.Class_point(c.dx, c.dy, c.ds, mu=c.dmu))
    out = {}
    out["step_P"], out["nx"] = LS.max_step_primal(k, c.frac_predict, PARS)
    out["ok"] = LS.s_bound_ok(k, c.s_new, c.frac, PARS)
    cand = dataclasses.replace(it, s=c.s_cand, y=c.y_cand, mu=c.mu_cand)
    out["range"] = LS.dual_step_range(k, cand, c.frac, PARS)
    out["pred"] = {st: LS.predicted_reduction_terms(k, st) for st in steps}
    new_it = dataclasses.replace(cand, grad=c.grad_cand, J=D.diag_matrix(c.N, c.J_cand))
    out["sd"] = {}
    for cfg in dual:
        dual_ls, lb, ub, sP, which = cfg
        cv = scaled(c, which)
        out["sd"][cfg] = LS.move_dual_step(k, new_it, sP, lb, ub, cv.scale_D, cv.scale_mu, dataclasses.replace(PARS, dual_ls=dual_ls))
    return out


class Worst:
    """The largest err / bound seen, printed at the end of a test (-s shows it)."""
    def __init__(self):
        self.r, self.where = 0.0, None

    def add(self, r, where):
        if r > self.r:
            self.r, self.where = r, where


def check_pred(c, got, ex, tag, worst):
    assert X.same_bits(got[1], ex["C_k"]) and X.same_bits(got[2], ex["P_k"]), (tag, got, ex["C_k"], ex["P_k"])
    phi, phi_b = ex["phi"]
    if phi is None:
        assert got[0] != got[0] and got[3] != got[3], (tag, got)
        return
    if c.tier == "dyadic":
        assert X.same_bits(got[0], X.exactly(phi)), (tag, got[0], float(phi))
    else:
        r = X._ratio(got[0], phi, phi_b)
        worst.add(r, (tag, "phi_red"))
        assert r <= 1.0, (tag, "phi_red", got[0], float(phi), phi_b, r)
    merit, merit_b = ex["merit"]
    if merit is None:
        assert got[3] != got[3], (tag, got)
    else:
        r = X._ratio(got[3], merit, merit_b)
        worst.add(r, (tag, "merit_red"))
        assert r <= 1.0, (tag, "merit_red", got[3], float(merit), merit_b, r)


def check_sd(c, got, cfg, S, tag, worst):
    dual_ls, lb, ub, sP, _ = cfg
    sd, bound = X.dual_step(c, lb, ub, sP, dual_ls, S)
    if sd is None:
        assert got != got, (tag, cfg, got)
    elif c.tier == "dyadic" or dual_ls == 0:
        assert X.same_bits(got, float(sd)), (tag, cfg, got, float(sd))
    else:
        r = X._ratio(got, sd, bound)
        worst.add(r, (tag, "step_size_D", cfg))
        assert r <= 1.0, (tag, cfg, got, float(sd), bound, r)


def check_round(c, got, variant, steps, dual, tag, worst, planted=True):
    """The outputs of device_round against ls_exact."""
    step_P, nx = X.max_step_primal(c)
    assert X.same_bits(got["nx"], nx) and X.same_bits(got["step_P"], step_P), (tag, got["nx"], nx, got["step_P"], step_P)
    assert got["ok"] == X.s_bound_ok(c), (tag, got["ok"])
    lb, ub = X.dual_step_range(c)
    assert X.same_bits(got["range"][0], lb) and X.same_bits(got["range"][1], ub), (tag, got["range"], lb, ub)
    sums = {}
    for which in {cfg[4] for cfg in dual} | {"both"}:
        near = base_sums(c.N, variant, which)
        sums[which] = near[1] if not planted else X.sums(scaled(c, which), near)
    for st in steps:
        check_pred(c, got["pred"][st], X.predicted(c, st, sums["both"]), (tag, st), worst)
    for cfg in dual:
        check_sd(scaled(c, cfg[4]), got["sd"][cfg], cfg, sums[cfg[4]], tag, worst)


def new_solver(N, kind, variant=0):
    k = KS.HIP_KKT_solver(kind)
    k.initialize_b(D.iterate(base_case(N, variant), KS.Class_iterate))
    return k


# ---- 1. the random tier: every N, both kinds, both step sizes, both branches of min(1, |dx|_inf), dual_ls in (0, 1, 3) ---------------------
@pytest.mark.parametrize("kind", ["schur", "symmetric"])
@pytest.mark.parametrize("N", D.RANDOM_N)
def test_random_tier(N, kind):
    k = new_solver(N, kind)
    worst = Worst()
    for big_dx in (0, 1):
        b = base_case(N, big_dx)
        assert (X.dx_norm(b) > 1.0) == bool(big_dx)
        check_round(b, device_round(k, b, b.steps, DUAL), big_dx, b.steps, DUAL, (N, kind, big_dx, "base"), worst, planted=False)
        for label, c in D.edge_cases(b):
            check_round(c, device_round(k, c, c.steps[1:], (OPEN,)), big_dx, c.steps[1:], (OPEN,), (N, kind, big_dx, label), worst)
    k.finalize_b()
    print(f"N = {N} {kind}: largest err / bound {worst.r:.3f} at {worst.where}")


# ---- 2. the dyadic tier: 256 workgroups, the fifth iteration, the ragged stride; one handle per N ------------------------------------------
_HANDLES = {}


def dyadic_handle(N):
    if N not in _HANDLES:
        _HANDLES[N] = new_solver(N, "symmetric")
    return _HANDLES[N]


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    for k in _HANDLES.values():
        k.finalize_b()
    _HANDLES.clear()


@pytest.mark.parametrize("part", ["base", "a", "b", "c", "reset", "n1", "n2", "n3", "n4"])
@pytest.mark.parametrize("N", D.DYADIC_N)
def test_dyadic_tier(N, part):
    k = dyadic_handle(N)
    b = base_case(N, 0)
    worst = Worst()
    if part == "base":
        got = device_round(k, b, b.steps, DUAL)
        check_round(b, got, 0, b.steps, DUAL, (N, "base"), worst, planted=False)
        if N == 600001:          # fixed partition, no atomics: a second round gives the same bits
            assert device_round(k, b, b.steps, DUAL) == got
        return
    cases = [(label, c) for label, c in D.edge_cases(b) if label.startswith(part + "@") or (part == "reset" and label.startswith("reset"))]
    assert len(cases) >= len(D.positions(N))
    for label, c in cases:
        check_round(c, device_round(k, c, c.steps[1:], (OPEN,)), 0, c.steps[1:], (OPEN,), (N, label), worst)


# ---- 3. the batch at full width: 3 items of W(262145), 256 live partial rows of up to 4 channels per item ------------------------------------
def batch_cases(N):
    """Three items that differ in values and in where their extrema sit: item 0 decides in the one entry of the fifth iteration, item 1 in
    the last partial row (and the first entry of the second stride), item 2 restarts dual_bounds in the last partial row."""
    c0 = D.plant(base_case(N, 0), "a", 262144)
    c1 = D.plant(D.plant(base_case(N, 1), "b", 262143), "c", 65536)
    c2 = D.plant_reset(D.plant(base_case(N, 2), "a", 65535), 262143)
    return [c0, c1, c2]


def batch_round(k, cs, its, items, out):
    """The five okkt_kkt_items_* calls over `items` (None: all), written into the arrays of `out` (slots that are not listed keep what
    the arrays hold)."""
    B, N = len(cs), cs[0].N
    lib, h = k._lib, k._k
    ip, ni = (None, 0) if items is None else (np.ascontiguousarray(items, np.int32).ctypes.data_as(i32p), len(items))
    st = lambda f: L.f64(np.stack([getattr(c, f) for c in cs]))
    sc = lambda vals: L.f64(np.array(vals, dtype=float))
    fp, fb, s_new, s_cand, y_cand, grad, grad_cand, Jc = (st(f) for f in ("frac_predict", "frac", "s_new", "s_cand", "y_cand", "grad", "grad_cand", "J_cand"))
    k._check(lib.okkt_kkt_items_max_step_primal(h, B, ip, ni, L.p_f64(fp), N, D.EX, L.p_f64(out["step_P"]), L.p_f64(out["nx"])), "max_step_primal")
    k._check(lib.okkt_kkt_items_s_bound_ok(h, B, ip, ni, L.p_f64(s_new), L.p_f64(fb), N, D.EX, out["ok"].ctypes.data_as(i32p)), "s_bound_ok")
    mu_c = sc([c.mu_cand for c in cs])
    k._check(lib.okkt_kkt_items_dual_step_range(h, B, ip, ni, L.p_f64(s_cand), L.p_f64(y_cand), L.p_f64(mu_c), D.COMP_FEAS, L.p_f64(fb), N, L.p_f64(out["lb"]),
                                                L.p_f64(out["ub"])), "dual_step_range")
    mu, dmu, pen, step = sc([c.mu for c in cs]), sc([c.dmu for c in cs]), sc([c.pen for c in cs]), sc([c.steps[b % 2] for b, c in enumerate(cs)])
    k._check(lib.okkt_kkt_items_predicted_reduction(h, B, ip, ni, L.p_f64(grad), L.p_f64(mu), L.p_f64(dmu), L.p_f64(pen), L.p_f64(step), L.p_f64(out["pred"])),
             "predicted_reduction")
    sP, lb, ub = sc([-INF] * B), sc([-INF] * B), sc([INF] * B)
    sD, sM = sc([c.scale_D for c in cs]), sc([c.scale_mu for c in cs])
    k._check(lib.okkt_kkt_items_dual_step(h, B, ip, ni, L.p_f64(Jc), N, L.p_f64(grad_cand), L.p_f64(s_cand), L.p_f64(y_cand), L.p_f64(mu_c), L.p_f64(pen), L.p_f64(sP),
                                          L.p_f64(lb), L.p_f64(ub), L.p_f64(sD), L.p_f64(sM), 1, L.p_f64(out["sd"])), "dual_step")


def item_result(out, b, c):
    """Slot b of the batch's outputs in the form check_round reads."""
    return dict(step_P=out["step_P"][b], nx=out["nx"][b], ok=bool(out["ok"][b]), range=(out["lb"][b], out["ub"][b]),
                pred={c.steps[b % 2]: tuple(out["pred"][b])}, sd={OPEN: out["sd"][b]})


def test_batch_of_three_at_full_width():
    N, B = 262145, 3
    assert D.nb(N) == 256 and D.serial_adds(N) == 5
    cs = batch_cases(N)
    its = [D.iterate(c, KS.Class_iterate) for c in cs]
    k = KS.HIP_KKT_solver("symmetric")
    k.initialize_b(its[0])
    k._set_structure(its[0])
    assert k.items_query()["eligible"] == 1 and LS.items_ls_query(k)["eligible"] == 1
    k.items_reserve(B)
    k.form_system_items(its)
    LS.set_direction_items(k, [KS.Class_point(c.dx, c.dy, c.ds, mu=c.dmu) for c in cs])
    out = dict(step_P=np.full(B, -7.0), nx=np.full(B, -7.0), ok=np.full(B, -7, np.int32), lb=np.full(B, -7.0), ub=np.full(B, -7.0), pred=np.full((B, 4), -7.0),
               sd=np.full(B, -7.0))
    worst = Worst()

    def check(b, call):
        c = cs[b]
        st = (c.steps[b % 2],)
        check_round(c, item_result(out, b, c), b, st, (OPEN,), (call, "item", b), worst)

    batch_round(k, cs, its, None, out)
    for b in range(B):
        check(b, "all")
    # the items differ: a batch that ignored the item index would not pass
    assert all(len({np.asarray(out[f][b]).tobytes() for b in range(B)}) == B for f in ("lb", "ub", "pred", "sd"))
    first = {f: a.copy() for f, a in out.items()}
    # the listed items [2, 0]: their outputs are written again (poisoned first), item 1's are those of the first call, untouched
    for a in out.values():
        a[0], a[2] = -7, -7
    batch_round(k, cs, its, [2, 0], out)
    for b in (2, 0):
        check(b, "[2, 0]")
    for f, a in out.items():
        assert np.asarray(a).tobytes() == np.asarray(first[f]).tobytes(), f
    k.finalize_b()
