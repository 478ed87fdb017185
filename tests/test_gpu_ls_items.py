"""Line-search batches (okkt_kkt_items_max_step_primal ...) against the single-iterate calls on a fresh solver per
item: step_size_P and norm(dx, Inf), the s-bound verdict, (lb, ub) of the dual range, the four predicted-reduction numbers and
step_size_D -- as bytes, no tolerance anywhere except the oracle anchor.  The families, the designed directions and the inputs of a round
are ls_items_designs.py's (their properties are checked on the host in test_ls_items_host.py); the serial side of a (family, kind, item,
direction) is computed once and shared."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import ls_items_designs as D
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import line_search as LS
from onephase_jl_amd.kkt_system_solver import _csc
from onephase_jl_amd.linear_system_solvers import OkktError
from oracle import kkt_oracle as KO
from oracle import line_search_oracle as LO

pytestmark = pytest.mark.gpu

CASES = [(name, kind) for name in ("d37", "banded", "chain") for kind in D.KINDS[name]]
PARS = LS.Class_ls_parameters(comp_feas=0.01)
i32p = C.POINTER(C.c_int32)


def bts(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def family(name, B):
    return D.family(name, KS.Class_iterate, B)


@functools.lru_cache(maxsize=None)
def designed(name, B):
    return D.designed_directions(family(name, B), KS.Class_point)


def cand_J(it, scale):
    J = _csc(it.J).copy()
    J.data = J.data * scale
    return J


def round_of(name, B, b, d, mode, alpha=None):
    """Item b's inputs: the designed y_cand goes with the designed direction."""
    it = family(name, B)[b]
    return D.round_inputs(b, it, d, designed(name, B)[1][b] if mode == "set" else None, alpha)


def result(step_P, nx, ok, lb, ub, pred, sd):
    return dict(step_P=bts(step_P), nx=bts(nx), ok=int(ok), range=bts([lb, ub]), pred=bts(pred), sd=bts(sd))


def serial_solver(it, kind, delta, d_set):
    """The serial sequence up to a resident direction on a fresh solver: the solve's own, or the given one."""
    k = KS.HIP_KKT_solver(kind)
    k.initialize_b(it)
    k.form_system_b(it)
    assert k.factor_b(delta) in (0, 1)
    if d_set is None:
        k.kkt_associate_rhs_b(it, KS.Reduct_affine())
        k.compute_direction_b()
    else:
        LS.set_direction(k, d_set)
    return k


def serial_dual_step(k, Jx, r, pen, step_P, lb, ub, dual_ls):
    out = C.c_double()
    g, s, y = L.f64(r.grad_cand), L.f64(r.s_cand), L.f64(r.y_cand)
    k._check(k._lib.okkt_kkt_dual_step(k._k, L.p_f64(Jx) if Jx is not None else None, L.p_f64(g), L.p_f64(s), L.p_f64(y), float(r.mu_cand), float(pen),
                                       float(step_P), float(lb), float(ub), int(dual_ls), float(r.scale_D), float(r.scale_mu), C.byref(out)), "okkt_kkt_dual_step")
    return out.value


def serial_calls(k, it, r, dual_ls=1, jmode="per", J_shared=None):
    """One line-search round with the LS.* calls on the solver's resident iterate and direction."""
    step_P, nx = LS.max_step_primal(k, r.frac_predict, PARS)
    ok = LS.s_bound_ok(k, r.s_cand, r.frac, PARS)
    cand = dataclasses.replace(it, s=r.s_cand, y=r.y_cand, mu=r.mu_cand)
    lb, ub = LS.dual_step_range(k, cand, r.frac, PARS)
    pred = LS.predicted_reduction_terms(k, r.alpha)
    if jmode == "per" and dual_ls == 1:
        new_it = dataclasses.replace(cand, grad=r.grad_cand, J=cand_J(it, r.J_scale))
        sd = LS.move_dual_step(k, new_it, r.alpha, lb, ub, r.scale_D, r.scale_mu, PARS)
    else:
        Jx = {"per": lambda: L.f64(cand_J(it, r.J_scale).data), "shared": lambda: L.f64(J_shared), "null": lambda: None}[jmode]()
        sd = serial_dual_step(k, Jx, r, it.a_norm_penalty_par, r.alpha, lb, ub, dual_ls)
    return result(step_P, nx, ok, lb, ub, pred, sd)


@functools.lru_cache(maxsize=None)
def serial_ref(name, kind, B, b, mode):
    """mode "solve": the direction of compute_direction_b; "set": the designed direction through LS.set_direction."""
    it = family(name, B)[b]
    d_set = designed(name, B)[0][b] if mode == "set" else None
    k = serial_solver(it, kind, D.DELTA[name], d_set)
    out = serial_calls(k, it, round_of(name, B, b, k.dir, mode))
    k.finalize_b()
    return out


def batch_solver(name, kind, B, mode, reserve=None):
    """A batch solver with the B items formed and their directions resident."""
    its = family(name, B)
    k = KS.HIP_KKT_solver(kind)
    k.initialize_b(its[0])
    k._set_structure(its[0])
    assert k.items_query()["eligible"] == 1
    q = LS.items_ls_query(k)
    assert q["eligible"] == 1 and q["extra_bytes_per_item"] > 0 and q["launches_max_step"] == 2 and q["launches_dual_range"] == 2
    k.items_reserve(reserve or B)
    k.form_system_items(its)
    if mode == "solve":
        flags, _ = k.factor_items([D.DELTA[name]] * B)
        k.kkt_associate_rhs_items(its, KS.Reduct_affine())
        dirs, _ = k.compute_direction_items(resident=True)       # the directions stay in the slots
        assert dirs == []
        dirs = [KS.Class_point(None, None, np.zeros(its[0].ncon()), mu=mu) for mu in k._items_dir_mu]      # ds is read below for the candidates only
    else:
        dirs = designed(name, B)[0]
        LS.set_direction_items(k, dirs)
    return k, its, dirs


def batch_calls(k, its, rounds, items=None, dual_ls=1, jmode="per", J_shared=None, frac_shared=False):
    """The same round for all items (or the listed ones) in five calls -> one result dict per slot (None: not listed)."""
    B = len(its)
    fp = rounds[0].frac_predict if frac_shared else np.stack([r.frac_predict for r in rounds])
    fb = rounds[0].frac if frac_shared else np.stack([r.frac for r in rounds])
    step_P, nx = LS.max_step_primal_items(k, fp, PARS, items)
    ok = LS.s_bound_ok_items(k, [r.s_cand for r in rounds], fb, PARS, items)
    cands = [dataclasses.replace(it, s=r.s_cand, y=r.y_cand, mu=r.mu_cand) for it, r in zip(its, rounds)]
    lb, ub = LS.dual_step_range_items(k, cands, fb, PARS, items)
    pred = LS.predicted_reduction_terms_items(k, [r.alpha for r in rounds], items)
    pars = dataclasses.replace(PARS, dual_ls=dual_ls)
    if jmode == "per":
        new_its = [dataclasses.replace(c, grad=r.grad_cand, J=cand_J(it, r.J_scale)) for c, it, r in zip(cands, its, rounds)]
        sd = LS.move_dual_step_items(k, new_its, [r.alpha for r in rounds], lb, ub, [r.scale_D for r in rounds], [r.scale_mu for r in rounds], pars, items)
    else:
        Jx = None if jmode == "null" else L.f64(J_shared)
        ip, ni = (None, 0) if items is None else (np.ascontiguousarray(items, np.int32).ctypes.data_as(i32p), len(items))
        arr = lambda vs: L.f64(np.array(vs, dtype=float))
        g, s, y = (L.f64(np.stack(v)) for v in ([r.grad_cand for r in rounds], [r.s_cand for r in rounds], [r.y_cand for r in rounds]))
        a = [arr([r.mu_cand for r in rounds]), arr([it.a_norm_penalty_par for it in its]), arr([r.alpha for r in rounds]), L.f64(lb), L.f64(ub),
             arr([r.scale_D for r in rounds]), arr([r.scale_mu for r in rounds])]
        sd = np.full(B, np.nan)
        k._check(k._lib.okkt_kkt_items_dual_step(k._k, B, ip, ni, L.p_f64(Jx) if Jx is not None else None, 0, L.p_f64(g), L.p_f64(s), L.p_f64(y),
                                                 *[L.p_f64(v) for v in a], int(dual_ls), L.p_f64(sd)), "okkt_kkt_items_dual_step")
    listed = range(B) if items is None else list(items)
    return [result(step_P[b], nx[b], ok[b], lb[b], ub[b], pred[b], sd[b]) if b in listed else None for b in range(B)]


def rounds_of(name, B, dirs, mode, k=None):
    """The rounds of all items.  After a solve the candidates need ds: it is read back once through items_select."""
    if mode == "solve":
        its = family(name, B)
        for b in range(B):
            k.items_select(b)
            n, m = its[b].dim(), its[b].ncon()
            dx, dy, ds = np.zeros(n), np.zeros(m), np.zeros(m)
            k._check(k._lib.okkt_kkt_get_direction(k._k, L.p_f64(dx), L.p_f64(dy), L.p_f64(ds)), "okkt_kkt_get_direction")
            dirs[b] = KS.Class_point(dx, dy, ds, mu=dirs[b].mu)
    return [round_of(name, B, b, dirs[b], mode) for b in range(B)]


# ---- 1. all five calls on every design and kind -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["solve", "set"])
@pytest.mark.parametrize("name,kind", CASES)
def test_five_calls_against_the_serial_sequence(name, kind, mode):
    B = 4
    k, its, dirs = batch_solver(name, kind, B, mode)
    rounds = rounds_of(name, B, dirs, mode, k)
    got = batch_calls(k, its, rounds)
    refs = [serial_ref(name, kind, B, b, mode) for b in range(B)]
    for b in range(B):
        assert got[b] == refs[b], (b, [f for f in refs[b] if got[b][f] != refs[b][f]])
    assert len({r["pred"] for r in refs}) == B and len({r["range"] for r in refs}) > 1         # a batch that ignored the item index would not pass
    # determinism: a second call gives the same bytes (fixed partition, no atomics)
    assert batch_calls(k, its, rounds) == got
    k.finalize_b()


@pytest.mark.parametrize("kind", D.KINDS["d37"])
def test_batch_of_one(kind):
    k, its, dirs = batch_solver("d37", kind, 1, "set")
    got = batch_calls(k, its, rounds_of("d37", 1, dirs, "set"))
    assert got[0] == serial_ref("d37", kind, 1, 0, "set")
    k.finalize_b()


@pytest.mark.parametrize("kind", D.KINDS["d37"])
def test_sixteen_items_with_their_own_scalars(kind):
    B = 16
    k, its, dirs = batch_solver("d37", kind, B, "set")
    rounds = rounds_of("d37", B, dirs, "set")
    assert len({r.mu_cand for r in rounds}) == B and len({r.alpha for r in rounds}) == B and len({r.scale_D for r in rounds}) == B and len({r.scale_mu for r in rounds}) == B
    got = batch_calls(k, its, rounds)
    for b in range(B):
        ref = serial_ref("d37", kind, B, b, "set")
        assert got[b] == ref, (b, [f for f in ref if got[b][f] != ref[f]])
    k.finalize_b()


# ---- 2. frac_stride = 0, the item list, backtracking ------------------------------------------------------------------------------------
def test_one_fraction_vector_for_every_item():
    B = 4
    k, its, dirs = batch_solver("banded", "schur", B, "set")
    rounds = rounds_of("banded", B, dirs, "set")
    same = [dataclasses.replace(r, frac_predict=rounds[0].frac_predict, frac=rounds[0].frac) for r in rounds]
    assert batch_calls(k, its, same, frac_shared=True) == batch_calls(k, its, same)
    k.finalize_b()


def test_item_list_leaves_the_other_slots():
    B = 4
    name, kind = "banded", "symmetric"
    k, its, dirs = batch_solver(name, kind, B, "set")
    rounds = rounds_of(name, B, dirs, "set")
    got = batch_calls(k, its, rounds, items=[3, 1])
    assert got[0] is None and got[2] is None
    for b in (3, 1):
        assert got[b] == serial_ref(name, kind, B, b, "set"), b
    # the raw call: outputs of unlisted slots keep what they held
    m = its[0].ncon()
    items = np.array([3, 1], dtype=np.int32)
    fp = L.f64(np.stack([r.frac_predict for r in rounds]))
    step, nx = np.full(B, -7.0), np.full(B, -7.0)
    k._check(k._lib.okkt_kkt_items_max_step_primal(k._k, B, items.ctypes.data_as(i32p), 2, L.p_f64(fp), m, 0.5, L.p_f64(step), L.p_f64(nx)), "max step")
    assert step[0] == -7.0 and step[2] == -7.0 and nx[0] == -7.0 and nx[2] == -7.0
    assert bts(step[3]) == got[3]["step_P"] and bts(step[1]) == got[1]["step_P"] and bts(nx[1]) == got[1]["nx"]
    lb, ub = np.full(B, -7.0), np.full(B, -7.0)
    s, y, mu = (L.f64(np.stack(v)) for v in ([r.s_cand for r in rounds], [r.y_cand for r in rounds], [r.mu_cand for r in rounds]))
    fb = L.f64(np.stack([r.frac for r in rounds]))
    k._check(k._lib.okkt_kkt_items_dual_step_range(k._k, B, items.ctypes.data_as(i32p), 2, L.p_f64(s), L.p_f64(y), L.p_f64(mu), 0.01, L.p_f64(fb), m, L.p_f64(lb),
                                                   L.p_f64(ub)), "range")
    assert (lb[0], ub[0], lb[2], ub[2]) == (-7.0,) * 4 and bts([lb[1], ub[1]]) == got[1]["range"] and bts([lb[3], ub[3]]) == got[3]["range"]
    # an empty list is accepted and writes nothing
    step[:] = -7.0
    assert k._lib.okkt_kkt_items_max_step_primal(k._k, B, items.ctypes.data_as(i32p), 0, L.p_f64(fp), m, 0.5, L.p_f64(step), L.p_f64(nx)) == L.OKKT_OK
    assert np.all(step == -7.0)
    k.finalize_b()


@pytest.mark.parametrize("name,kind", [("d37", "schur"), ("chain", "symmetric")])
def test_backtracking_loop_items_leave_in_different_rounds(name, kind):
    """Three rounds, alpha halved each round; item b leaves after round b (the last two stay to the end), so the list shrinks from
    [0, 1, 2, 3] to [1, 2, 3] to [2, 3].  Every round's outputs against the serial loop on one solver per item."""
    B = 4
    k, its, dirs = batch_solver(name, kind, B, "set")
    serial = [serial_solver(its[b], kind, D.DELTA[name], dirs[b]) for b in range(B)]
    active = list(range(B))
    for rnd in range(3):
        rounds = [round_of(name, B, b, dirs[b], "set", alpha=0.4 / (b + 1) / 2 ** rnd) for b in range(B)]
        got = batch_calls(k, its, rounds, items=active)
        for b in range(B):
            if b in active:
                ref = serial_calls(serial[b], its[b], rounds[b])
                assert got[b] == ref, (rnd, b, [f for f in ref if got[b][f] != ref[f]])
            else:
                assert got[b] is None
        active = [b for b in active if b > rnd]
    assert active == [3]
    for s in serial:
        s.finalize_b()
    k.finalize_b()


# ---- 3. reset, NaN and non-finite items next to ordinary ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("d37", "symmetric"), ("banded", "schur"), ("chain", "symmetric")])
def test_reset_nan_and_nonfinite_items_in_one_call(name, kind):
    B = 6
    k, its, dirs = batch_solver(name, kind, B, "set")
    rounds = rounds_of(name, B, dirs, "set")
    got = batch_calls(k, its, rounds)
    refs = [serial_ref(name, kind, B, b, "set") for b in range(B)]
    for b in range(B):
        assert got[b] == refs[b], (b, D.ROLES[b], [f for f in refs[b] if got[b][f] != refs[b][f]])
    by_role = {D.ROLES[b]: np.frombuffer(refs[b]["range"]) for b in range(1, 5)}
    assert by_role["reset_mid"][1] <= -1.0 and tuple(by_role["reset_last"]) == (0.0, -1.0) and tuple(by_role["nonfinite"]) == (0.0, -1.0)
    assert np.isnan(np.frombuffer(refs[3]["step_P"])[0]) and np.isnan(np.frombuffer(refs[3]["pred"])[2])
    assert np.all(np.isfinite(np.frombuffer(refs[0]["range"]))) and np.isfinite(np.frombuffer(refs[5]["step_P"])[0])
    k.finalize_b()


# ---- 4. dual_step: where J comes from, and dual_ls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("jmode,dual_ls", [("per", 1), ("shared", 1), ("null", 1), ("per", 3), ("null", 0)])
def test_dual_step_jacobians_and_dual_ls(jmode, dual_ls):
    B = 4
    name, kind = "banded", "schur"
    k, its, dirs = batch_solver(name, kind, B, "set")
    rounds = rounds_of(name, B, dirs, "set")
    J_shared = _csc(its[0].J).data * 1.02
    got = batch_calls(k, its, rounds, dual_ls=dual_ls, jmode=jmode, J_shared=J_shared)
    for b in range(B):
        ks = serial_solver(its[b], kind, D.DELTA[name], dirs[b])
        ref = serial_calls(ks, its[b], rounds[b], dual_ls=dual_ls, jmode=jmode, J_shared=J_shared)
        ks.finalize_b()
        assert got[b] == ref, (b, [f for f in ref if got[b][f] != ref[f]])
        if dual_ls == 0:
            assert got[b]["sd"] == bts(np.frombuffer(got[b]["range"])[1])          # step_size_D = ub, nothing launched
    if jmode == "per" and dual_ls == 1:
        with pytest.raises(OkktError, match="dual_ls == 2"):
            LS.move_dual_step_items(k, its, 0.1, 0.0, 1.0, 1.0, 1.0, dataclasses.replace(PARS, dual_ls=2))
    k.finalize_b()


# ---- 5. select ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KINDS["banded"])
def test_select_after_set_direction_items(kind):
    B = 4
    k, its, dirs = batch_solver("banded", kind, B, "set")
    rounds = rounds_of("banded", B, dirs, "set")
    step_P, nx = LS.max_step_primal_items(k, np.stack([r.frac_predict for r in rounds]), PARS)
    for b in (2, 0):
        k.items_select(b)
        assert LS.max_step_primal(k, rounds[b].frac_predict, PARS) == (step_P[b], nx[b])
        assert k.dir is dirs[b]
    k.finalize_b()


# ---- 6. the oracle anchor ------------------------------------------------------------------------------------------------------------------
def test_batched_results_against_the_oracle():
    """Both paths could drift together: the batch against oracle/line_search_oracle.py on the d37 design (sums of 37 and 17 terms: their
    rounding stays orders of magnitude below the tolerance), with the rules of test_gpu_line_search.py -- exact for the max / min
    results, close(., ., 1e-12) for the sums."""
    B = 6
    name, kind = "d37", "schur"
    k, its, dirs = batch_solver(name, kind, B, "set")
    rounds = rounds_of(name, B, dirs, "set")
    got = batch_calls(k, its, rounds)
    close = lambda a, b, tol=1e-12: abs(a - b) <= tol * max(1.0, abs(b))
    for b in (0, 1, 2, 4, 5):                                  # item 3 holds the NaN: the oracle's dual_bounds asserts s > 0
        it, d, r = its[b], dirs[b], rounds[b]
        oit = KO.Iterate(x=it.x, y=it.y, s=it.s, mu=it.mu, J=it.J, H=it.H, grad=it.grad, cons=it.cons, a_norm_penalty_par=it.a_norm_penalty_par)
        od = KO.Direction(d.x, d.y, d.s, mu=d.mu)
        g = {f: np.frombuffer(v) if isinstance(v, bytes) else v for f, v in got[b].items()}
        assert g["nx"][0] == np.max(np.abs(d.x))
        assert g["step_P"][0] == LO.simple_max_step(oit.s, od.s, LO.lb_s_predict(oit, od, r.frac_predict, 0.5))
        assert bool(g["ok"]) == LO.s_bound_ok(oit, od, r.s_cand, r.frac, 0.5)
        assert tuple(g["range"]) == LO.dual_step_range(oit, od, r.s_cand, r.y_cand, r.mu_cand, 0.01, r.frac), (b, D.ROLES[b])
        exp = LO.predicted_reduction_terms(oit, od, r.alpha)
        assert g["pred"][1] == exp[1] and g["pred"][2] == exp[2]
        assert close(g["pred"][0], exp[0]) and close(g["pred"][3], exp[3]), (b, g["pred"], exp)
        ocand = KO.Iterate(x=it.x, y=r.y_cand, s=r.s_cand, mu=r.mu_cand, J=cand_J(it, r.J_scale), H=it.H, grad=r.grad_cand, cons=it.cons,
                           a_norm_penalty_par=it.a_norm_penalty_par)
        lb, ub = g["range"]
        if np.isfinite(r.y_cand).all():
            assert close(g["sd"][0], LO.move_dual_step(ocand, od, r.alpha, lb, ub, 1, r.scale_D, r.scale_mu)), b
    k.finalize_b()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    B = 4
    name, kind = "d37", "schur"
    its = family(name, B)
    dirs, _ = designed(name, B)
    k = KS.HIP_KKT_solver(kind)
    k.initialize_b(its[0])
    k._set_structure(its[0])
    lib, h = k._lib, k._k
    n, m = its[0].dim(), its[0].ncon()
    buf = L.f64(np.ones(B * max(n, m) * 4))
    ibuf = np.zeros(16, np.int32)
    p, ip = L.p_f64(buf), ibuf.ctypes.data_as(i32p)

    def refused(rc, word):
        assert rc == L.OKKT_ERR_INVALID and word in lib.okkt_kkt_last_error(h).decode(), (rc, lib.okkt_kkt_last_error(h))

    max_step = lambda nB, items=None, ni=0, fs=m, frac=p, out=p: lib.okkt_kkt_items_max_step_primal(h, nB, items, ni, frac, fs, 0.5, out, None)
    refused(max_step(B), "no slots are reserved")                                      # the gate of the family
    k.items_reserve(B)
    refused(lib.okkt_kkt_items_set_direction(h, B, p, p, p), "okkt_kkt_items_form_system has not been called")      # a direction call before form
    refused(max_step(B), "okkt_kkt_items_form_system has not been called")
    k.form_system_items(its[:3])
    refused(lib.okkt_kkt_items_set_direction(h, B, p, p, p), "B above the 3 items")
    refused(max_step(3), "no direction: ")                                             # formed, but no item holds a direction
    refused(lib.okkt_kkt_items_set_direction(h, 3, p, None, p), "a required array is NULL")
    LS.set_direction_items(k, dirs[:2])
    refused(max_step(3), "no direction: ")                                             # B above the items that hold one
    refused(max_step(B), "B above the 3 items")
    refused(max_step(2, frac=None), "a required array is NULL")
    refused(max_step(2, out=None), "a required array is NULL")
    refused(max_step(2, fs=m + 1), "frac_stride must be 0")
    for bad, word in (([0, 2], "outside 0 .. B-1"), ([1, 1], "listed twice"), ([-1, 0], "outside 0 .. B-1")):
        arr = np.array(bad, dtype=np.int32)
        refused(max_step(2, arr.ctypes.data_as(i32p), 2), word)
    refused(lib.okkt_kkt_items_s_bound_ok(h, 2, None, 0, p, p, 3, 0.5, ip), "frac_stride must be 0")
    refused(lib.okkt_kkt_items_s_bound_ok(h, 2, None, 0, None, p, m, 0.5, ip), "a required array is NULL")
    refused(lib.okkt_kkt_items_dual_step_range(h, 2, None, 0, p, p, None, 0.01, p, m, p, p), "a required array is NULL")
    refused(lib.okkt_kkt_items_predicted_reduction(h, 2, None, 0, None, p, p, p, p, p), "a required array is NULL")
    refused(lib.okkt_kkt_items_dual_step(h, 2, None, 0, None, 0, None, p, p, p, p, p, p, p, p, p, 1, p), "a required array is NULL")
    refused(lib.okkt_kkt_items_dual_step(h, 3, None, 0, None, 0, p, p, p, p, p, p, p, p, p, p, 0, p), "no direction: ")
    # the two items that hold a direction still answer, and so does the serial sequence with the LS.* calls on the same solver
    rounds = [round_of(name, B, b, dirs[b], "set") for b in range(2)]
    step_P, _ = LS.max_step_primal_items(k, np.stack([r.frac_predict for r in rounds]), PARS)
    assert [bts(v) for v in step_P] == [serial_ref(name, kind, B, b, "set")["step_P"] for b in range(2)]
    k.items_release()
    refused(max_step(2), "no slots are reserved")
    it = its[1]
    k.form_system_b(it)
    assert k.factor_b(D.DELTA[name]) in (0, 1)
    LS.set_direction(k, dirs[1])
    assert serial_calls(k, it, round_of(name, B, 1, dirs[1], "set")) == serial_ref(name, kind, B, 1, "set")
    k.finalize_b()
