"""KKT batches (okkt_kkt_items_*) against the single-iterate calls on a solver of its own per item: the assembled
matrix, schur_diag, diag_min, inertia and flag, the delta loop's (status, #fac, delta, warnings), the rhs triple, dx, dy, ds and the six
numbers of the N err -- as bytes, no tolerance anywhere except the oracle anchor.  The designed batches are kkt_items_ref.py's (their
predictions are checked on the host in test_kkt_items_host.py); the serial side is computed once per (item, kind, parameters) and shared."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import kkt_items_ref as IR
import lanczos_ref as R
from conftest import iterate_from_record
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, linear_solver_HIP
from oracle import kkt_oracle as KO

pytestmark = pytest.mark.gpu

KINDS = ["schur", "symmetric"]
ETAS = {"affine": KS.Reduct_affine, "stable": KS.Reduct_stable}
ERR_FIELDS = ("error_D", "error_P", "error_mu", "overall", "rhs_norm", "ratio")


def bts(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def pars_of(delta_max=None, itref=3):
    pars = KS.Class_parameters()
    pars.kkt.ItRefine_Num = itref
    if delta_max is not None:
        pars.delta.max = delta_max
    return pars


def err_bytes(e):
    return bts([getattr(e, f) for f in ERR_FIELDS])


def serial_run(it, kind, eta="affine", delta_max=None, itref=3, explicit_delta=None, keep=False):
    """The single-iterate sequence on a fresh solver: a dict of everything observable (bytes), and the solver itself with keep."""
    k = KS.HIP_KKT_solver(kind, pars_of(delta_max, itref))
    k.initialize_b(it)
    k.form_system_b(it)
    out = dict(A=bts(k.matrix().data), sd=bts(k.schur_diag), dmin=bts(k.diag_min()))
    if explicit_delta is None:
        prev = it.delta
        status, nfac, delta = k.ipopt_strategy_b(it)
        it.delta = prev
        out.update(loop=(status, nfac, bts(delta), k.diag_dom_warnings), delta=delta)
    else:
        out.update(flag=k.factor_b(explicit_delta), inertia=k.inertia, delta=explicit_delta)
    out["D"] = bts(linear_solver_HIP.of_kkt(k).diag())
    k.kkt_associate_rhs_b(it, ETAS[eta]())
    out["rhs"] = (bts(k.rhs.dual_r), bts(k.rhs.primal_r), bts(k.rhs.comp_r))
    try:
        k.compute_direction_b()
    except OkktError as e:              # check_for_nan of the mirror: the bytes are still what the device computed
        assert "NaN" in str(e)
    out["dir"] = (bts(k.dir.x), bts(k.dir.y), bts(k.dir.s))
    out["err"] = err_bytes(k.kkt_err_norm)
    if keep:
        return out, k
    k.finalize_b()
    return out


@functools.lru_cache(maxsize=None)
def serial_design(lam, prev, kind, eta="affine", delta_max=None, itref=3):
    return serial_run(IR.item(KS.Class_iterate, lam, prev), kind, eta, delta_max, itref)


def batch_solver(its, kind, delta_max=None, itref=3, reserve=None):
    k = KS.HIP_KKT_solver(kind, pars_of(delta_max, itref))
    k.initialize_b(its[0])
    k._set_structure(its[0])
    q = k.items_query()
    assert q["eligible"] == 1 and q["reason"] == L.OKKT_KKT_ITEMS_OK and q["bytes_per_item"] > 0
    k.items_reserve(reserve or len(its))
    return k


def selected(k, b):
    """Slot b in the solver's own state: (assembled values, schur_diag, D) as bytes."""
    k.items_select(b)
    return bts(k.matrix().data), bts(k.schur_diag), bts(linear_solver_HIP.of_kkt(k).diag()) if k.ready == "factored" else None


# ---- 1. form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_form_system_items(kind):
    lams = (-4e-4, -3.7, 0.5)
    its = IR.batch(KS.Class_iterate, lams)
    k = batch_solver(its, kind)
    k.form_system_items(its)
    dmin = k.diag_min_items()
    for b, lam in enumerate(lams):
        ref = serial_design(lam, 0.0, kind)
        A, sd, _ = selected(k, b)
        assert A == ref["A"] and sd == ref["sd"], b
        assert bts(dmin[b]) == ref["dmin"], b
        assert bts(k.diag_min()) == ref["dmin"]               # the single-iterate call on the selected slot
    k.finalize_b()


@pytest.mark.parametrize("kind", KINDS)
def test_form_system_items_shared_H(kind):
    """One H object for every item (an LP / QP sweep): it goes in with stride 0; s and y differ."""
    base = IR.item(KS.Class_iterate, -3.7)
    rng = np.random.default_rng(5)
    its = [dataclasses.replace(base, s=base.s * rng.uniform(0.5, 2.0, size=len(base.s)), y=base.y * rng.uniform(0.5, 2.0, size=len(base.y))) for _ in range(3)]
    assert all(it.H is base.H and it.J is base.J for it in its)
    k = batch_solver(its, kind)
    k.form_system_items(its)
    dmin = k.diag_min_items()
    refs = [serial_run(it, kind) for it in its]
    assert len({r["A"] for r in refs}) == 3
    for b in range(3):
        A, sd, _ = selected(k, b)
        assert (A, sd, bts(dmin[b])) == (refs[b]["A"], refs[b]["sd"], refs[b]["dmin"]), b
    # and the whole step on the shared values
    res, launches = k.ipopt_strategy_items(its)
    k.kkt_associate_rhs_items(its, KS.Reduct_affine())
    dirs, errs = k.compute_direction_items()
    for b in range(3):
        assert (res[b][0], res[b][1], bts(res[b][2])) == refs[b]["loop"][:3]
        assert (bts(dirs[b].x), bts(dirs[b].y), bts(dirs[b].s)) == refs[b]["dir"] and err_bytes(errs[b]) == refs[b]["err"]
    k.finalize_b()


# ---- 2. explicit delta ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_factor_items_explicit_delta(kind):
    deltas = (0.0, 0.5, 1e3)
    its = [IR.item(KS.Class_iterate, -3.7) for _ in deltas]
    refs = [serial_run(its[b], kind, explicit_delta=d) for b, d in enumerate(deltas)]
    assert [r["flag"] for r in refs] == [0, 0, 1]
    k = batch_solver(its, kind)
    k.form_system_items(its)
    flags, inertias = k.factor_items(deltas)
    assert flags == [r["flag"] for r in refs] and inertias == [r["inertia"] for r in refs]
    k.kkt_associate_rhs_items(its, KS.Reduct_affine())
    dirs, errs = k.compute_direction_items()          # a direction whatever the flag, as in the reference
    for b in range(3):
        assert selected(k, b)[2] == refs[b]["D"]
        assert (bts(dirs[b].x), bts(dirs[b].y), bts(dirs[b].s)) == refs[b]["dir"] and err_bytes(errs[b]) == refs[b]["err"]
    k.finalize_b()


@pytest.mark.parametrize("kind", KINDS)
def test_nan_item_stays_in_its_slot(kind):
    its = [IR.item(KS.Class_iterate, lam) for lam in (-3.7, -3.7, -4e-4)]
    H = its[1].H.copy()
    H.data[len(H.data) // 2] = np.nan
    its[1] = dataclasses.replace(its[1], H=H)
    refs = [serial_run(it, kind, explicit_delta=5.0) for it in its]
    assert refs[1]["flag"] == 0 and refs[1]["inertia"][3] > 0
    k = batch_solver(its, kind)
    k.form_system_items(its)
    flags, inertias = k.factor_items([5.0] * 3)
    assert flags == [r["flag"] for r in refs] == [1, 0, 1]
    assert inertias == [r["inertia"] for r in refs]
    k.kkt_associate_rhs_items(its, KS.Reduct_affine())
    with pytest.raises(OkktError, match=r"NaN in \w \(item 1\)"):          # check_for_nan, as compute_direction_b
        k.compute_direction_items()
    dirs, errs = k.compute_direction_items(check_nan=False)
    for b in (0, 2):
        assert selected(k, b) == (refs[b]["A"], refs[b]["sd"], refs[b]["D"])
        assert (bts(dirs[b].x), bts(dirs[b].y), bts(dirs[b].s)) == refs[b]["dir"] and err_bytes(errs[b]) == refs[b]["err"]
    k.finalize_b()


# ---- 3. + 4. the delta loop, the rhs and the direction -----------------------------------------------------------------------------------
def run_batch(lams, prevs, kind, eta="affine", delta_max=None, itref=3, resident=False):
    """The batched step on the designs against the serial one and the host model; returns the loop's results and the launches."""
    its = IR.batch(KS.Class_iterate, lams, prevs)
    k = batch_solver(its, kind, delta_max, itref)
    k.form_system_items(its)
    res, launches = k.ipopt_strategy_items(its)
    d = pars_of(delta_max).delta
    want = [IR.predict(lam, prev, d) for lam, prev in zip(lams, prevs)]
    print(f"{kind} B={len(lams)} launches {launches} results {res}")
    assert res == want
    assert launches == max(w[1] for w in want)
    assert [it.delta for it in its] == [w[2] for w in want]
    rhs = k.kkt_associate_rhs_items(its, ETAS[eta]())
    dirs, errs = k.compute_direction_items(resident=resident)
    for b, (lam, prev) in enumerate(zip(lams, prevs)):
        ref = serial_design(lam, prev, kind, eta, delta_max, itref)
        assert (res[b][0], res[b][1], bts(res[b][2]), k.items_diag_dom_warnings[b]) == ref["loop"], b
        assert (bts(rhs[b].dual_r), bts(rhs[b].primal_r), bts(rhs[b].comp_r)) == ref["rhs"], b
        assert err_bytes(errs[b]) == ref["err"], b
        if resident:
            k.items_select(b)
            n, m = its[b].dim(), its[b].ncon()
            dx, dy, ds = np.zeros(n), np.zeros(m), np.zeros(m)
            k._check(k._lib.okkt_kkt_get_direction(k._k, L.p_f64(dx), L.p_f64(dy), L.p_f64(ds)), "okkt_kkt_get_direction")
            assert (bts(dx), bts(dy), bts(ds)) == ref["dir"], b
        else:
            assert (bts(dirs[b].x), bts(dirs[b].y), bts(dirs[b].s)) == ref["dir"], b
    k.finalize_b()
    return res, launches


@pytest.mark.parametrize("eta", sorted(ETAS))
@pytest.mark.parametrize("kind,itref", [("schur", 1), ("schur", 3), ("symmetric", 3)])
def test_loop_rhs_direction_four_designs(kind, itref, eta):
    res, launches = run_batch(IR.LAMS, [0.0] * 4, kind, eta, itref=itref)
    assert res[0] == ("success", 1, 0.0) and len({r[1] for r in res}) == 4


@pytest.mark.parametrize("kind", KINDS)
def test_direction_stays_resident(kind):
    run_batch(IR.LAMS, [0.0] * 4, kind, resident=True)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_of_one(kind):
    run_batch([-3.7], [0.0], kind)


@pytest.mark.parametrize("kind", KINDS)
def test_sixteen_items_with_previous_deltas(kind):
    lams, prevs = IR.sixteen()
    run_batch(lams, prevs, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_all_convex_batch_is_one_launch(kind):
    res, launches = run_batch([0.5] * 3, [0.0] * 3, kind)
    assert launches == 1 and res == [("success", 1, 0.0)] * 3


@pytest.mark.parametrize("kind", KINDS)
def test_delta_max_fails_item_3_alone_and_it_still_gives_a_direction(kind):
    """delta_max below what item 3 needs: status 0 for that item alone (in the last round), and run_batch compares its direction, from
    the failed factor, as bytes like the others'."""
    res, launches = run_batch(IR.LAMS, [0.0] * 4, kind, delta_max=IR.DELTA_MAX_LOW)
    assert [r[0] for r in res] == ["success", "success", "success", "failure"]
    assert res[2] == ("success", 10, 16.777216) and res[3] == ("failure", 11, 134.217728) and launches == 11


@pytest.mark.parametrize("kind", KINDS)
def test_item_leaves_with_status_0_while_another_goes_on(kind):
    """The same delta_max with a previous delta on item 3: it passes delta_max in round 5 and keeps that failed factor in its slot
    while item 2 makes five more attempts over an item list without it and succeeds; the direction of item 3 (compared in run_batch)
    comes from the factor it left with, not from anything a later round wrote."""
    res, launches = run_batch(IR.LAMS, list(IR.DELTA_MAX_PREVS), kind, delta_max=IR.DELTA_MAX_LOW)
    assert [r[0] for r in res] == ["success", "success", "success", "failure"]
    assert res[3][1] == 5 and res[2] == ("success", 10, 16.777216) and launches == 10


# ---- 5. select ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_select_leaves_the_serial_state(kind):
    its = IR.batch(KS.Class_iterate, IR.LAMS)
    k = batch_solver(its, kind)
    k.form_system_items(its)
    k.ipopt_strategy_items(its)
    k.kkt_associate_rhs_items(its, KS.Reduct_stable())
    k.compute_direction_items(resident=True)
    k.items_select(2)
    ref, ks = serial_run(IR.item(KS.Class_iterate, IR.LAMS[2]), kind, "stable", keep=True)
    assert (bts(k.matrix().data), bts(k.schur_diag)) == (ref["A"], ref["sd"])
    assert (bts(k.rhs.dual_r), bts(k.rhs.primal_r), bts(k.rhs.comp_r)) == ref["rhs"]      # the mirror's rhs is the item's triple
    k.compute_direction_b()                                  # the single-iterate call on the resident rhs of the slot
    assert (bts(k.dir.x), bts(k.dir.y), bts(k.dir.s)) == ref["dir"] and err_bytes(k.kkt_err_norm) == ref["err"]
    assert k.condest() == ks.condest()
    assert k.is_diag_dom() == ks.is_diag_dom()
    # another reduction on the selected slot goes through the single-iterate rhs as well
    for s in (k, ks):
        s.kkt_associate_rhs_b(s.factor_it, KS.Reduct_affine())
        s.compute_direction_b()
    assert bts(k.dir.x) == bts(ks.dir.x) and bts(k.dir.y) == bts(ks.dir.y) and bts(k.dir.s) == bts(ks.dir.s)
    ks.finalize_b()
    k.finalize_b()


# ---- 6. a tree with several levels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_h", [40, 400])
def test_hanging_chain_levels_meet_the_item_list(N_h):
    """The hanging chain at the size tests/test_gpu_batch.py uses (40 intervals: the KKT handle's plan is one level of tasks) and at 400
    intervals (n + m = 1608: several levels), where the level lists and the item list of the delta loop meet."""
    prob = synth.hanging_chain(N_h=N_h)
    rng = np.random.default_rng(2)
    n, m = prob["n"], prob["m"]
    grad, cons = rng.normal(size=n), prob["s"] + 0.1 * rng.normal(size=m)
    its = [KS.Class_iterate(x=np.zeros(n), y=prob["y"] * rng.uniform(0.3, 3.0, size=m), s=prob["s"] * rng.uniform(0.3, 3.0, size=m), mu=prob["mu"], J=prob["J"],
                            H=prob["H"] * (1.0 if b % 2 == 0 else -0.5 * b), grad=grad * (1 + b), cons=cons) for b in range(4)]
    k = batch_solver(its, "symmetric")
    levels = linear_solver_HIP.of_kkt(k).batch_query()["levels"]
    assert levels > 1 or N_h == 40
    k.form_system_items(its)
    res, launches = k.ipopt_strategy_items(its)
    k.kkt_associate_rhs_items(its, KS.Reduct_affine())
    dirs, errs = k.compute_direction_items()
    for it in its:
        it.delta = 0.0
    refs = [serial_run(it, "symmetric") for it in its]
    print(f"chain{N_h}: levels {levels}", res, launches)
    assert len({r[1] for r in res}) > 1                        # the items leave the loop in different rounds
    assert launches == max(r[1] for r in res)
    for b in range(4):
        assert (res[b][0], res[b][1], bts(res[b][2]), k.items_diag_dom_warnings[b]) == refs[b]["loop"], b
        assert (bts(dirs[b].x), bts(dirs[b].y), bts(dirs[b].s)) == refs[b]["dir"] and err_bytes(errs[b]) == refs[b]["err"], b
        assert selected(k, b)[2] == refs[b]["D"], b
    k.finalize_b()


# ---- 7. the item list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_round_over_a_subset_leaves_the_other_slots(kind):
    its = IR.batch(KS.Class_iterate, [-3.7] * 4)
    k = batch_solver(its, kind)
    k.form_system_items(its)
    i32 = C.POINTER(C.c_int32)
    # a list that leaves slots out before any factorisation of the batch: refused (slots 0 and 2 would hold no factor)
    first = np.array([1, 3], dtype=np.int32)
    fl = np.zeros(4, dtype=np.int32)
    assert k._lib.okkt_debug_kkt_items_factor_list(k._k, 4, first.ctypes.data_as(i32), 2, L.p_f64(np.full(4, 7.0)), fl.ctypes.data_as(i32)) == L.OKKT_ERR_INVALID
    assert "leaves slots out" in k._lib.okkt_kkt_last_error(k._k).decode()
    k.factor_items([7.0, 7.0, 7.0, 7.0])
    ls = linear_solver_HIP.of_kkt(k)

    def D(b):
        ls.batch_select(b)
        return bts(ls.diag())

    before = [D(b) for b in range(4)]
    assert len(set(before)) == 1
    items = np.array([1, 3], dtype=np.int32)
    delta = L.f64(np.array([11.0, 0.25, 13.0, 900.0]))
    flags = np.full(4, -7, dtype=np.int32)
    k._check(k._lib.okkt_debug_kkt_items_factor_list(k._k, 4, items.ctypes.data_as(i32), 2, L.p_f64(delta), flags.ctypes.data_as(i32)), "factor list")
    assert list(flags) == [-7, 0, -7, 1]
    after = [D(b) for b in range(4)]
    assert after[0] == before[0] and after[2] == before[2]
    assert after[1] == serial_run(its[1], kind, explicit_delta=0.25)["D"] and after[3] == serial_run(its[3], kind, explicit_delta=900.0)["D"]
    # a slot named twice, or outside the batch, is refused
    bad = np.array([1, 1], dtype=np.int32)
    assert k._lib.okkt_debug_kkt_items_factor_list(k._k, 4, bad.ctypes.data_as(i32), 2, L.p_f64(delta), flags.ctypes.data_as(i32)) == L.OKKT_ERR_INVALID
    bad = np.array([1, 4], dtype=np.int32)
    assert k._lib.okkt_debug_kkt_items_factor_list(k._k, 4, bad.ctypes.data_as(i32), 2, L.p_f64(delta), flags.ctypes.data_as(i32)) == L.OKKT_ERR_INVALID
    k.finalize_b()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def _serial_still_runs(k, it, kind, **kw):
    it.delta = 0.0
    k.form_system_b(it)
    status, nfac, delta = k.ipopt_strategy_b(it)
    it.delta = 0.0
    k.kkt_associate_rhs_b(it, KS.Reduct_affine())
    k.compute_direction_b()
    assert np.all(np.isfinite(k.dir.x)) and status == "success"
    return status, nfac, delta


def test_refused_kinds_and_options(golden):
    it = IR.item(KS.Class_iterate, -3.7)
    cases = [("schur_direct", {}, it, L.OKKT_KKT_ITEMS_SCHUR_DIRECT, "Schur-direct"),
             ("schur", dict(schur_dense_rows=2), it, L.OKKT_KKT_ITEMS_DENSE_ROWS, "schur_dense_rows"),
             ("symmetric", dict(hip_ls_scaling=1), it, L.OKKT_KKT_ITEMS_SCALING, "scaling"),
             ("symmetric", dict(hip_ls_refine_steps=2), it, L.OKKT_KKT_ITEMS_LS_REFINE, "okkt_kkt_set_ls_refine"),
             ("clever_symmetric", {}, iterate_from_record(golden["toy_lps"][0], KS.Class_iterate), L.OKKT_KKT_ITEMS_CLEVER, "clever-symmetric")]
    for kind, opts, itk, reason, word in cases:
        k = KS.HIP_KKT_solver(kind, **opts)
        k.initialize_b(itk)
        if k._pattern is None:          # (initialize! of the clever-symmetric kind sets the structure itself)
            assert k.items_query()["reason"] == L.OKKT_KKT_ITEMS_NO_STRUCTURE      # the first reason, whatever the kind
        k._set_structure(itk)
        q = k.items_query()
        assert (q["eligible"], q["reason"]) == (0, reason), kind
        for call in (lambda: k.items_reserve(2), lambda: k.form_system_items([itk, itk])):
            with pytest.raises(OkktError, match=word):
                call()
        with pytest.raises(OkktError, match="form_system_items has not been called"):
            k.diag_min_items()
        assert k._lib.okkt_kkt_items_select(k._k, 0) == L.OKKT_ERR_INVALID and word in k._lib.okkt_kkt_last_error(k._k).decode()
        assert k._lib.okkt_kkt_items_reserve(k._k, 2) == L.OKKT_ERR_INVALID
        _serial_still_runs(k, itk, kind)
        k.finalize_b()
    # the order: on a handle to which two reasons apply the earlier code answers
    big = R.indefinite_design(KS.Class_iterate, 1031, -3.7)
    both = [("schur_direct", dict(schur_dense_rows=2), it, L.OKKT_KKT_ITEMS_SCHUR_DIRECT, "Schur-direct"),
            ("schur", dict(schur_dense_rows=2, hip_ls_scaling=1), it, L.OKKT_KKT_ITEMS_DENSE_ROWS, "schur_dense_rows"),
            ("symmetric", dict(hip_ls_scaling=1, hip_ls_refine_steps=2), it, L.OKKT_KKT_ITEMS_SCALING, "scaling"),
            ("schur_direct", {}, big, L.OKKT_KKT_ITEMS_SCHUR_DIRECT, "Schur-direct"),
            ("schur", dict(hip_ls_scaling=1), big, L.OKKT_KKT_ITEMS_SCALING, "scaling")]
    for kind, opts, itk, reason, word in both:
        k = KS.HIP_KKT_solver(kind, **opts)
        k.initialize_b(itk)
        k._set_structure(itk)
        assert k.items_query()["reason"] == reason, (kind, opts)
        with pytest.raises(OkktError, match=word):
            k.items_reserve(2)
        k.finalize_b()
    # a plan with big fronts: the reason of okkt_batch_query is passed on
    k = KS.HIP_KKT_solver("schur")
    k.initialize_b(big)
    k._set_structure(big)
    assert k.items_query()["reason"] == L.OKKT_KKT_ITEMS_PLAN + L.OKKT_BATCH_BIG_FRONTS
    with pytest.raises(OkktError, match="takes no uniform batch"):
        k.items_reserve(2)
    _serial_still_runs(k, big, "schur")
    k.finalize_b()


@pytest.mark.parametrize("kind", KINDS)
def test_calls_out_of_order(kind):
    its = IR.batch(KS.Class_iterate, IR.LAMS)
    k = KS.HIP_KKT_solver(kind)
    k.initialize_b(its[0])
    k._set_structure(its[0])
    lib, h = k._lib, k._k
    buf = np.zeros(4 * 64)
    ibuf = np.zeros(16, np.int32)
    p, ip = L.p_f64(buf), ibuf.ctypes.data_as(C.POINTER(C.c_int32))

    def refused(rc, word):
        assert rc == L.OKKT_ERR_INVALID and word in lib.okkt_kkt_last_error(h).decode(), lib.okkt_kkt_last_error(h)

    refused(lib.okkt_kkt_items_diag_min(h, 1, p), "no slots are reserved")
    refused(lib.okkt_kkt_items_reserve(h, 0), "outside 1 .. 65535")
    refused(lib.okkt_kkt_items_reserve(h, 65536), "outside 1 .. 65535")
    k.items_reserve(3)
    with pytest.raises(OkktError, match="B must be in 1 .. the reserved 3"):
        k.form_system_items(its)                                                     # B above the reservation
    refused(lib.okkt_kkt_items_factor(h, 3, p, None, ip), "kkt solver not ready to factor: form_system has not been called")
    refused(lib.okkt_kkt_items_ipopt_strategy(h, 3, p, None, ip, ip, p, ip, ip), "form_system has not been called")
    refused(lib.okkt_kkt_items_system_rhs(h, 3, p, p, p, p, p, p, 0.0, 0.0, 0.0, None, None, None), "form_system has not been called")   # rhs before form
    refused(lib.okkt_kkt_items_select(h, 0), "okkt_kkt_items_select: b outside")
    three = its[:3]
    k.form_system_items(three)
    refused(lib.okkt_kkt_items_compute_direction(h, 3, 3, None, None, None, None), "kkt solver not ready to compute direction!")   # before factor
    k.ipopt_strategy_items(three)
    refused(lib.okkt_kkt_items_compute_direction(h, 3, 3, None, None, None, None), "no resident rhs")
    refused(lib.okkt_kkt_items_compute_direction(h, 3, 3, p, None, None, None), "three host vectors or three NULLs")
    # the delta-candidate batch takes the linear solver's slots for itself: the reservation says so, and a new one works
    k.items_select(1)
    k.ipopt_strategy_batch(three[1], 8)
    refused(lib.okkt_kkt_items_diag_min(h, 3, p), "have been replaced")
    k.items_reserve(4)
    for it in its:
        it.delta = 0.0
    k.form_system_items(its)
    res, _ = k.ipopt_strategy_items(its)
    assert res == [IR.predict(lam, 0.0, KS.Class_delta_parameters()) for lam in IR.LAMS]
    k.items_release()
    refused(lib.okkt_kkt_items_diag_min(h, 1, p), "no slots are reserved")
    lsh = C.c_void_p(lib.okkt_kkt_linear_solver(h))                                  # the linear solver's slots went with the reservation
    assert lib.okkt_batch_select(lsh, 0) == L.OKKT_ERR_INVALID and b"no slots are reserved" in lib.okkt_last_error(lsh)
    _serial_still_runs(k, its[2], kind)
    k.finalize_b()


# ---- 9. the oracle anchor -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_directions_against_the_oracle(kind):
    """Both paths could drift together: the batch's directions against oracle/kkt_oracle.py at the deltas the loop ended with, at the
    tolerance tests/test_gpu_kkt_solvers.py::test_synthetic_directions_vs_oracle uses for the same quantity (1e-9 of max(1, |d|_inf))."""
    its = IR.batch(KS.Class_iterate, IR.LAMS)
    k = batch_solver(its, kind)
    k.form_system_items(its)
    res, _ = k.ipopt_strategy_items(its)
    k.kkt_associate_rhs_items(its, KS.Reduct_affine())
    dirs, errs = k.compute_direction_items()
    perm = k.linear_solver_perm()
    for b, lam in enumerate(IR.LAMS):
        ito = R.indefinite_design(KO.Iterate, IR.N, lam)
        ko = KO.pick_KKT_solver(kind, perm=perm)
        ko.initialize_b(ito)
        ko.form_system_b(ito)
        assert ko.factor_b(res[b][2]) == 1
        ko.kkt_associate_rhs_b(ito, KO.Reduct_affine())
        ko.compute_direction_b()
        for a in ("x", "y", "s"):
            da, db = getattr(dirs[b], a), getattr(ko.dir, a)
            assert np.max(np.abs(da - db)) <= 1e-9 * max(1.0, np.max(np.abs(db))), (b, a, np.max(np.abs(da - db)))
    k.finalize_b()
