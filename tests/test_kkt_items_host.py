"""KKT batches (okkt_kkt_items_*), what needs no GPU: the designed batches of kkt_items_ref.py keep their
distance from the attempt grid and tell their items apart, the attempt sequencing of the loop over items (csrc/kkt_items_seq.h, through
its host-only hook) returns what the spectrum predicts, the symbols exist, and a handle without a device answers the query and is refused
by everything else."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kkt_items_ref as IR
import lanczos_ref as R
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["okkt_kkt_items_query", "okkt_kkt_items_reserve", "okkt_kkt_items_release", "okkt_kkt_items_form_system", "okkt_kkt_items_diag_min",
         "okkt_kkt_items_factor", "okkt_kkt_items_ipopt_strategy", "okkt_kkt_items_system_rhs", "okkt_kkt_items_compute_direction",
         "okkt_kkt_items_select"]


def delta_pars(delta_max=None):
    d = KS.Class_delta_parameters()
    if delta_max is not None:
        d.max = delta_max
    return d


def designed_batches():
    """(name, lams, prevs, delta parameters) of every batch the device tests run the loop on."""
    l16, p16 = IR.sixteen()
    return [("four", list(IR.LAMS), [0.0] * 4, delta_pars()),
            ("one", [-3.7], [0.0], delta_pars()),
            ("sixteen", l16, p16, delta_pars()),
            ("convex", [0.5] * 3, [0.0] * 3, delta_pars()),
            ("delta-max", list(IR.LAMS), [0.0] * 4, delta_pars(IR.DELTA_MAX_LOW)),
            ("delta-max-early", list(IR.LAMS), list(IR.DELTA_MAX_PREVS), delta_pars(IR.DELTA_MAX_LOW))]


def test_one_pattern_for_every_lam():
    its = IR.batch(KS.Class_iterate, IR.LAMS)
    for it in its[1:]:
        for a, b in ((it.H.indptr, its[0].H.indptr), (it.H.indices, its[0].H.indices), (it.J.indptr, its[0].J.indptr), (it.J.indices, its[0].J.indices)):
            assert np.array_equal(a, b)
    # the convex item is positive definite, the others are not
    assert np.linalg.eigvalsh(R.dense_q(its[0]))[0] > 0.0
    for lam in IR.LAMS[1:]:
        assert IR.spectrum(lam)[1] < 0.0 and abs(IR.spectrum(lam)[1] / lam - 1.0) < 1e-9


@pytest.mark.parametrize("name,lams,prevs,d", designed_batches(), ids=[b[0] for b in designed_batches()])
def test_designed_batches_keep_their_margin(name, lams, prevs, d):
    for lam, prev in zip(lams, prevs):
        if lam < 0.0:
            assert IR.margin(lam, prev, d) >= 0.1, (lam, prev)          # no attempt within 10 % of -lambda_min


def test_predictions_differ_between_items():
    d = delta_pars()
    four = [IR.predict(lam, 0.0, d) for lam in IR.LAMS]
    assert four[0] == ("success", 1, 0.0)
    assert len({p[1] for p in four}) == 4 and len({p[2] for p in four}) == 4          # a batch that ignored the item index would not pass
    l16, p16 = IR.sixteen()
    sixteen = [IR.predict(lam, prev, d) for lam, prev in zip(l16, p16)]
    assert sum(1 for p in p16 if p != 0.0) == 8
    for b in range(4, 8):
        assert p16[b] != p16[b - 4]
        if l16[b] < 0.0:
            assert sixteen[b] != sixteen[b - 4], b                     # the previous delta moves an item's result
    # delta_max below what item 3 needs: status 0 for that item alone -- in the last round with no previous delta, in round 5 of 10 with one
    low = [IR.predict(lam, 0.0, delta_pars(IR.DELTA_MAX_LOW)) for lam in IR.LAMS]
    assert [p[0] for p in low] == ["success", "success", "success", "failure"]
    assert low[2] == ("success", 10, 16.777216) and low[3] == ("failure", 11, 134.217728)
    early = [IR.predict(lam, prev, delta_pars(IR.DELTA_MAX_LOW)) for lam, prev in zip(IR.LAMS, IR.DELTA_MAX_PREVS)]
    assert [p[0] for p in early] == ["success", "success", "success", "failure"]
    assert early[3][1] == 5 and 100.0 < early[3][2] < 900.0 and early[1][1] == 5 and early[2][1] == 10      # item 2 outlasts the failed one by five rounds


def _model(lams, prevs, d):
    """The loop over items of the library, host only: an attempt succeeds when delta >= need = -lambda_min (the margin keeps every attempt
    away from equality)."""
    lib = L.load()
    B = len(lams)
    p = L.OkktKktPars()
    lib.okkt_kkt_default_pars(C.byref(p))
    p.delta_start, p.delta_min, p.delta_max, p.delta_inc, p.delta_dec, p.delta_zero = d.start, d.min, d.max, d.inc, d.dec, d.zero
    dmin = L.f64(np.array([IR.spectrum(lam)[0] for lam in lams]))
    need = L.f64(np.array([-IR.spectrum(lam)[1] for lam in lams]))
    prev = L.f64(np.array(prevs, dtype=float))
    status, nfac = np.zeros(B, np.int32), np.zeros(B, np.int32)
    delta = np.zeros(B)
    launches = C.c_int32()
    i32 = C.POINTER(C.c_int32)
    rc = lib.okkt_debug_items_loop_model(B, L.p_f64(dmin), L.p_f64(prev), L.p_f64(need), C.byref(p), status.ctypes.data_as(i32), nfac.ctypes.data_as(i32),
                                         L.p_f64(delta), C.byref(launches))
    assert rc == L.OKKT_OK
    return [("success" if s == 1 else "failure", int(f), float(dl)) for s, f, dl in zip(status, nfac, delta)], launches.value


@pytest.mark.parametrize("name,lams,prevs,d", designed_batches(), ids=[b[0] for b in designed_batches()])
def test_loop_over_items_returns_the_predictions(name, lams, prevs, d):
    got, launches = _model(lams, prevs, d)
    want = [IR.predict(lam, prev, d) for lam, prev in zip(lams, prevs)]
    assert got == want                                                # the same scalar arithmetic: equal doubles
    assert launches == max(p[1] for p in want)


def test_symbols():
    lib = L.load()
    txt = open(os.path.join(ROOT, "include", "okkt.h")).read()
    assert "okkt_kkt_items_info" in txt
    for name in NAMES + ["okkt_debug_items_loop_model", "okkt_debug_kkt_items_factor_list"]:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name + " is not declared in include/okkt.h"
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    for m in ("items_query", "items_reserve", "items_release", "form_system_items", "diag_min_items", "factor_items", "ipopt_strategy_items",
              "kkt_associate_rhs_items", "compute_direction_items", "items_select"):
        assert callable(getattr(KS.HIP_KKT_solver, m))


def _host_handle(lib, kind):
    o = L.OkktOpts()
    assert lib.okkt_default_opts(C.byref(o)) == 0
    o.host_symbolic_only = 1
    k = C.c_void_p()
    assert lib.okkt_kkt_create(C.byref(k), C.byref(o), kind) == 0
    return k


@pytest.mark.parametrize("kind", [L.OKKT_KKT_SCHUR, L.OKKT_KKT_SYMMETRIC, L.OKKT_KKT_CLEVER_SYMMETRIC, L.OKKT_KKT_SCHUR_DIRECT])
def test_host_symbolic_only_handle(kind):
    """The query answers without a device; a handle without a device never gets a structure, so "structure not set" is the first reason
    for every kind (it precedes the kind's own).  Every device entry point returns OKKT_ERR_NO_DEVICE."""
    lib = L.load()
    k = _host_handle(lib, kind)
    info = L.OkktKktItemsInfo()
    assert lib.okkt_kkt_items_query(k, C.byref(info)) == L.OKKT_OK
    assert (info.eligible, info.reason, info.bytes_per_item) == (0, L.OKKT_KKT_ITEMS_NO_STRUCTURE, 0)
    assert lib.okkt_kkt_items_query(k, None) == L.OKKT_ERR_INVALID
    buf = np.zeros(64)
    ibuf = np.zeros(64, np.int32)
    i32 = C.POINTER(C.c_int32)
    p, ip = L.p_f64(buf), ibuf.ctypes.data_as(i32)
    calls = [lambda: lib.okkt_kkt_items_reserve(k, 4),
             lambda: lib.okkt_kkt_items_form_system(k, 1, p, 0, p, 0, p, p),
             lambda: lib.okkt_kkt_items_diag_min(k, 1, p),
             lambda: lib.okkt_kkt_items_factor(k, 1, p, None, ip),
             lambda: lib.okkt_kkt_items_ipopt_strategy(k, 1, p, None, ip, ip, p, ip, ip),
             lambda: lib.okkt_kkt_items_system_rhs(k, 1, p, p, p, p, p, p, 0.0, 0.0, 0.0, None, None, None),
             lambda: lib.okkt_kkt_items_compute_direction(k, 1, 3, None, None, None, None),
             lambda: lib.okkt_kkt_items_select(k, 0)]
    for call in calls:
        assert call() == L.OKKT_ERR_NO_DEVICE
        assert b"no HIP device" in lib.okkt_kkt_last_error(k)
    assert lib.okkt_kkt_items_release(k) == L.OKKT_OK
    assert lib.okkt_kkt_destroy(k) == L.OKKT_OK
