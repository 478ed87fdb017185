"""Line-search batches (okkt_kkt_items_max_step_primal ...), what needs no GPU: the symbols exist and agree with
the Python signatures, a handle without a device answers the query and is refused by every device entry point, and the designed families
and directions of ls_items_designs.py have the properties the device tests rely on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ls_items_designs as D
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import line_search as LS
from oracle import line_search_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["okkt_kkt_items_set_direction", "okkt_kkt_items_max_step_primal", "okkt_kkt_items_s_bound_ok", "okkt_kkt_items_dual_step_range",
         "okkt_kkt_items_predicted_reduction", "okkt_kkt_items_dual_step", "okkt_kkt_items_ls_query"]


def test_symbols():
    lib = L.load()
    txt = open(os.path.join(ROOT, "include", "okkt.h")).read()
    assert "okkt_kkt_items_ls_info" in txt
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name + " is not declared in include/okkt.h"
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    for f in ("set_direction_items", "max_step_primal_items", "s_bound_ok_items", "dual_step_range_items", "predicted_reduction_terms_items",
              "move_dual_step_items"):
        assert callable(getattr(LS, f))
    # the struct of the family and every existing signature stay as they were
    assert [f for f, _ in L.OkktKktItemsInfo._fields_] == ["eligible", "reason", "bytes_per_item", "launches_form", "launches_direction"]


@pytest.mark.parametrize("kind", [L.OKKT_KKT_SCHUR, L.OKKT_KKT_SYMMETRIC])
def test_host_symbolic_only_handle(kind):
    lib = L.load()
    o = L.OkktOpts()
    assert lib.okkt_default_opts(C.byref(o)) == 0
    o.host_symbolic_only = 1
    k = C.c_void_p()
    assert lib.okkt_kkt_create(C.byref(k), C.byref(o), kind) == 0
    info = L.OkktKktItemsLsInfo()
    assert lib.okkt_kkt_items_ls_query(k, C.byref(info)) == L.OKKT_OK
    assert (info.eligible, info.reason, info.extra_bytes_per_item) == (0, L.OKKT_KKT_ITEMS_NO_STRUCTURE, 0)
    assert lib.okkt_kkt_items_ls_query(k, None) == L.OKKT_ERR_INVALID
    buf = np.ones(64)
    ibuf = np.zeros(64, np.int32)
    p, ip = L.p_f64(buf), ibuf.ctypes.data_as(C.POINTER(C.c_int32))
    calls = [lambda: lib.okkt_kkt_items_set_direction(k, 1, p, p, p),
             lambda: lib.okkt_kkt_items_max_step_primal(k, 1, None, 0, p, 0, 0.5, p, p),
             lambda: lib.okkt_kkt_items_s_bound_ok(k, 1, None, 0, p, p, 0, 0.5, ip),
             lambda: lib.okkt_kkt_items_dual_step_range(k, 1, None, 0, p, p, p, 0.01, p, 0, p, p),
             lambda: lib.okkt_kkt_items_predicted_reduction(k, 1, None, 0, p, p, p, p, p, p),
             lambda: lib.okkt_kkt_items_dual_step(k, 1, None, 0, None, 0, p, p, p, p, p, p, p, p, p, p, 1, p)]
    for call in calls:
        assert call() == L.OKKT_ERR_NO_DEVICE
        assert b"no HIP device" in lib.okkt_kkt_last_error(k)
    assert lib.okkt_kkt_destroy(k) == L.OKKT_OK


@pytest.mark.parametrize("name", sorted(D.SIZES))
def test_families_share_one_structure_and_differ_in_values(name):
    its = D.family(name, KS.Class_iterate, 4)
    n, m = D.SIZES[name]
    assert (its[0].dim(), its[0].ncon()) == (n, m)
    for it in its[1:]:
        for a, b in ((it.H.indptr, its[0].H.indptr), (it.H.indices, its[0].H.indices), (it.J.indptr, its[0].J.indptr), (it.J.indices, its[0].J.indices)):
            assert np.array_equal(a, b)
    for attr in ("s", "y", "grad"):
        assert len({np.asarray(getattr(it, attr)).tobytes() for it in its}) == 4
    assert len({it.mu for it in its}) == 4 and len({it.a_norm_penalty_par for it in its}) == 4
    assert all(np.all(it.s > 0) and np.all(it.y > 0) for it in its)
    # the partition of a map-reduce launch: min(256, ceil(len / 1024)) workgroups
    wg = lambda length: min(256, -(-length // 1024))
    assert (wg(n), wg(m)) == {"d37": (1, 1), "banded": (2, 3), "chain": (2, 2)}[name]
    if name == "d37":
        assert n + m < 256 and len({it.H.data.tobytes() for it in its}) == 4
    if name == "banded":
        assert all(it.H is its[0].H and it.J is its[0].J for it in its)
        H, J = its[0].H.tocoo(), its[0].J.tocsr()
        assert np.all((H.row - H.col >= 0) & (H.row - H.col <= 1))
        for i in (0, 1, m // 2, m - 1):
            c0 = (i * (n - 2)) // m
            assert list(J.indices[J.indptr[i]:J.indptr[i + 1]]) == [c0, c0 + 1, c0 + 2]
    if name == "chain":
        assert m - 1024 == 22 and n - 1024 == 18          # the second workgroup is almost empty


def _np_resets(s, mu, y, dy, cf):
    """The rows of dual_bounds' loop that set (lb, ub) = (0, -1), with numpy."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ub_dy = mu / (cf * s * dy) - y / dy
        lb_dy = mu * cf / (s * dy) - y / dy
    return [int(i) for i in np.nonzero((dy == 0.0) & ((lb_dy >= 0.0) | (ub_dy <= 0.0)))[0]]


@pytest.mark.parametrize("name", sorted(D.SIZES))
def test_designed_directions_reset_where_they_say(name):
    B = 6
    its = D.family(name, KS.Class_iterate, B)
    dirs, ycands = D.designed_directions(its, KS.Class_point)
    m = its[0].ncon()
    cf = 0.01
    seen = set()
    for b, (it, d, yc) in enumerate(zip(its, dirs, ycands)):
        role = D.ROLES[b % len(D.ROLES)]
        seen.add(role)
        r = D.round_inputs(b, it, d, yc)
        want, skipped = D.reset_rows(role, m)
        assert _np_resets(r.s_cand, r.mu_cand, yc, d.y, cf) == want, (b, role)
        assert all(d.y[i] == 0.0 and yc[i] > 0.0 for i in skipped)
        nx = np.max(np.abs(d.x))
        assert (nx < 1.0) == (b % 2 == 0)
        if role == "nan_ds":
            assert np.isnan(d.s).sum() == 1 and np.all(np.isfinite(d.y))
            continue                                        # s_cand holds the NaN: the oracle's loop asserts s > 0
        lb, ub = LO.dual_bounds(r.s_cand, r.mu_cand, yc, d.y, cf)
        if want:
            last = want[-1]
            assert ub <= -1.0, (b, role, ub)                 # behind a reset the interval starts at (0, -1)
            # only what follows the last reset counts
            tail = slice(last + 1, m)
            lb_t, ub_t = LO.dual_bounds(r.s_cand[tail], r.mu_cand, yc[tail], d.y[tail], cf)
            assert lb == max(lb_t, 0.0) and ub == min(ub_t, -1.0)
            if role == "reset_last":
                assert last == m - 1 and (lb, ub) == (0.0, -1.0) and math.copysign(1.0, d.y[m - 1]) < 0
        elif role == "nonfinite":
            assert (lb, ub) == (0.0, -1.0)
            ok = np.isfinite(yc)
            lb_f, ub_f = LO.dual_bounds(r.s_cand[ok], r.mu_cand, yc[ok], d.y[ok], cf)
            assert (lb_f, ub_f) != (0.0, -1.0)               # without the row the interval is an ordinary one: the fallback made (0, -1)
        else:
            assert not np.any(d.y == 0.0)
    assert seen == set(D.ROLES)
