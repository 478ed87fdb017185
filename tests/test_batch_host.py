"""Host-side tests of the uniform batches: the symbols and the struct, okkt_batch_query -- which plans take a
batch, why the others do not, what a slot costs and how many launches a batch is -- on handles without a device, and the refusals
that need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import lanczos_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["okkt_batch_query", "okkt_batch_reserve", "okkt_batch_release", "okkt_batch_set_mode", "okkt_batch_mode_used", "okkt_factor_batch",
       "okkt_factor_batch_dev", "okkt_solve_batch", "okkt_solve_batch_dev", "okkt_batch_select"]


def host_handle(A=None, perm=None, **opts):
    h = linear_solver_HIP("symmetric", host_symbolic_only=1, **opts)
    initialize_b(h)
    if perm is not None:
        h.set_perm(perm)
    if A is not None:
        h.analyze(A)
    return h


def err(h):
    return h._lib.okkt_last_error(h._h).decode()


def kkt(prob):
    return synth.augmented_matrix(prob, delta=0.0)


def design37():
    it = R.indefinite_design(KS.Class_iterate, 37, -3.7)
    return kkt(dict(H=sp.csc_matrix(it.H), J=sp.csc_matrix(it.J), s=it.s, y=it.y, n=it.dim(), m=it.ncon()))


IN_SCOPE = {
    "chain400": lambda: kkt(synth.hanging_chain(N_h=400)),
    "chain40": lambda: kkt(synth.hanging_chain(N_h=40)),
    "S-tiny": lambda: kkt(synth.make_config("S-tiny", seed=3)),
    "S-tiny-schur": lambda: synth.schur_matrix(synth.make_config("S-tiny", seed=3)),
    "infeasible-lp": lambda: kkt(synth.infeasible_lp(rows=60, cols=90)),
    "indefinite-37": design37,
}


def test_symbols_signatures_and_struct():
    lib = L.load()
    txt = open(os.path.join(ROOT, "include", "okkt.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name + " is not declared in include/okkt.h"
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # two int32, two int64, six int32: no padding
    assert C.sizeof(L.OkktBatchInfo) == 2 * 4 + 2 * 8 + 6 * 4
    m = re.search(r"typedef struct \{([^}]*)\} okkt_batch_info;", txt)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == [f for f, _ in L.OkktBatchInfo._fields_]
    for name in ("OK", "NOT_ANALYZED", "PARTITIONED", "SCHUR", "SCALING", "BIG_FRONTS"):
        assert int(re.search(r"#define OKKT_BATCH_" + name + r" (\d+)", txt).group(1)) == getattr(L, "OKKT_BATCH_" + name)


@pytest.mark.parametrize("name", sorted(IN_SCOPE))
def test_in_scope_plans_are_eligible(name):
    h = host_handle(IN_SCOPE[name]())
    st = h.stats()
    assert st["n_big_fronts"] == 0
    q = h.batch_query(nrhs_max=1)
    assert q["eligible"] == 1 and q["reason"] == L.OKKT_BATCH_OK
    assert q["max_front"] == st["max_front"] <= 136
    # a slot holds the arena and more; on a handle without a device plan the arena is the dense bound that okkt_stats reports
    assert q["bytes_per_item"] >= st["arena_bytes"] + 2 * 8 * st["n"]
    # tasks are whole subtrees of fronts: at most one per front, at most one level of tasks per level of fronts
    assert 1 <= q["tasks_per_item"] <= st["nsuper"]
    assert 1 <= q["levels"] <= st["nlevels"] and q["levels"] <= q["tasks_per_item"]
    # level mode: the shifts and counters, then one launch per level; per group of right-hand sides gather, up, down, scatter
    assert q["launches_factor_level"] == q["levels"] + 1
    assert q["launches_solve_level"] == 2 * q["levels"] + 2
    # item mode: one launch each, whatever the plan
    assert q["launches_factor_item"] == 1 and q["launches_solve_item"] == 1
    # more work columns cost more
    q4 = h.batch_query(nrhs_max=4)
    assert q4["bytes_per_item"] > q["bytes_per_item"]
    assert h.batch_query(nrhs_max=3)["bytes_per_item"] == q4["bytes_per_item"] == h.batch_query(nrhs_max=9)["bytes_per_item"]


def test_levels_of_designed_trees():
    """The launch counts follow the task tree: leaves only -> one level; a root over three separators over twenty leaves each -> three
    (neither the separators' subtrees nor the whole tree are small enough to be one task)."""
    d = ft.build([ft.N(5), ft.N(33), ft.N(7), ft.N(20)])
    h = host_handle(d.A, d.perm, ordering=2, **ft.NO_RELAX)
    q = h.batch_query()
    assert (q["eligible"], q["levels"], q["tasks_per_item"]) == (1, 1, 4)
    assert q["launches_factor_level"] == 2 and q["launches_solve_level"] == 4
    leaves = [ft.N(16 + (i % 2), 16) for i in range(20)]
    d = ft.build([ft.N(40, 0, *[ft.N(17, 16, *[ft.N(nd.k, nd.c) for nd in leaves]) for _ in range(3)])])
    h = host_handle(d.A, d.perm, ordering=2, **ft.NO_RELAX)
    assert h.stats()["nsuper"] == 64 and h.stats()["nlevels"] == 3
    q = h.batch_query()
    assert (q["eligible"], q["levels"], q["tasks_per_item"]) == (1, 3, 64)
    assert q["launches_factor_level"] == 4 and q["launches_solve_level"] == 8


def test_ineligible_plans_each_with_their_reason():
    # not analysed
    h = host_handle()
    q = h.batch_query()
    assert (q["eligible"], q["reason"]) == (0, L.OKKT_BATCH_NOT_ANALYZED)
    # big fronts: S-small; one front of 137 rows under small_front_max = 136 (136 rows are taken)
    h = host_handle(kkt(synth.make_config("S-small", seed=3)))
    assert h.stats()["n_big_fronts"] > 0
    q = h.batch_query()
    assert (q["eligible"], q["reason"], q["bytes_per_item"]) == (0, L.OKKT_BATCH_BIG_FRONTS, 0)
    for f, want in ((136, (1, L.OKKT_BATCH_OK)), (137, (0, L.OKKT_BATCH_BIG_FRONTS))):
        d = ft.build([ft.N(f)])
        h = host_handle(d.A, d.perm, ordering=2, small_front_max=136, **ft.NO_RELAX)
        q = h.batch_query()
        assert (q["eligible"], q["reason"]) == want and q["max_front"] == f
    # under the default small_front_max = 128 a front of 129 rows is a big front already
    d = ft.build([ft.N(129)])
    assert host_handle(d.A, d.perm, ordering=2, **ft.NO_RELAX).batch_query()["reason"] == L.OKKT_BATCH_BIG_FRONTS
    # a Schur set
    K = kkt(synth.make_config("S-tiny", seed=3))
    h = host_handle()
    h.set_schur([0, 1, 2])
    h.analyze(K)
    q = h.batch_query()
    assert (q["eligible"], q["reason"]) == (0, L.OKKT_BATCH_SCHUR)
    # a partitioned handle
    h = host_handle(K)
    assert h._lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    h.analyze(K)
    q = h.batch_query()
    assert (q["eligible"], q["reason"]) == (0, L.OKKT_BATCH_PARTITIONED)
    # a scaling
    h = host_handle(K)
    h.set_scaling("ruiz")
    q = h.batch_query()
    assert (q["eligible"], q["reason"]) == (0, L.OKKT_BATCH_SCALING)
    h.set_scaling("none")
    assert h.batch_query()["eligible"] == 1


def test_refusals_without_a_device():
    lib = L.load()
    K = kkt(synth.make_config("S-tiny", seed=3))
    h = host_handle(K)
    n = h.stats()["n"]
    info = L.OkktBatchInfo()
    assert lib.okkt_batch_query(None, 1, C.byref(info)) == L.OKKT_ERR_INVALID
    assert lib.okkt_batch_query(h._h, 1, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_batch_query(h._h, 0, C.byref(info)) == L.OKKT_ERR_INVALID and "nrhs_max" in err(h)
    # bad arguments before the device is asked for; then there is none
    for B in (0, -1, 65536):
        assert lib.okkt_batch_reserve(h._h, B, 1) == L.OKKT_ERR_INVALID and "B outside" in err(h)
    assert lib.okkt_batch_reserve(h._h, 4, 0) == L.OKKT_ERR_INVALID and "nrhs_max" in err(h)
    assert lib.okkt_batch_reserve(None, 4, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_batch_reserve(h._h, 4, 1) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_batch_release(h._h) == L.OKKT_OK          # nothing reserved: nothing to do
    assert lib.okkt_batch_set_mode(h._h, 3) == L.OKKT_ERR_INVALID
    assert lib.okkt_batch_set_mode(h._h, 2) == L.OKKT_OK and lib.okkt_batch_mode_used(h._h) == 0
    x = np.zeros(4 * n)
    inert = (L.OkktInertia * 4)()
    flags = (C.c_int32 * 4)()
    assert lib.okkt_factor_batch(h._h, 4, None, 0, None, 0, 40, 60, L.OKKT_SYM_SYMMETRIC, inert, flags) == L.OKKT_ERR_INVALID
    assert lib.okkt_factor_batch(h._h, 4, L.p_f64(x), 0, None, 0, 40, 60, L.OKKT_SYM_SYMMETRIC, inert, flags) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_factor_batch_dev(h._h, 4, None, 0, None, 0, 40, 60, L.OKKT_SYM_SYMMETRIC, inert, flags) == L.OKKT_ERR_INVALID
    assert lib.okkt_solve_batch(h._h, 4, None, L.p_f64(x), 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_solve_batch(h._h, 4, L.p_f64(x), L.p_f64(x), 1) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_solve_batch_dev(h._h, 4, None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_batch_select(None, 0) == L.OKKT_ERR_INVALID
    assert lib.okkt_batch_select(h._h, 0) == L.OKKT_ERR_NO_DEVICE
    # the handle is as usable as before
    assert h.batch_query()["eligible"] == 1
