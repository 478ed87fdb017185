"""Host-side tests of the scenario batches: the symbols and the struct, okkt_schur_batch_query -- which plans
take a scenario batch, why the others do not, what an item costs and how many launches a batch is -- on handles without a device, the
answer okkt_batch_query keeps giving for them, and the refusals that need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import schur_batch_designs as sbd  # noqa: E402
import schur_trees as sct  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["okkt_schur_batch_query", "okkt_schur_batch_reserve", "okkt_schur_batch_release", "okkt_factor_schur_batch", "okkt_factor_schur_batch_dev",
       "okkt_schur_batch_get", "okkt_schur_batch_get_dev", "okkt_schur_batch_factor", "okkt_schur_batch_factor_dev", "okkt_schur_batch_condense",
       "okkt_schur_batch_condense_dev", "okkt_schur_batch_expand", "okkt_schur_batch_expand_dev", "okkt_schur_batch_solve", "okkt_schur_batch_solve_dev",
       "okkt_schur_batch_select"]
REASONS = ("OK", "NOT_ANALYZED", "PARTITIONED", "NO_SET", "BIG_FRONTS", "SET_TOO_LARGE")


def err(h):
    return h._lib.okkt_last_error(h._h).decode()


def host_design(roots, set_it=True, **opts):
    """a host-only handle on a designed forest, its last root held back as the Schur set"""
    d = ft.build(roots)
    h = linear_solver_HIP("symmetric", host_symbolic_only=1, ordering=2, **dict(ft.NO_RELAX, **opts))
    initialize_b(h)
    if set_it:
        h.set_schur(sct.set_index(d))
    h.set_perm(d.perm)
    h.analyze(d.A)
    return h, d


def test_symbols_signatures_and_struct():
    lib = L.load()
    txt = open(os.path.join(ROOT, "include", "okkt.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name + " is not declared in include/okkt.h"
        assert name in L.SIGNATURES and name not in L.MISSING, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # two int32, four int64, four int32: no padding
    assert C.sizeof(L.OkktSchurBatchInfo) == 2 * 4 + 4 * 8 + 4 * 4
    m = re.search(r"typedef struct \{([^}]*)\} okkt_schur_batch_info;", txt)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == [f for f, _ in L.OkktSchurBatchInfo._fields_]
    for code, name in enumerate(REASONS):
        assert int(re.search(r"#define OKKT_SBATCH_" + name + r" (\d+)", txt).group(1)) == getattr(L, "OKKT_SBATCH_" + name) == code
    # the group size of the sums is a constant of the interface
    assert int(re.search(r"#define OKKT_SBATCH_GROUP (\d+)", txt).group(1)) == L.OKKT_SBATCH_GROUP == sbd.GROUP == 32
    # the size of okkt_batch_info has not moved
    assert C.sizeof(L.OkktBatchInfo) == 2 * 4 + 2 * 8 + 6 * 4


@pytest.mark.parametrize("name", sorted(sbd.DESIGNS))
def test_designs_are_eligible(name):
    sc = sbd.scenario(name)
    h = sc.handle(host=True)
    st = h.stats()
    d = sc.d
    # the analysis reproduces the design: the interior fronts are the designed ones, the set is the last front
    assert st["nsuper"] == len(d.nodes) and st["n"] == d.n
    interior = [nd["f"] for nd in d.nodes[:-1]]
    q = h.schur_batch_query(nrhs_max=1)
    assert (q["eligible"], q["reason"], q["ns"]) == (1, L.OKKT_SBATCH_OK, sc.ns), q
    assert q["max_front"] == max(interior) <= 136
    # an item holds the arena (on a handle without a device plan the dense bound that okkt_stats reports) and more
    assert q["bytes_per_item"] >= st["arena_bytes"] + 2 * 8 * st["n"] + 8 * sc.ns
    # shared: at least the sum and the dense factor's matrix
    assert q["bytes_shared"] >= 2 * 8 * sc.ns * sc.ns
    # the launch counts follow the interior's levels: the Schur front is in none
    assert 1 <= q["tasks_per_item"] <= len(interior)
    assert 1 <= q["levels"] <= max(nd["level"] for nd in d.nodes[:-1]) + 1 and q["levels"] <= q["tasks_per_item"]
    assert q["launches_factor"] == q["levels"] + 2
    assert q["launches_solve"] == 2 * q["levels"] + 6
    q4 = h.schur_batch_query(nrhs_max=4)
    assert q4["bytes_per_item"] > q["bytes_per_item"] and q4["bytes_shared"] == q["bytes_shared"]
    # the uniform batches keep their answer for such a handle
    qb = h.batch_query()
    assert (qb["eligible"], qb["reason"]) == (0, L.OKKT_BATCH_SCHUR)


def test_levels_of_designed_interiors():
    """leaves only under the set -> one level; the three-level interior keeps its three levels (the separators' subtrees are too large
    to be one task) with the chain of small fronts as one more task of the lowest level"""
    h, _ = host_design([ft.N(4, 0, ft.N(5, 1), ft.N(33, 2), ft.N(7, 3))])
    q = h.schur_batch_query()
    assert (q["eligible"], q["levels"], q["tasks_per_item"]) == (1, 1, 3)
    assert q["launches_factor"] == 3 and q["launches_solve"] == 8
    q = sbd.scenario("three-levels-chain").handle(host=True).schur_batch_query()
    assert (q["eligible"], q["levels"]) == (1, 3)
    assert q["tasks_per_item"] == 64 + 1
    # a childless set beside interior roots: the roots are the tasks
    q = sbd.scenario("childless-set").handle(host=True).schur_batch_query()
    assert (q["eligible"], q["max_front"]) == (1, 40)


def test_ineligible_plans_each_with_their_reason():
    # not analysed (also: a set given after the analysis)
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    q = h.schur_batch_query()
    assert (q["eligible"], q["reason"]) == (0, L.OKKT_SBATCH_NOT_ANALYZED)
    K = synth.augmented_matrix(synth.make_config("S-tiny", seed=3), delta=0.0)
    h.analyze(K)
    h.set_schur([0, 1, 2])
    assert h.schur_batch_query()["reason"] == L.OKKT_SBATCH_NOT_ANALYZED
    # no set
    h2, _ = host_design([ft.N(4, 0, ft.N(5, 1))], set_it=False)
    q = h2.schur_batch_query()
    assert (q["eligible"], q["reason"], q["bytes_per_item"]) == (0, L.OKKT_SBATCH_NO_SET, 0)
    assert h2.batch_query()["eligible"] == 1
    # partitioned (the reason comes before the missing set's)
    hp = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(hp)
    hp.analyze(K)
    assert hp._lib.okkt_dist_set_partition(hp._h, 2, 0) == L.OKKT_OK
    hp.analyze(K)
    q = hp.schur_batch_query()
    assert (q["eligible"], q["reason"]) == (0, L.OKKT_SBATCH_PARTITIONED)
    assert hp.batch_query()["reason"] == L.OKKT_BATCH_PARTITIONED
    # the set of three on S-tiny, analysed: taken
    h.analyze(K)
    q = h.schur_batch_query()
    assert (q["eligible"], q["ns"]) == (1, 3)
    assert h.batch_query()["reason"] == L.OKKT_BATCH_SCHUR
    # an interior front of 137 rows under small_front_max = 136, beside one of 136 that is taken; the set itself is under no bound
    for f, want in ((136, (1, L.OKKT_SBATCH_OK)), (137, (0, L.OKKT_SBATCH_BIG_FRONTS))):
        hh, _ = host_design([ft.N(200, 0, ft.N(f - 63, 63), ft.N(10, 5))], small_front_max=136)
        q = hh.schur_batch_query()
        assert (q["eligible"], q["reason"]) == want and q["max_front"] == f and q["ns"] == 200, q
        assert hh.batch_query()["reason"] == L.OKKT_BATCH_SCHUR
    # under the default small_front_max = 128 an interior front of 129 rows is a big front already
    hh, _ = host_design([ft.N(20, 0, ft.N(120, 9))])
    assert hh.schur_batch_query()["reason"] == L.OKKT_SBATCH_BIG_FRONTS
    # ns = 2049: a reason of its own (2048 is taken: the designs of the device tests hold one); big fronts come first where both apply
    hh, _ = host_design([ft.N(2049, 0, ft.N(5, 1))])
    q = hh.schur_batch_query()
    assert (q["eligible"], q["reason"], q["ns"], q["bytes_shared"]) == (0, L.OKKT_SBATCH_SET_TOO_LARGE, 2049, 0), q
    assert hh.batch_query()["reason"] == L.OKKT_BATCH_SCHUR
    hh, _ = host_design([ft.N(2049, 0, ft.N(200, 1))])
    assert hh.schur_batch_query()["reason"] == L.OKKT_SBATCH_BIG_FRONTS


def test_refusals_without_a_device():
    lib = L.load()
    sc = sbd.scenario("set-2-leaf")
    h = sc.handle(host=True)
    n, ns = sc.dim, sc.ns
    info = L.OkktSchurBatchInfo()
    assert lib.okkt_schur_batch_query(None, 1, C.byref(info)) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_query(h._h, 1, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_query(h._h, 0, C.byref(info)) == L.OKKT_ERR_INVALID and "nrhs_max" in err(h)
    # bad arguments before the device is asked for; then there is none
    for B in (0, -1, 65536):
        assert lib.okkt_schur_batch_reserve(h._h, B, 1) == L.OKKT_ERR_INVALID and "B outside" in err(h)
    assert lib.okkt_schur_batch_reserve(h._h, 4, 0) == L.OKKT_ERR_INVALID and "nrhs_max" in err(h)
    assert lib.okkt_schur_batch_reserve(None, 4, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_reserve(h._h, 4, 1) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_release(None) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_release(h._h) == L.OKKT_OK          # nothing reserved: nothing to do
    x = np.zeros(4 * n)
    r = np.zeros(4 * ns)
    S = np.zeros(ns * ns)
    v = np.zeros(4 * len(sc.rowval))
    inert = (L.OkktInertia * 4)()
    flags = (C.c_int32 * 4)()
    P = L.p_f64
    kind = L.OKKT_SYM_SYMMETRIC
    assert lib.okkt_factor_schur_batch(h._h, 4, None, 0, None, 0, sc.n1pos, sc.n1neg, kind, inert, flags) == L.OKKT_ERR_INVALID
    assert lib.okkt_factor_schur_batch(None, 4, P(v), 0, None, 0, sc.n1pos, sc.n1neg, kind, inert, flags) == L.OKKT_ERR_INVALID
    assert lib.okkt_factor_schur_batch(h._h, 4, P(v), 0, None, 0, sc.n1pos, sc.n1neg, kind, inert, flags) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_factor_schur_batch_dev(h._h, 4, None, 0, None, 0, sc.n1pos, sc.n1neg, kind, inert, flags) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_get(h._h, 0, None, ns) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_get(h._h, 0, P(S), ns) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_get_dev(h._h, -1, None, ns) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_factor(None, None, ns, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_factor(h._h, None, ns, None, None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_factor_dev(h._h, None, ns, None, None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_condense(h._h, 4, None, P(r), None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_condense(h._h, 4, P(x), None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_condense(h._h, 4, P(x), P(r), None, 1) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_condense_dev(h._h, 4, None, None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_expand(h._h, 4, P(x), None, P(x), 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_expand(h._h, 4, P(x), P(r), P(x), 1) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_expand_dev(h._h, 4, None, None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_solve(h._h, 4, None, None, P(x), 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_solve(h._h, 4, P(x), None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_solve(h._h, 4, P(x), None, P(x), 1) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_schur_batch_solve_dev(h._h, 4, None, None, None, 1) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_select(None, 0) == L.OKKT_ERR_INVALID
    assert lib.okkt_schur_batch_select(h._h, 0) == L.OKKT_ERR_NO_DEVICE
    # the handle is as usable as before
    assert h.schur_batch_query()["eligible"] == 1
