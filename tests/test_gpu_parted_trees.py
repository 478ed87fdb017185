"""GPU tests: the partitioned (subtree-sharded) factor and solve -- okkt_dist_set_partition and the okkt_dist_* phases, the parted
branches of the numeric set-up, k_pack_cb, k_pack_cv, k_exchange_x and the top schedule -- on the designed cuts of parted_trees.py.
test_gpu_sharded.py takes whatever cut the ordering gives two synthetic problems and compares one solution with the unsharded
handle; here the cut is chosen (no top, a wide top, a top of two levels, a top of small fronts; boundary fronts of every class;
empty parts; parts that are tasks of small fronts; a wide front inside part 0 and inside a part > 0) and checked before any GPU time
is spent (test_parted_trees.py), and every case is compared with the simplicial oracle on the same permutation: the pivot counts,
the factor composed from the parts (column j from the part that owns it, the top from part 0), the solutions against the solution of
the fp64 matrix refined in long double, and every rank's buffer in front of every exchange (RecordingComm).

All virtual ranks live in one process (LocalComm).  The tolerances are those of test_gpu_front_shapes.py for the same front classes.
The route switches (read once per process) run in subprocesses (parted_trees_case.py)."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import parted_trees as pt  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402
from test_gpu_front_shapes import TOL_D, TOL_L, TOL_X, check_factor, hip_solver  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_UNPARTED = {}


def unparted_error(name):
    """forward error of an unpartitioned handle on the same design and permutation (printed beside the partitioned one)"""
    if name not in _UNPARTED:
        r = pt.reference(name)
        h = hip_solver()
        h.set_perm(r.d.perm)
        assert h.ls_factor_b(r.d.A, r.d.npos, r.d.nneg) == 1
        _UNPARTED[name] = max(ft.fwd_err(h.ls_solve(b), xt) for b, xt in zip(r.B, r.XT))
        finalize_b(h)
    return _UNPARTED[name]


def cb_error(r, i, slot):
    """The owner's slot of boundary front i against the update matrix of the oracle's factor, U = -(L_cb D) L_cb^T over the pivot
    columns of the front's subtree, L_cb the CB rows of those columns.  With |dL| <= TOL_L max|L| and |dD| <= TOL_D |D|, what the
    factor itself is held to, an entry of U (a sum of nsub products l d l) is off by at most
    nsub max|D| max|L_cb| (2 TOL_L max|L| + TOL_D max|L_cb|); the rounding of the sum itself is far below that.
    Returns the error relative to max|U|."""
    nd = r.d.nodes[i]
    c0, c1 = pt.subtree_cols(r.d, i)
    Lcb = r.L[nd["rows"][nd["k"]:]][:, c0:c1].toarray()
    Dsub = r.D[c0:c1]
    U = -(Lcb * Dsub) @ Lcb.T
    err = float(np.max(np.abs(np.triu(slot - U))))          # slot[j, i] with i >= j: on and above the diagonal of the array
    lcb = float(np.max(np.abs(Lcb)))
    bound = (c1 - c0) * float(np.max(np.abs(Dsub))) * lcb * (2.0 * TOL_L * float(abs(r.L).max()) + TOL_D * lcb)
    assert err <= bound, ("cb against the oracle's update matrix", i, err, bound)
    return err / float(np.max(np.abs(U)))


def check_exchanges(r, nparts, res):
    """What every rank held in front of each exchange (step 5 of the module's checks)."""
    d = r.d
    owners = pt.DESIGNS[r.name]["cuts"][nparts]
    sl, ncb, ncv = pt.slots(d, owners)
    co = pt.col_owner(d, owners)
    top_cols = np.flatnonzero(co == -1)
    cb = res["cb"]
    assert cb.shape == (nparts, max(ncb, 1))
    e_cb = 0.0
    # cb reduce: a slot is written by its owner alone, and only on and below the diagonal (column-major, j * r + i)
    for i, rr, ocb, _ in sl:
        for p in range(nparts):
            slot = cb[p, ocb:ocb + rr * rr].reshape(rr, rr)        # slot[j, i]
            if p != owners[i]:
                assert not slot.any(), ("cb", i, p)
            else:
                assert not np.tril(slot, -1).any(), ("cb above the diagonal", i, p)
                assert np.isfinite(slot).all() and slot.any(), ("cb", i, p)
                e_cb = max(e_cb, cb_error(r, i, slot))
    masks = np.array([(co == p) | ((co == -1) & (p == 0)) for p in range(nparts)])
    support = np.zeros((nparts, d.n), dtype=bool)
    for p in range(nparts):
        support[p, d.perm[masks[p]]] = True
    assert np.array_equal(support.sum(axis=0), np.ones(d.n, dtype=np.int64))      # disjoint, and they cover 0 .. n - 1
    for q, xt in enumerate(r.XT):
        cv, x, sol = res[f"cv/{q}"], res[f"x/{q}"], res[f"sol/{q}"]
        assert cv.shape == (nparts, max(ncv, 1)) and x.shape == sol.shape == (nparts, d.n)
        for i, rr, _, ocv in sl:
            for p in range(nparts):
                slot = cv[p, ocv:ocv + rr]
                if p != owners[i]:
                    assert not slot.any(), ("cv", i, p)
                else:
                    assert np.isfinite(slot).all() and slot.any(), ("cv", i, p)
        # x broadcast: the source holds the solution on the top's columns, packed
        xtop = x[0, :len(top_cols)]
        assert np.max(np.abs(xtop - xt[d.perm[top_cols]]), initial=0.0) <= TOL_X * np.max(np.abs(xt)), ("x", q)
        # sol reduce: every rank its own columns (the top counts for rank 0), exact zeros elsewhere
        for p in range(nparts):
            assert not sol[p, ~support[p]].any(), ("sol", q, p)
            assert np.isfinite(sol[p]).all() and np.all(sol[p, support[p]] != 0.0), ("sol", q, p)
        assert np.array_equal(sol.sum(axis=0), res["X"][q])
        if len(top_cols) == 0:
            # no top: nothing is packed, the buffers stay as they were allocated
            assert cb.shape[1] == cv.shape[1] == 1 and not cb.any() and not cv.any() and not x.any()
    return e_cb


def check_results(r, nparts, res, variant):
    """Steps 2 - 5: the flag and the pivot counts, the composed factor, the solutions (the repeated ones bitwise equal), the
    exchange buffers.  Prints the PARTTREE line and returns its figures."""
    d = r.d
    fig = dict(name=r.name, nparts=nparts, variant=variant)
    assert int(res["flag"]) == 1 and tuple(res["inertia"]) == (d.npos, d.nneg, 0, 0), (res["flag"], res["inertia"])
    Lh = sp.csc_matrix((res["Lx"], res["Li"], res["Lp"]), shape=(d.n, d.n))
    errs = [ft.fwd_err(x, xt) for x, xt in zip(res["X"], r.XT)]
    e_d, e_l = check_factor(d, r.o, res["inertia"], res["D"], Lh, tol_d=np.inf, tol_l=np.inf)
    fig.update(e_d=e_d, e_l=e_l, err=max(errs), e_oracle=r.e_oracle, e_unparted=unparted_error(r.name))
    print(f"PARTTREE {json.dumps(fig)}")
    assert e_d <= TOL_D and e_l <= TOL_L, (e_d, e_l)
    assert max(errs) <= TOL_X, errs
    assert np.array_equal(res["X"], res["X_again"])
    fig["e_cb"] = check_exchanges(r, nparts, res)
    print(f"PARTTREE-CB {json.dumps(dict(name=r.name, nparts=nparts, variant=variant, e_cb=fig['e_cb']))}")
    return fig


def check_wrong(d, res, w):
    """Step 6: the wrong inertia is refused with the true counts, and the factorisation right behind it is the first one again."""
    assert int(w["wrong_flag"]) == 0 and tuple(w["wrong_inertia"]) == (d.npos, d.nneg, 0, 0), (w["wrong_flag"], w["wrong_inertia"])
    assert int(w["right_flag"]) == 1 and tuple(w["right_inertia"]) == (d.npos, d.nneg, 0, 0)
    assert np.array_equal(w["right_D"], res["D"]) and np.array_equal(w["right_Lx"], res["Lx"]) and np.array_equal(w["right_X"], res["X"])


@pytest.mark.parametrize("case", pt.CASES, ids=pt.case_id)
def test_partitioned_factor_and_solve_on_designed_cut(case):
    """One design at one number of parts, "plain" values: the cut is the catalogue's; flag and pivot counts; D and L composed from
    the parts against the oracle; two right-hand sides solved one at a time against the true solution, a repeated solve bitwise
    equal; every exchange buffer; a wrong inertia and the right one behind it; other values on the same solvers bit for bit those
    of fresh ones."""
    name, nparts = case
    want = pt.DESIGNS[name]
    r = pt.reference(name)
    d = r.d
    sh = pt.sharded(d, nparts)
    sn, col, _ = sh.owners()
    assert sn.tolist() == want["cuts"][nparts]
    assert (sh.info["n_boundary"], sh.info["cb_doubles"]) == (want["n_boundary"], want["cb_doubles"])
    assert sh.info["cv_doubles"] == pt.slots(d, want["cuts"][nparts])[2]
    for s in sh.solvers:
        assert np.array_equal(s.perm(), d.perm)
    res = pt.device_results(sh, d, r.B)
    check_results(r, nparts, res, "in-process")
    check_wrong(d, res, pt.wrong_then_right(sh, d, r.B))
    # refactorisation: other values, the same pattern, the same solvers -- against fresh ones
    d2 = pt.build(name, seed=1)
    assert np.array_equal(d2.A.indices, d.A.indices) and np.array_equal(d2.A.indptr, d.A.indptr)
    fresh = pt.sharded(d, nparts)
    one, two = pt.device_results(sh, d2, r.B), pt.device_results(fresh, d2, r.B)
    sh.finalize()
    fresh.finalize()
    assert int(one["flag"]) == 1 and tuple(one["inertia"]) == (d2.npos, d2.nneg, 0, 0)
    assert not np.array_equal(one["D"], res["D"])
    for k in ("flag", "inertia", "D", "Lx", "X", "X_again"):
        assert np.array_equal(one[k], two[k]), k


# ---- the route switches (subprocesses) --------------------------------------------------------------------------------------------
VARIANTS = {
    "default": ({}, {}),
    "DEBUG_POISON=1": ({"OKKT_DEBUG_POISON": "1"}, {}),
    "PARTED_TASKS=0": ({"OKKT_PARTED_TASKS": "0"}, {}),
    "DATAFLOW=0": ({"OKKT_DATAFLOW": "0"}, {}),
    "FLOW=0": ({"OKKT_FLOW": "0"}, {}),
    "early_exit=1": ({}, {"early_exit": 1}),
    "panel_nb=64,small_front_max=32": ({}, {"panel_nb": 64, "small_front_max": 32}),
}
WRONG = ("default", "early_exit=1")      # the variants that also run the wrong inertia
_RUNS = {}


def run_case(variant):
    if variant not in _RUNS:
        env, opts = VARIANTS[variant]
        e = dict(os.environ)
        e.update(env)
        args = (["wrong"] if variant in WRONG else []) + [pt.case_id(c) for c in pt.VARIANT_CASES]
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "case.npz")
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "parted_trees_case.py"), out, json.dumps(opts), *args],
                               cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0 and "CASE_OK" in p.stdout, (variant, p.stdout[-400:], p.stderr[-1500:])
            with np.load(out) as z:
                res = {k: z[k] for k in z.files}
        _RUNS[variant] = res
    return _RUNS[variant]


def of_case(res, case):
    key = pt.case_id(case) + "/"
    return {k[len(key):]: v for k, v in res.items() if k.startswith(key)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_designed_cuts_under_route_switches(variant):
    """The variant cases under every route switch: flag, pivot counts, composed factor, solutions and exchange buffers as in the
    in-process test.  The exact zeros of the buffers under the poison are what catches a NaN that a mask lets through.  A handle
    with early exit behaves like the default one (the partitioned path always runs to the end): the same wrong-inertia flag and
    counts, and bit for bit the default's factor and solutions."""
    t0 = time.perf_counter()
    res = run_case(variant)
    for case in pt.VARIANT_CASES:
        name, nparts = case
        one = of_case(res, case)
        r = pt.reference(name)
        want = pt.DESIGNS[name]
        assert np.array_equal(one["perm"], r.d.perm)
        assert (int(one["info/n_boundary"]), int(one["info/cb_doubles"])) == (want["n_boundary"], want["cb_doubles"])
        check_results(r, nparts, one, variant)
        if variant in WRONG:
            check_wrong(r.d, one, one)
        if variant == "early_exit=1":
            base = of_case(run_case("default"), case)
            for k in ("D", "Lx", "X", "wrong_flag", "wrong_inertia"):
                assert np.array_equal(one[k], base[k]), (case, k)
    print(f"PARTTREE-TIME {json.dumps(dict(variant=variant, seconds=round(time.perf_counter() - t0, 2)))}")
