"""GPU tests: pivot classification and counting, the host's early check and the device stop flag of a retry ("Early exit
in the delta loop") on designed fronts (inertia_designs.py).  Every expected count is the simplicial oracle's or the design's own.

In-process, per design (handles of hip_solver(): NO_RELAX, the design's permutation):
  (a) counting: tolerances inside the spectrum of |D| (three quantiles, each in a gap >= 1e-6 wide where the HIP D is within 1e-10
      of the oracle's), pivots exactly on +-inertia_tol and one ulp outside it, pivots that are 0, NaN and +inf -- the 4-tuple is the
      reference's, and a tolerance changes no bit of D or L;
  (b) without early_exit a wrong request after a failed one still runs to the end: complete counts and a factor to solve with.

In a subprocess per route variant (inertia_case.py): first the counts at the 25 % tolerance and on the boundary matrices under that
route (early_exit = 0), then early_exit = 1, one handle per design, no solve in between:
  1. decided_low, a first attempt (host check only): flag 0; the counts are those of every front below some level l >= 1, or complete;
     where the documented rule names a level, of exactly that level, and pivots are left out; okkt_solve is refused;
  2. decided_low again (device flag on): flag 0, counts <= the true ones, no zero, they prove the failure themselves, and nothing
     above the level that decides is counted;
  3. the right request at the 25 % tolerance on a second handle, as a retry: a zero raises the stop;
  4. the right request as a retry (limits met exactly): flag 1, exact counts, D, L and five solutions bitwise those of a fresh
     early_exit = 0 handle;  5. again as a first attempt: the same bits;
  6. (npos - 1, nneg + 1), decided by the very last pivots, first and as a retry: flag 0 and complete counts or pos > npos - 1; then
     the right request with the bits of 4.
On the small-class, task-chain and small-only designs the scheduled units are not the designed levels: 1 asserts counts <= the true
ones, no zero, and neg > m_req there.  One INERTIA line per design and variant records what the stops actually skipped."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import inertia_designs as idn  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402
from test_gpu_front_shapes import VARIANTS as SHAPE_VARIANTS, hip_solver, parse_routes, route_of, solve_batch  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["default", "DATAFLOW=0", "TASKS=0", "FOLD_LONE=0", "RELEASE_CB=0", "DEBUG_POISON=1", "panel_nb=64,small_front_max=32"]
TOL_X = 1e-10      # a solve against the oracle's fp64 solve ("plain" values: both are within 1e-11 of the true solution)


def factor(h, A, n, m):
    return h.ls_factor_b(A, n, m), tuple(h.inertia)


@pytest.mark.parametrize("name", idn.ALL)
def test_counts_against_the_oracle(name):
    """(a): three tolerances inside the spectrum, the four boundary matrices at inertia_tol = 0.5, the isolated 0 / NaN / inf roots."""
    r = idn.reference(name)
    d = r.design
    right = (d.npos, d.nneg)
    h = hip_solver()
    h.set_perm(d.perm)
    assert factor(h, d.A, *right) == (1, (d.npos, d.nneg, 0, 0))
    D0, L0 = h.diag(), h.factor_csc()
    finalize_b(h)
    for tol, gap, want in idn.quantile_tols(name):
        h = hip_solver(inertia_tol=tol)
        h.set_perm(d.perm)
        flag, got = factor(h, d.A, *right)
        print(f"INERTIA {json.dumps(dict(name=name, tol=tol, gap=gap, got=got, want=want))}")
        assert flag == 0 and got == want, (tol, got, want)
        Lh = h.factor_csc()
        assert np.array_equal(h.diag(), D0) and np.array_equal(Lh.data, L0.data) and np.array_equal(Lh.indices, L0.indices)
        finalize_b(h)
    h = hip_solver(inertia_tol=idn.T_BOUNDARY)
    h.set_perm(d.perm)
    for kind, (A, want) in idn.boundary_matrices(name).items():
        flag, got = factor(h, A, *right)
        print(f"INERTIA {json.dumps(dict(name=name, boundary=kind, got=got, want=want))}")
        assert got == want, (kind, got, want)
        assert flag == int(want == (d.npos, d.nneg, 0, 0))
    finalize_b(h)
    A, perm, whole, want = idn.isolated(name)
    h = hip_solver()
    h.set_perm(perm)
    flag, got = factor(h, A, d.npos + 2, d.nneg + 1)
    assert flag == 0 and got == want, (got, want)
    assert np.array_equal(h.diag()[:d.n], D0)
    finalize_b(h)


@pytest.mark.parametrize("name", idn.ALL)
def test_complete_counts_by_default(name):
    """(b): early_exit = 0.  A wrong request that level 0 decides, twice (the second after a failed one): flag 0, exactly
    (npos, nneg, 0, 0), D and L bitwise those of the right request, and the factor solves (take_step2! after a failed flag)."""
    r = idn.reference(name)
    d = r.design
    low = idn.decided_low(name)
    B = ft.rhs(d.n, 5)
    h = hip_solver(early_exit=0)
    h.set_perm(d.perm)
    assert factor(h, d.A, d.npos, d.nneg) == (1, (d.npos, d.nneg, 0, 0))
    D0, L0, X0 = h.diag(), h.factor_csc().data, solve_batch(h, B)
    for _ in range(2):
        assert factor(h, d.A, *low) == (0, (d.npos, d.nneg, 0, 0))
        assert np.array_equal(h.diag(), D0) and np.array_equal(h.factor_csc().data, L0)
        X = solve_batch(h, B)
        assert np.array_equal(X, X0)
    finalize_b(h)
    for x, b in zip(X0, B):
        assert ft.fwd_err(x, r.oracle.ls_solve(b)) <= TOL_X


# ---- the early exit under every route (subprocesses) -----------------------------------------------------------------------------
_RUNS = {}


def run_case(variant, mode, names, debug=False):
    """(record, arrays of step 4) of one subprocess; with debug also its stderr (the OKKT_DEBUG_FRONTS lines)"""
    key = (variant, mode, tuple(names), debug)
    if key not in _RUNS:
        env, opts = SHAPE_VARIANTS[variant]
        e = dict(os.environ)
        e.update(env)
        if debug:
            e["OKKT_DEBUG_FRONTS"] = "1"
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "case.npz")
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "inertia_case.py"), out, json.dumps(opts), mode, *names],
                               cwd=ROOT, env=e, capture_output=True, text=True, timeout=240)
            assert p.returncode == 0 and "CASE_OK" in p.stdout, (variant, mode, p.stdout[-400:], p.stderr[-1500:])
            with np.load(out) as z:
                res = {k: z[k] for k in z.files}
        _RUNS[key] = (json.loads(str(res.pop("record"))), res, p.stderr)
    return _RUNS[key][:2] + ((_RUNS[key][2],) if debug else ())


def le(a, b):
    return all(x <= y for x, y in zip(a, b))


def check_steps(name, q):
    """the record of one design (inertia_case.py, "steps") against the reference; returns what the INERTIA line reports"""
    r = idn.reference(name)
    d = r.design
    n_low, m_low = idn.decided_low(name)
    pre = idn.level_prefix_counts(name)
    true = (d.npos, d.nneg, 0, 0)
    ok = [1, d.npos, d.nneg, 0, 0]
    assert q["fresh"] == ok
    # counting under this route (complete counts): the 25 % tolerance changes no bit of the factor, the boundary pivots
    assert q["tol25"] == [0] + list(idn.quantile_tols(name)[1][2]) and q["tol25_same_as_fresh"], q["tol25"]
    for kind, (_, want) in idn.boundary_matrices(name).items():
        assert q["boundary"][kind][1:] == list(want), (kind, q["boundary"][kind], want)
    # 1. first attempt: the host's check
    flag, *c1 = q["s1"]
    assert flag == 0 and c1[2:] == [0, 0], q["s1"]
    stopped = [l for l in range(1, len(pre)) if tuple(c1[:2]) == pre[l]]
    at = None if not stopped else ("complete" if stopped[-1] == len(pre) - 1 else stopped[-1])
    lv = idn.documented_early_level(name)
    if name in idn.UNITS_DIFFER:
        assert le(c1, true) and c1[1] > m_low, (q["s1"], m_low)
    else:
        assert stopped, (q["s1"], pre)
        if lv is not None:
            assert tuple(c1[:2]) == pre[lv] and sum(c1) < d.n, (q["s1"], lv, pre)
    if at == "complete":
        assert q["s1_solve"] == "solved"
    else:
        assert q["s1_solve"].startswith("refused"), q["s1_solve"]
    # 2. the same request as a retry: the device flag
    flag, *c2 = q["s2"]
    assert flag == 0 and le(c2, true) and c2[2:] == [0, 0], q["s2"]
    assert c2[1] > m_low or c2[0] > n_low, (q["s2"], n_low, m_low)
    # ... and the stop comes no later than the level that decides.  Level 0 holds m_low + 1 negative pivots.  Within a level the small
    # fronts run first, k_fold_counts then adds their slots to the slot the big fronts count in, so whichever kernel of level 0 adds
    # last sees the true total and raises the flag; the kernels of level 1 are launched behind it and return at once: nothing above
    # level 0 is counted.  (Task chains span levels: there everything below the big root is counted before the root's level at the
    # latest, and the root must not run.  The small-class design's root may share a task with a child: no such bound.)
    if name not in idn.UNITS_DIFFER:
        assert le(c2[:2], pre[1]), (q["s2"], pre[1])
    elif name == "task-chains-under-big":
        assert le(c2[:2], pre[-2]), (q["s2"], pre[-2])
    # 3. a zero raises the stop
    want3 = idn.quantile_tols(name)[1][2]
    assert q["s3_before"][0] == 0
    flag, *c3 = q["s3"]
    assert flag == 0 and c3[2] >= 1 and le(c3, want3), (q["s3"], want3)
    # 4. - 6.
    assert q["s4"] == ok and q["s4_same_as_fresh"], q["s4"]
    assert q["s5"] == ok and q["s5_same_as_s4"], q["s5"]
    for key in ("s6_first", "s6"):
        flag, *c6 = q[key]
        assert flag == 0 and le(c6, true) and c6[2:] == [0, 0], (key, q[key])
        assert tuple(c6) == true or c6[0] > d.npos - 1, (key, q[key])
    assert q["s6_right"] == ok and q["s6_right_same_as_s4"], q["s6_right"]
    return dict(name=name, route=route_of(d), s1_level=at, early_level=lv, s1=c1, s2=c2, s3=c3, s6=q["s6"][1:])


@pytest.mark.parametrize("variant", VARIANTS)
def test_early_exit_under_route_switches(variant):
    """Steps 1 to 6 of the module docstring on every design under one route variant.  Without the dataflow launch and without
    released CBs the bits of step 4 are those of the default run."""
    rec, res = run_case(variant, "steps", idn.ALL)
    failures = []
    for name in idn.ALL:
        print(f"INERTIA_RAW {json.dumps(dict(name=name, variant=variant, **rec[name]))}")
    for name in idn.ALL:
        try:
            line = check_steps(name, rec[name])
            print(f"INERTIA {json.dumps(dict(variant=variant, **line))}")
        except AssertionError as e:      # every design is checked and printed before the test fails
            failures.append((name, str(e)[:600]))
    assert not failures, failures
    assert set(res) == {f"{name}/{k}" for name in idn.ALL for k in ("D", "Lx", "X")}
    if variant in ("DATAFLOW=0", "RELEASE_CB=0"):
        _, base = run_case("default", "steps", idn.ALL)
        assert set(base) == set(res)
        for k in base:
            assert np.array_equal(res[k], base[k]), k


def test_the_small_only_design_is_one_launch_of_tasks():
    """OKKT_DEBUG_FRONTS on flow-small-only: no level holds a big front and the tasks form at least two levels -- the schedule under
    which all of them run as one launch whose tasks hand over through flags and an epoch -- and steps 1 to 6 hold there as well."""
    name = "flow-small-only"
    rec, _, err = run_case("default", "steps", [name], debug=True)
    classes = parse_routes(err)[name][2]
    print(f"INERTIA {json.dumps(dict(name=name, classes=classes))}")
    assert len(classes) >= 2 and all(c[3] == 0 for c in classes.values()), classes
    check_steps(name, rec[name])


def test_definite_kind_counts_a_negative_boundary_pivot():
    """sym_kind definite on an all-positive copy of mixed-level, early_exit = 1: -t on the first pivot of one leaf is a negative pivot
    (the tolerance of the definite kind is 0 whatever inertia_tol says) -- the oracle's counts at tolerance 0, flag 0; then the clean
    matrix as a retry whose limits (n, 0) are met exactly: flag 1."""
    name = "mixed-level"
    rec, _ = run_case("default", "definite", [name])
    q = rec[name]
    d = idn.reference(name).design
    Apos = idn.set_diagonal(d.A, np.arange(d.n), 0.0)
    Apos.data[Apos.indptr[:-1]] = np.abs(d.A.diagonal())
    Aneg = idn.set_diagonal(Apos, d.perm[idn.leaf_first_pivots(d)[:1]], -idn.T_BOUNDARY)
    o = idn._factor(Aneg, d.perm, d.n, 0)
    assert o.inertia(0.0) == (d.n - 1, 1, 0, 0)
    assert idn._factor(Apos, d.perm, d.n, 0).inertia(0.0) == (d.n, 0, 0, 0)
    print(f"INERTIA {json.dumps(dict(name=name, kind='definite', **q))}")
    assert q["neg_pivot"] == [0, d.n - 1, 1, 0, 0]
    assert q["clean"] == [1, d.n, 0, 0, 0] and q["clean_solve_finite"]


def test_schur_mode_never_stops_early():
    """mixed-level with its last root as the Schur set, early_exit = 1: a wrong request that level 0 decides, twice (the second is a
    retry), then the right one.  Early exit is off in Schur mode: every time the complete, exact counts of A11 (the oracle's D)."""
    name = "mixed-level"
    rec, _ = run_case("default", "schur", [name])
    q = rec[name]
    r = idn.reference(name)
    n1 = r.design.n - r.design.nodes[-1]["k"]
    want = [int(np.sum(r.D[:n1] > 0)), int(np.sum(r.D[:n1] < 0))]
    print(f"INERTIA {json.dumps(dict(name=name, kind='schur', **q))}")
    assert q["want"] == want and sum(want) == n1
    assert q["low_first"] == [0] + want + [0, 0]
    assert q["low_retry"] == [0] + want + [0, 0]
    assert q["right_retry"] == [1] + want + [0, 0]
