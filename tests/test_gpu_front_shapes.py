"""GPU tests: every factor and solve route of the numeric phase on fronts whose shapes are designed (front_trees.py), against the
simplicial oracle on the same permutation.  The whole-tree tests (S-small, S-C3, S-C5, S-metric) take whatever front shapes the
ordering produces; here every pivot / CB edge, thin and tall front, small-front class, mixed level, forest, deep chain and fan-in
of the catalogue is made to happen on purpose, and each is checked for its shape, inertia, D, L and its solutions (against the
solution of the fp64 matrix refined in long double), for repeated solves and for a refactorisation on the same handle.
The other routes (schedule switches read once per process) run the same designs in subprocesses (front_shapes_case.py).
Here the counted inertia always equals the request; pivot counting at a tolerance and the early exit of the delta loop on these
designs are in test_gpu_inertia_designs.py."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from onephase_jl_amd import _lib as L
from onephase_jl_amd.linear_system_solvers import finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_D = 1e-10          # max relative error of D
TOL_L = 1e-10          # max |L_hip - L_oracle| / max |L_oracle|
TOL_X = 1e-11          # forward error, "plain" values
TOL_BATCH = 1e-13      # a column of a batch against its single solve
SMALL_MAX = 128        # the default small_front_max

# "ipm" values, designs whose pivot blocks of more than 384 columns are solved through explicit inverses of 1024-column blocks:
# forward error of the HIP solve / the oracle's (worst of two vectors each), measured on MI355X.  On these designs the explicit
# inverses are no worse than the oracle's substitution but on the forest (2.8 x: three roots of 500, 1100 and 1700 pivot columns)
# and on k = 385 / c = 1 (1.45 x: one padded 1024-column block of 385 columns); nowhere near the 5 - 40 x of DESIGN section 5.
IPM_INV_RATIO = {
    "edge-k129-c700": 0.14, "edge-k385-c1": 1.45, "edge-k1023-c128": 0.17, "edge-k1024-c63": 0.16, "edge-k1025-c1": 0.34,
    "edge-k2047-c0": 0.13, "edge-k2048-c127": 0.35, "edge-k2049-c129": 0.17, "thin-tall-k1-2-127-128-c2100": 0.37,
    "thin-k128-f2049": 0.64, "mixed-level": 0.22, "mixed-level-scatter": 0.52, "forest-3-roots": 2.80, "fan-in-8": 0.46,
}


def hip_solver(**o):
    h = linear_solver_HIP("symmetric", ordering=2, **dict(ft.NO_RELAX, **o))
    initialize_b(h)
    return h


def solve_batch(h, B):
    X = np.zeros_like(B)
    h._check(h._lib.okkt_solve(h._h, L.p_f64(np.ascontiguousarray(B)), L.p_f64(X), B.shape[0]), "okkt_solve")
    return X


_REF = {}


def reference(name, values="plain", seed=0):
    """(design, oracle factor, full matrix, right-hand sides, true solutions); cached: the variants reuse it."""
    key = (name, values, seed)
    if key not in _REF:
        d = ft.build(ft.DESIGNS[name][0], values=values, seed=seed)
        o = oracle.linear_solver_ORACLE("symmetric", perm=d.perm)
        o.ls_factor_b(d.A, d.npos, d.nneg)
        M = ft.full_csr(d.A)
        B = ft.rhs(d.n, 5)
        XT = np.array([ft.true_solution(M, o.ls_solve, b) for b in B])
        _REF[key] = (d, o, M, B, XT)
    return _REF[key]


def check_factor(d, o, inertia, D, Lh, tol_d=TOL_D, tol_l=TOL_L):
    """shape (the designed L pattern, relaxed zeros stored: panel boundaries visible), inertia, sign(D), D and L against the oracle"""
    P = d.l_pattern()
    Lh = sp.csc_matrix(Lh)
    Lh.sort_indices()
    assert np.array_equal(Lh.indptr, P.indptr) and np.array_equal(Lh.indices, P.indices), "the fronts are not the designed ones"
    assert tuple(inertia[:3]) == tuple(o.inertia()[:3]), (inertia, o.inertia())
    d_o = o.diag()
    assert np.array_equal(np.sign(D), np.sign(d_o))
    e_d = float(np.max(np.abs(D - d_o) / np.abs(d_o)))
    Lo = o.L()
    e_l = float(abs(Lh - Lo).max() / abs(Lo).max())
    assert e_d <= tol_d and e_l <= tol_l, (e_d, e_l)
    return e_d, e_l


def route_of(d):
    """'inverse' when a big front has more than 384 pivot columns (explicit inverses of 1024-column blocks), else 'substitution'"""
    return "inverse" if any(k > 384 and f > SMALL_MAX for k, f, _ in d.fronts) else "substitution"


@pytest.mark.parametrize("name", list(ft.DESIGNS))
def test_designed_fronts_plain_values(name):
    """One design, "plain" values: shape, inertia, D and L against the oracle; three solves of one vector after the factorisation
    (the last two bitwise equal), batches of 1, 4 and 5 right-hand sides (5: two passes of at most kMaxRhs = 4) each column equal to
    its single solve, every solution within TOL_X of the true solution; then new values on the same pattern and handle give, bit for
    bit, the D, L and x of a fresh handle (nothing stale in the shared CB region or the solve's inverses)."""
    d, o, M, B, XT = reference(name)
    h = hip_solver()
    h.set_perm(d.perm)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == o.ls_factor_b(d.A, d.npos, d.nneg)
    assert np.array_equal(h.perm(), d.perm)
    st = h.stats()
    assert {k: st[k] for k in d.fingerprint()} == d.fingerprint()
    xs = [h.ls_solve(B[0]) for _ in range(3)]
    for x in xs:
        assert ft.fwd_err(x, XT[0]) <= TOL_X
    assert np.array_equal(xs[1], xs[2])
    check_factor(d, o, h.inertia, h.diag(), h.factor_csc())
    singles = np.array([h.ls_solve(b) for b in B])
    errs = [ft.fwd_err(x, xt) for x, xt in zip(singles, XT)]
    assert max(errs) <= TOL_X, errs
    for nrhs in (1, 4, 5):
        X = solve_batch(h, B[:nrhs])
        for r in range(nrhs):
            assert np.max(np.abs(X[r] - singles[r])) <= TOL_BATCH * np.max(np.abs(singles[r])), (nrhs, r)
            assert ft.fwd_err(X[r], XT[r]) <= TOL_X, (nrhs, r)
    # refactorisation: other values, the same pattern, the same handle -- against a fresh handle
    d2 = ft.build(ft.DESIGNS[name][0], seed=1)
    assert np.array_equal(d2.A.indices, d.A.indices) and np.array_equal(d2.A.indptr, d.A.indptr)
    runs = []
    for hh in (h, hip_solver()):
        if hh is not h:
            hh.set_perm(d.perm)
        hh.ls_factor_b(d2.A, d2.npos, d2.nneg)
        Lh = hh.factor_csc()
        runs.append((hh.inertia, hh.diag(), Lh.data, [hh.ls_solve(B[0]) for _ in range(3)], solve_batch(hh, B)))
        finalize_b(hh)
    (i1, D1, L1, x1, X1), (i2, D2, L2, x2, X2) = runs
    assert i1 == i2 and np.array_equal(D1, D2) and np.array_equal(L1, L2)
    for a, b in zip(x1, x2):
        assert np.array_equal(a, b)
    assert np.array_equal(X1, X2)
    print(f"FRONTSHAPE {json.dumps(dict(name=name, values='plain', route=route_of(d), err=max(errs)))}")


@pytest.mark.parametrize("name", list(ft.DESIGNS))
def test_ipm_values_forward_error(name):
    """One design, "ipm" values (late interior-point scaling, quasi-definite: -s/y from 1e-6 to 1e6 on the negative columns, then
    equilibrated): inertia equal to the oracle's, D and L, and the forward error of two right-hand sides against the true solution.
    Substitution routes (no pivot block of more than 384 columns): at most 2 x the oracle's error -- measured 0.12 .. 1.12 x (the
    oracle at 5e-15 .. 6e-11).  Explicit-inverse routes: at most 2 x the ratio measured on MI355X, 0.13 .. 2.8 x (IPM_INV_RATIO).
    D and L within TOL_D / TOL_L as for the plain values (measured at most 1.1e-11 and 1.2e-13)."""
    d, o, M, B, XT = reference(name, "ipm")
    h = hip_solver()
    h.set_perm(d.perm)
    assert h.ls_factor_b(d.A, d.npos, d.nneg) == o.ls_factor_b(d.A, d.npos, d.nneg)
    assert tuple(h.inertia[:3]) == (d.npos, d.nneg, 0)
    e_d, e_l = check_factor(d, o, h.inertia, h.diag(), h.factor_csc(), tol_d=np.inf, tol_l=np.inf)
    e_h = max(ft.fwd_err(h.ls_solve(b), xt) for b, xt in zip(B[:2], XT[:2]))
    e_o = max(ft.fwd_err(o.ls_solve(b), xt) for b, xt in zip(B[:2], XT[:2]))
    finalize_b(h)
    route = route_of(d)
    print(f"FRONTSHAPE {json.dumps(dict(name=name, values='ipm', route=route, e_hip=e_h, e_oracle=e_o, e_d=e_d, e_l=e_l))}")
    assert e_d <= TOL_D and e_l <= TOL_L, (e_d, e_l)
    bound = 2.0 if route == "substitution" else 2.0 * IPM_INV_RATIO[name]
    assert e_h <= bound * e_o, (e_h, e_o)


# ---- the same designs under the other routes (subprocesses) -----------------------------------------------------------------------
VARIANTS = {
    "default": ({}, {}),
    "DATAFLOW=0": ({"OKKT_DATAFLOW": "0"}, {}),
    "SOLVE_MID=0": ({"OKKT_SOLVE_MID": "0"}, {}),
    "SOLVE_MID=1024": ({"OKKT_SOLVE_MID": "1024"}, {}),
    "SOLVE_ROUTE_THIN=0": ({"OKKT_SOLVE_ROUTE_THIN": "0"}, {}),
    "FOLD_LONE=0": ({"OKKT_FOLD_LONE": "0"}, {}),
    "TASKS=0": ({"OKKT_TASKS": "0"}, {}),
    "RELEASE_CB=0": ({"OKKT_RELEASE_CB": "0"}, {}),
    "DEBUG_POISON=1": ({"OKKT_DEBUG_POISON": "1"}, {}),
    "panel_nb=64,small_front_max=32": ({}, {"panel_nb": 64, "small_front_max": 32}),
}
_RUNS = {}


def run_case(variant, names, debug=False):
    key = (variant, tuple(names), debug)
    if key not in _RUNS:
        env, opts = VARIANTS[variant]
        e = dict(os.environ)
        e.update(env)
        if debug:
            e["OKKT_DEBUG_FRONTS"] = "1"
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "case.npz")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "front_shapes_case.py"), out, json.dumps(opts), *names],
                               cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "CASE_OK" in r.stdout, (variant, r.stdout[-400:], r.stderr[-1500:])
            with np.load(out) as z:
                res = {k: z[k] for k in z.files}
        _RUNS[key] = (res, r.stderr)
    return _RUNS[key]


def check_case(res, name):
    d, o, M, B, XT = reference(name)
    Lh = sp.csc_matrix((res[f"{name}/Lx"], res[f"{name}/Li"], res[f"{name}/Lp"]), shape=(d.n, d.n))
    assert np.array_equal(res[f"{name}/perm"], d.perm)
    check_factor(d, o, res[f"{name}/inertia"], res[f"{name}/D"], Lh)
    X = res[f"{name}/X"]
    errs = [ft.fwd_err(x, xt) for x, xt in zip(X, XT)]
    assert max(errs) <= TOL_X, errs


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_designs_under_route_switches(variant):
    """The mixed-level, fan-in, deep-chain and k = 2049 / c = 129 designs under every route switch: the same checks against the
    oracle.  Without released CBs (each front its own f x f buffer) the results are bitwise those of the default run."""
    res, _ = run_case(variant, ft.VARIANT_DESIGNS)
    for name in ft.VARIANT_DESIGNS:
        check_case(res, name)
    if variant == "RELEASE_CB=0":
        base, _ = run_case("default", ft.VARIANT_DESIGNS)
        for k in base:
            assert np.array_equal(res[k], base[k]), k


def parse_routes(stderr):
    """design -> (big fronts [(level, f, k)], dataflow levels [fronts], small-class counts per level)"""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.match(r"okkt-case: design (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), ([], [], {}))
            continue
        if cur is None:
            continue
        m = re.search(r"big front level (\d+)\s+f (\d+)\s+k (\d+)", line)
        if m:
            cur[0].append(tuple(int(v) for v in m.groups()))
        m = re.search(r"dataflow level: (\d+) fronts", line)
        if m:
            cur[1].append(int(m.group(1)))
        m = re.search(r"level (\d+) units by class: (\d+) \(<= 32\) (\d+) \(<= 64\) (\d+) \(<= small_max\) (\d+) \(big\)", line)
        if m:
            cur[2][int(m.group(1))] = tuple(int(v) for v in m.groups()[1:])
    return out


def test_every_designed_big_front_takes_its_route():
    """OKKT_DEBUG_FRONTS on every design: each designed big front (f > small_max) is scheduled as a big front of its level with its
    own f and k, each level of big fronts is one dataflow launch of all of them; the lone mid-size fronts of the fold designs join the
    big fronts up to the limit of 3 and stay in the small classes past it.  (Levels of units equal the designed levels here: the only
    designs with small fronts below a big one are the small-class and task-chain designs, whose big fronts are compared without level.)"""
    names = list(ft.DESIGNS)
    res, err = run_case("default", names, debug=True)
    routes = parse_routes(err)
    for name in names:
        print(f"FRONTROUTE {json.dumps(dict(name=name, big=routes[name][0], dataflow=routes[name][1], classes=routes[name][2]))}")
    for name in names:
        if name in ft.VARIANT_DESIGNS:
            check_case(res, name)
        d = ft.build(ft.DESIGNS[name][0])
        big, df, cls = routes[name]
        want = sorted((lv, f, k) for k, f, lv in d.fronts if f > SMALL_MAX)
        folded = sorted((lv, f, k) for k, f, lv in d.fronts if 32 < f <= SMALL_MAX and lv == 0) if name in ("fold-lone-1", "fold-lone-3") else []
        got = sorted(big)
        if name.startswith(("small-classes", "task-chains")):
            assert sorted(x[1:] for x in got) == sorted(x[1:] for x in want), (name, got, want)
        else:
            assert got == sorted(want + folded), (name, got, want, folded)
            per_level = {}
            for lv, _, _ in got:
                per_level[lv] = per_level.get(lv, 0) + 1
            assert sorted(df) == sorted(per_level.values()), (name, df, per_level)
        if name == "fold-lone-4":
            assert cls[0][1] + cls[0][2] == 4, cls
    mixed = routes["mixed-level"][0]
    assert sorted(x for x in mixed if x[0] == 0) == [(0, 300, 100), (0, 450, 300), (0, 450, 450), (0, 750, 500)]
