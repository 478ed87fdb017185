"""GPU tests: Schur mode (okkt_set_schur / okkt_factor_schur / okkt_get_schur / condense / expand / the dense factor and the fused
solve, DESIGN.md sections 8.4 and 8.7) on designed trees (schur_trees.py).  The other Schur tests take the fronts an ordering finds
under random sets; here the set is the last root of a designed forest, so every class of child under the Schur front (small fronts
of each LDS class, chains of small fronts run as tasks, thin / mid / wide big fronts, scattered CBs, eight CBs alive together), the
set sizes 2, 17, 64, 65, 128, 129, 130, 256, 257, 2048, 2049 and 2101 (the chunked assembly), a set without children, interior roots
that never touch the set and batches of 1 .. 5 right-hand sides (2: the R = 2 kernels) are made to happen on purpose.

The reference is the long-double S and r2 of schur_trees.reference and the true solution of the whole system.  The accuracy rule
for S and r2: the whole-matrix oracle does the device's elimination in the same order in fp64; its own distance from the reference,
e_oracle, is the yardstick, and the device may be at most 2 x max(1, RATIO) x e_oracle away, RATIO the device's e_dev / e_oracle
as measured once on MI355X (the tables below; the device is deterministic, the factor 2 covers other seeds).  Where the set has no
child, e_oracle is 0 and so must e_dev be: S is A22 and r2 is b2, bit for bit.
The route switches (read once per process) run in subprocesses (schur_trees_case.py)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import front_trees as ft  # noqa: E402
import schur_trees as sct  # noqa: E402
from onephase_jl_amd.linear_system_solvers import finalize_b  # noqa: E402
from schur_trees_case import BATCHES  # noqa: E402
from test_gpu_front_shapes import SMALL_MAX, TOL_BATCH, TOL_X, parse_routes  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# e_dev / e_oracle of S and of r2 (worst of the batches of 1 .. 5 right-hand sides), measured on MI355X: the SCHURTREE lines of one run
# of this file, (S, r2) per design; 1.0 where e_oracle = 0 (no child).  e_oracle is 0.3e-16 .. 4.4e-16 (S) and 0.7e-16 .. 1.9e-15 (r2)
# with "plain" values.  The oracle's S sums the products of a column and rounds once at the size of A22's entry; the device rounds
# once per child that adds its CB: the largest ratios belong to the sets with 4 and 6 children on every diagonal entry (3.25, 2.87)
# and to the set of 2 rows whose e_oracle happens to be 0.3e-16 (2.45).  The route switches measured the same figures for S and r2 figures within 15 % of these.
RATIO = {
    "plain": {
        "edge-k129-c700": (0.98, 0.78), "edge-k255-c129": (1.12, 0.75), "edge-k257-c127": (0.96, 0.72), "edge-k383-c63": (0.98, 0.88),
        "edge-k384-c128": (0.85, 0.84), "edge-k385-c1": (2.45, 0.70), "edge-k1023-c128": (1.24, 0.60), "edge-k1024-c63": (0.82, 0.73),
        "edge-k1025-c1": (0.21, 0.86), "edge-k2048-c127": (0.80, 0.72), "edge-k2049-c129": (1.06, 0.54),
        "thin-tall-k1-2-127-128-c2100": (3.25, 1.51), "thin-k128-f2049": (1.00, 1.00), "small-classes-f32-33-64-65-128-129": (1.39, 0.93),
        "task-chains-under-big": (1.42, 0.38), "fold-lone-1": (1.32, 0.61), "fold-lone-3": (1.32, 0.45), "fold-lone-4": (1.33, 0.57),
        "mixed-level": (1.00, 1.00), "mixed-level-scatter": (1.00, 1.00), "forest-3-roots": (1.00, 1.00), "deep-chain-6": (0.96, 0.33),
        "fan-in-8": (1.73, 0.30), "set-65-small-only": (1.37, 0.61), "set-256": (0.99, 1.00), "set-257": (1.28, 0.74),
        "set-2048": (1.00, 0.50), "set-2049-thin": (2.87, 1.19), "lone-roots-then-set": (0.98, 0.60),
    },
    # e_oracle 7.7e-16 .. 5.9e-13 (S), 2.8e-15 .. 7.5e-12 (r2)
    "ipm": {
        "set-65-small-only": (2.06, 0.87), "set-257": (0.41, 0.42), "set-2049-thin": (0.44, 0.46), "fan-in-8": (0.68, 1.62),
        "task-chains-under-big": (1.02, 0.74), "edge-k1025-c1": (0.84, 0.68),
    },
}
# "ipm" values: forward error of the fused solve / that of numpy.linalg.solve on the dense fp64 matrix, measured on MI355X.  Every
# design is above 2, for one reason: numpy's LU pivots, the factorisation of A11 does not (static pivoting in the designed order),
# and with s/y from 1e-6 to 1e6 on the diagonal an unpivoted elimination loses what the whole-matrix oracle on the same order loses.
# The oracle's own forward error on these systems (e_oracle_solve in the SCHURTREE lines) is 3.6e-12, 1.0e-13, 3.6e-12, 2.4e-12,
# 8.1e-15 and 2.1e-10 against numpy's 0.5e-14 .. 4.6e-14; the fused solve measured at most 1.9 x the oracle's.
IPM_SOLVE_RATIO = {
    "set-65-small-only": 360.73, "set-257": 5.87, "set-2049-thin": 252.25, "fan-in-8": 12.16, "task-chains-under-big": 2.19, "edge-k1025-c1": 2339.10,
}


def ratio(values, name):
    return RATIO[values][name]


def inertia_of(w):
    return int((w > 0).sum()), int((w < 0).sum())


def check_results(r, res, values, batches, solutions=True):
    """One factorisation's results (schur_trees.device_results) against the reference r: the flag and the inertia of A11, S
    symmetric, S = A22 wherever no child's CB reaches, S and r2 under the accuracy rule, the inertias of the dense factor, and
    (solutions) the expanded and the fused solutions within TOL_X of the true one.  Returns the measured figures."""
    d, name = r.d, r.name
    assert int(res["flag"]) == 1 and tuple(res["inertia"]) == (r.n1pos, r.n1neg, 0, 0), (res["flag"], res["inertia"])
    S = res["S"]
    assert S.shape == (r.ns, r.ns) and np.array_equal(S, S.T)
    away = ~r.reached
    assert np.array_equal(S[away], r.A22[away]), "an entry no contribution block reaches is not A22"
    rs, rr = ratio(values, name)
    e_s = float(np.max(np.abs(S - r.S_ref)) / r.smax)
    fig = dict(name=name, values=values, ns=r.ns, e_S=e_s, e_oracle_S=r.e_oracle_S, e_oracle_r2=r.e_oracle_r2)
    e_r2 = 0.0
    for nr in batches:
        e_r2 = max(e_r2, float(np.max(np.abs(res[f"r2/{nr}"] - r.R2_ref[:nr])) / r.rmax))
    fig["e_r2"] = e_r2
    fig["ratio_S"] = e_s / r.e_oracle_S if r.e_oracle_S > 0 else (1.0 if e_s == 0 else np.inf)
    fig["ratio_r2"] = e_r2 / r.e_oracle_r2 if r.e_oracle_r2 > 0 else (1.0 if e_r2 == 0 else np.inf)
    if solutions:
        fig["err_expand"] = max(ft.fwd_err(x, xt) for nr in batches for x, xt in zip(res[f"xe/{nr}"], r.XT))
        fig["err_solve"] = max(ft.fwd_err(x, xt) for nr in batches for x, xt in zip(res[f"xs/{nr}"], r.XT))
    print(f"SCHURTREE {json.dumps(fig)}")
    assert e_s <= 2.0 * max(1.0, rs) * r.e_oracle_S, (e_s, r.e_oracle_S, rs)
    assert e_r2 <= 2.0 * max(1.0, rr) * r.e_oracle_r2, (e_r2, r.e_oracle_r2, rr)
    assert int(res["sflag"]) == 1
    assert tuple(res["total_inertia"]) == (d.npos, d.nneg, 0, 0), res["total_inertia"]
    assert tuple(res["schur_inertia"]) == inertia_of(r.eig) + (0, 0), (res["schur_inertia"], inertia_of(r.eig))
    assert np.array_equal(res["S_after"], S)      # the dense factor works on a copy
    if solutions:
        assert fig["err_expand"] <= TOL_X and fig["err_solve"] <= TOL_X, fig
    return fig


reference = sct.reference


@pytest.mark.parametrize("name", list(sct.DESIGNS))
def test_schur_on_designed_tree_plain_values(name):
    """One design, "plain" values: S, the inertias, r2, the expansion of the reference's x2 and the fused solve against the
    reference; batches of 1 .. 5 right-hand sides, each column within TOL_BATCH of its single call and bitwise equal on a repeated
    call; then other values on the same handle give bit for bit the S, r2 and x of a fresh handle, and the first values the first S."""
    r = reference(name)
    d, B, X2 = r.d, r.B, r.X2
    if name in sct.CHILDLESS:
        assert not r.reached.any() and r.e_oracle_S == 0.0 and r.e_oracle_r2 == 0.0
    h = sct.schur_handle(d)
    assert np.array_equal(h.perm(), d.perm)
    st = h.stats()
    assert {k: st[k] for k in d.fingerprint()} == d.fingerprint()
    batches = (1, 2, 3, 4, 5)
    res = sct.device_results(h, d, r.n1pos, r.n1neg, B, X2, batches=batches)
    check_results(r, res, "plain", batches)
    calls = {"r2": lambda nr, rows: h.schur_condense(B[rows]), "xe": lambda nr, rows: h.schur_expand(B[rows], X2[rows]),
             "xs": lambda nr, rows: h.schur_solve(B[rows])}
    for what, call in calls.items():
        singles = np.array([call(1, slice(i, i + 1)).ravel() for i in range(sct.NRHS)])
        for nr in batches:
            again = call(nr, slice(0, nr)).reshape(nr, -1)
            assert np.array_equal(again, res[f"{what}/{nr}"]), (what, nr)
            for i in range(nr):
                assert np.max(np.abs(again[i] - singles[i])) <= TOL_BATCH * np.max(np.abs(singles[i])), (what, nr, i)
    # refactorisation: other values, the same pattern, the same handle -- against a fresh handle; then back
    d2 = sct.build(name, seed=1)
    assert np.array_equal(d2.A.indices, d.A.indices) and np.array_equal(d2.A.indptr, d.A.indptr)
    p2 = sct.interior_positive(d2)
    runs = []
    for hh in (h, sct.schur_handle(d)):
        runs.append(sct.device_results(hh, d2, p2, r.n1 - p2, B, X2, batches=(sct.NRHS,)))
        if hh is not h:
            finalize_b(hh)
    assert int(runs[0]["flag"]) == 1
    assert not np.array_equal(runs[0]["S"], res["S"])
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    back = sct.device_results(h, d, r.n1pos, r.n1neg, B, X2, batches=(sct.NRHS,))
    for k in back:
        assert np.array_equal(back[k], res[k]), k
    finalize_b(h)


@pytest.mark.parametrize("name", sct.IPM_DESIGNS)
def test_schur_on_designed_tree_ipm_values(name):
    """One design, "ipm" values (late interior-point scaling, then equilibrated): the same checks of S, r2 and the inertias, and the
    forward error of the fused solve at most 2 x the ratio to numpy.linalg.solve on the dense fp64 matrix that IPM_SOLVE_RATIO
    records (every design measured above 2; the reason is there)."""
    r = reference(name, "ipm")
    d, B = r.d, r.B
    h = sct.schur_handle(d)
    res = sct.device_results(h, d, r.n1pos, r.n1neg, B, r.X2, batches=(sct.NRHS,))
    finalize_b(h)
    Xn = np.linalg.solve(r.M.toarray(), B.T).T
    e_np = max(ft.fwd_err(x, xt) for x, xt in zip(Xn, r.XT))
    e_dev = max(ft.fwd_err(x, xt) for x, xt in zip(res[f"xs/{sct.NRHS}"], r.XT))
    print(f"SCHURTREE {json.dumps(dict(name=name, values='ipm', e_solve=e_dev, e_numpy=e_np, e_oracle_solve=r.e_oracle_solve, ratio_solve=e_dev / e_np))}")
    check_results(r, res, "ipm", (sct.NRHS,), solutions=False)
    assert e_dev <= 2.0 * max(1.0, IPM_SOLVE_RATIO[name]) * e_np, (e_dev, e_np)


# ---- the route switches (subprocesses) --------------------------------------------------------------------------------------------
VARIANTS = {
    "default": ({}, {}),
    "DATAFLOW=0": ({"OKKT_DATAFLOW": "0"}, {}),
    "TASKS=0": ({"OKKT_TASKS": "0"}, {}),
    "FOLD_LONE=0": ({"OKKT_FOLD_LONE": "0"}, {}),
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
        given = {f"{name}/X2": reference(name).X2 for name in names if name in sct.VARIANT_DESIGNS}
        with tempfile.TemporaryDirectory() as tmp:
            inp, out = os.path.join(tmp, "given.npz"), os.path.join(tmp, "case.npz")
            np.savez(inp, **given)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schur_trees_case.py"), inp, out, json.dumps(opts), *names],
                               cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0 and "CASE_OK" in p.stdout, (variant, p.stdout[-400:], p.stderr[-1500:])
            with np.load(out) as z:
                res = {k: z[k] for k in z.files}
        _RUNS[key] = (res, p.stderr)
    return _RUNS[key]


def of_design(res, name):
    return {k[len(name) + 1:]: v for k, v in res.items() if k.startswith(name + "/")}


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "default"])
def test_schur_designs_under_route_switches(variant):
    """The small-only, task-chain, fan-in and chunked designs under every route switch: the checks of the plain test, without the
    refactorisation.  Without released CBs (each front its own f x f buffer) S and r2 are bitwise those of the default run."""
    res, _ = run_case(variant, sct.VARIANT_DESIGNS)
    for name in sct.VARIANT_DESIGNS:
        one = of_design(res, name)
        assert np.array_equal(one["perm"], reference(name).d.perm)
        check_results(reference(name), one, "plain", BATCHES)
    if variant == "RELEASE_CB=0":
        base, _ = run_case("default", sct.VARIANT_DESIGNS)
        for k in base:
            if k.split("/")[1] in ("S", "r2", "flag", "inertia"):
                assert np.array_equal(res[k], base[k]), k


def test_schur_front_is_in_no_schedule():
    """OKKT_DEBUG_FRONTS on every Schur design: the scheduled big fronts are exactly the designed interior fronts of more than
    small_max rows (and the lone mid-size fronts the fold rule moves to them), each level of them is one dataflow launch of all of
    them -- the Schur front, whatever its size, is in no level and in no dataflow launch."""
    names = list(sct.DESIGNS)
    res, err = run_case("default", names, debug=True)
    routes = parse_routes(err)
    for name in names:
        print(f"SCHURROUTE {json.dumps(dict(name=name, big=routes[name][0], dataflow=routes[name][1], classes=routes[name][2]))}")
    for name in names:
        if name in sct.VARIANT_DESIGNS:
            check_results(reference(name), of_design(res, name), "plain", BATCHES)
        d = sct.build(name)
        ns = sct.set_size(d)
        big, df, cls = routes[name]
        interior = d.fronts[:-1]
        want = sorted((lv, f, k) for k, f, lv in interior if f > SMALL_MAX)
        # the fold rule: up to 3 lone leaf fronts of 33 .. small_max rows join the big fronts of their level
        parents = {nd["parent"] for nd in d.nodes}
        lone = sorted((lv, f, k) for i, (k, f, lv) in enumerate(interior) if 32 < f <= SMALL_MAX and i not in parents)
        folded = lone if want and 1 <= len(lone) <= 3 else []
        got = sorted(big)
        assert not any(f == ns and k == ns for _, f, k in got), (name, got)
        assert got == sorted(want + folded), (name, got, want, folded)
        per_level = {}
        for lv, _, _ in got:
            per_level[lv] = per_level.get(lv, 0) + 1
        assert sorted(df) == sorted(per_level.values()), (name, df, per_level)
