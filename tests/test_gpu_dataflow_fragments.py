"""GPU tests of the fragment map of the dataflow launch's update tasks (csrc/df_fragments.h, df_syrk_tiles in csrc/dataflow.hip): which
of a wave's 32 columns sits in which accumulator and operand register, and the operand ring's LDS image.  A renaming of registers
changes no product and no order of summation, so the dataflow launch (OKKT_DATAFLOW=1) and the per-step launches of csrc/numeric.hip
(OKKT_DATAFLOW=0, k_big_syrk: its own map, its own ring) must give D, the stored L, the inertia and a solution BIT FOR BIT -- a column
loaded, masked or stored under the wrong name would not.  The shapes are the smallest at which the map can go wrong (designed
fronts, tests/front_trees.py, amalgamation off):

  dense385      one front, f = k = 385: three whole block columns and a 1 x 1 last block; plain update tasks exist from tile column q + 2 on
  child130      k = 130, c = 301 under a root of 320 pivots: a last pivot block of 2 columns (the zero page behind it in the ring),
                contribution-block tiles of 128 / 128 / 45 rows (the row and column limits), f = 431 odd (the last row's shifted pair)
  child520      k = 520, c = 140 under a root of 200 pivots: a group of four panels, the lone last panels, a partial last tile column
  child130s     child130 with a scattered contribution block (its tile columns live in the shared region)
  child130g1    child130 with OKKT_DF_GROUP=1: every update is a task of one panel (K = 128)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESIGNS = {"dense385": "385,0,0,0", "child130": "130,301,320,0", "child520": "520,140,200,0", "child130s": "130,301,320,1"}


def run(out, env, names):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dataflow_fragments_case.py"), out] + [f"{n}:{DESIGNS[n]}" for n in names],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CASE_OK" in r.stdout, (env, r.stdout[-400:], r.stderr[-1500:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """One process per setting of the switches, every design in it."""
    d = tmp_path_factory.mktemp("fragments")
    return {"steps": run(str(d / "steps.npz"), {"OKKT_DATAFLOW": "0"}, list(DESIGNS)),
            "flow": run(str(d / "flow.npz"), {"OKKT_DATAFLOW": "1"}, list(DESIGNS)),
            "group1": run(str(d / "group1.npz"), {"OKKT_DATAFLOW": "1", "OKKT_DF_GROUP": "1"}, ["child130"])}


@pytest.mark.parametrize("name,flow", [("dense385", "flow"), ("child130", "flow"), ("child520", "flow"), ("child130s", "flow"), ("child130", "group1")],
                         ids=["dense385", "child130", "child520", "child130s", "child130g1"])
def test_the_dataflow_launch_equals_the_per_step_launches_bit_for_bit(results, name, flow):
    a, b = results["steps"], results[flow]
    n = int(a[f"{name}/n"])
    assert a[f"{name}/inertia"].tolist() == b[f"{name}/inertia"].tolist() and int(a[f"{name}/inertia"][:2].sum()) == n
    assert np.array_equal(a[f"{name}/d"], b[f"{name}/d"])
    assert np.array_equal(a[f"{name}/Lp"], b[f"{name}/Lp"]) and np.array_equal(a[f"{name}/Li"], b[f"{name}/Li"])
    assert np.array_equal(a[f"{name}/Lx"], b[f"{name}/Lx"])
    assert np.array_equal(a[f"{name}/x"], b[f"{name}/x"]) and np.isfinite(a[f"{name}/x"]).all()
