"""The two direction entry points share one pass (kkt.hip): okkt_kkt_compute_directions with a single triple must give, bit for bit,
what okkt_kkt_system_rhs + okkt_kkt_compute_direction give for that triple -- dx, dy, ds, every field of okkt_kkt_error and the
solve count of the timers -- for every kind the pass serves, with and without a residual round, with dense rows of J and with the
refined solve of the symmetric kind."""
import os
import sys

import numpy as np
import pytest

from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_schur_dense_rows as td  # noqa: E402

pytestmark = pytest.mark.gpu

# S-tiny has n = 40 and rows of J of at most 4 entries; the three appended rows hold 24 to 40, so a threshold of 20 entries
# (schur_dense_rows > 0: rows longer than that) makes exactly them the border
DENSE_THRESHOLD = 20

#        name                 kind            moved  dense  handle options
CASES = [("schur",            "schur",        False, False, {}),
         ("schur_direct",     "schur_direct", True,  False, {}),
         ("symmetric",        "symmetric",    False, False, {}),
         ("symmetric_refine", "symmetric",    False, False, dict(hip_ls_refine_steps=2, hip_ls_refine_tol=0.0)),
         ("schur_dense",      "schur",        False, True,  dict(schur_dense_rows=DENSE_THRESHOLD)),
         ("schur_direct_dense", "schur_direct", True, True, dict(schur_dense_rows=DENSE_THRESHOLD))]

_PROBLEMS = {}


def problem(dense):
    if dense not in _PROBLEMS:
        prob = synth.make_config("S-tiny", seed=4, well_scaled=True)
        _PROBLEMS[dense] = td.with_dense_rows(prob, 3, seed=4) if dense else prob
    return _PROBLEMS[dense]


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("name,kind,moved,dense,opts", CASES, ids=[c[0] for c in CASES])
def test_one_triple_through_both_entry_points(name, kind, moved, dense, opts, rounds):
    prob = problem(dense)
    it = td.synth_iterate(prob, KS.Class_iterate, 4)
    pars = KS.Class_parameters()
    pars.kkt.ItRefine_Num = rounds
    k = KS.HIP_KKT_solver(kind, pars, **opts)
    k.initialize_b(it)
    k.form_system_b(it)
    assert k.factor_b(1e-6) == 1
    if dense:
        assert list(k.dense_rows()) == list(range(prob["m"] - 3, prob["m"]))
    # schur_direct reads y, s and J of the current iterate: a moved one makes cur_Jcsr differ from Jcsr
    cur = td.moved(KS.Class_iterate, it, 4) if moved else it
    eta = KS.Reduct_stable()
    k.kkt_associate_rhs_b(cur, eta)
    [(d, kerr)] = k.compute_directions_b([eta])
    solves_batched = k.timers()["n_solves"]
    k.kkt_associate_rhs_b(cur, eta)
    k.compute_direction_b()
    solves_single = k.timers()["n_solves"]
    one = k.kkt_err_norm
    fields = ("error_D", "error_P", "error_mu", "overall", "rhs_norm", "ratio")
    print("DIRECTION_PATHS", name, rounds, solves_batched, solves_single,
          [float(np.max(np.abs(getattr(d, a) - getattr(k.dir, a)))) for a in ("x", "y", "s")],
          [(getattr(kerr, f), getattr(one, f)) for f in fields])
    for a in ("x", "y", "s"):
        assert np.array_equal(getattr(d, a), getattr(k.dir, a)), (name, rounds, a)
    for f in fields:
        assert getattr(kerr, f) == getattr(one, f), (name, rounds, f)
    assert solves_batched == solves_single
    if kind != "symmetric":
        assert solves_single == rounds
    elif not opts:
        assert solves_single == 1
    k.finalize_b()
