"""CPU tests of the symmetric equilibration (okkt_set_scaling): the properties of the numpy restatement
(scaling_ref.py), the condition every test input must meet so that the GPU comparisons can be exact, and the argument checks of the
ABI on a host_symbolic_only handle."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd import synth
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaling_ref as sr  # noqa: E402


def s_small_K():
    return sp.csc_matrix(sp.tril(synth.augmented_matrix(synth.make_config("S-small", seed=1), delta=1e-4)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_row_maxima_after_ten_sweeps(seed):
    A = sr.random_symmetric(400, seed)
    s, e, info = sr.ruiz(A, 10)
    assert info["zero_rows"] == 0
    assert 0.45 < info["rowmax_min"] and info["rowmax_max"] <= 2.0, info
    assert np.array_equal(s, np.ldexp(1.0, e)) and np.all(np.abs(e) <= sr.EXP_MAX)
    # the definition, entry by entry, on the dense matrix
    D = np.abs(sp.tril(A).toarray())
    D = D + np.tril(D, -1).T
    assert np.array_equal(np.max((D * s[:, None]) * s[None, :], axis=1), info["rowmax"])


def test_s_small_condition_number():
    K = s_small_K()
    s, _, info = sr.ruiz(K, 10)
    full = lambda A: (A + sp.tril(A, -1).T).toarray()
    k0 = np.linalg.cond(full(K), 1)
    k1 = np.linalg.cond(full(sr.prescaled(K, s)), 1)
    print("SCALING " + json.dumps({"test": "s_small_cond", "cond1": float(k0), "cond1_scaled": float(k1), "rowmax_min": info["rowmax_min"],
                                   "rowmax_max": info["rowmax_max"]}))
    assert k1 < k0 / 1e3, (k0, k1)
    assert 0.45 < info["rowmax_min"] and info["rowmax_max"] <= 2.0


def test_rounding_rule():
    s = np.array([0.5, 0.7071067811865475, sr.SQRT_HALF, 0.75, 1.0, 3.0, 1e-200, 1e200, 0.0, np.inf, np.nan])
    r, e = sr.round_pow2(s)
    assert list(r[:6]) == [0.5, 0.5, 1.0, 1.0, 1.0, 4.0]
    assert e[6] == -sr.EXP_MAX and e[7] == sr.EXP_MAX and list(r[8:]) == [1.0, 1.0, 1.0]


def all_inputs():
    out = dict(sr.small_cases())
    out["S-small-K"] = s_small_K()
    out["S-small-well-scaled"] = sp.csc_matrix(sp.tril(synth.augmented_matrix(synth.make_config("S-small", seed=1, well_scaled=True), delta=1e-4)))
    for seed in (0, 1, 2):
        out[f"random-400-{seed}"] = sr.random_symmetric(400, seed)
    return out


def test_inputs_keep_the_mantissas_away_from_the_rounding_threshold():
    # a condition on the inputs: a last-bit difference in a square root cannot flip a rounding
    for name, A in all_inputs().items():
        for sweeps in (1, 3, 10):
            assert sr.mantissa_margin(A, sweeps) >= 1e-6, (name, sweeps, sr.mantissa_margin(A, sweeps))


def test_zero_row_and_duplicates_in_the_restatement():
    A = sr.with_zero_row()
    s, e, info = sr.ruiz(A, 10)
    assert info["zero_rows"] == 1 and s[11] == 1.0 and e[11] == 0
    T = sr.with_duplicates_and_upper()
    dim, colptr, rowval, nzval = sr.arrays(T)
    # the same matrix in canonical form (duplicates summed, upper entries dropped) gives the same scaling
    M = sp.tril(sp.csc_matrix((nzval, rowval, colptr), shape=(dim, dim))).tocsc()
    M.sum_duplicates()
    assert np.array_equal(sr.ruiz(T, 10)[0], sr.ruiz(M, 10)[0])
    P = sr.prescaled(T, sr.ruiz(T, 10)[0])
    assert isinstance(P, tuple) and np.array_equal(P[1], colptr) and np.array_equal(P[2], rowval)


# ---- the ABI on a host_symbolic_only handle -------------------------------------------------------------------------------------

def host_handle(A=None):
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    if A is not None:
        h.analyze(A)
    return h


def err(h):
    return h._lib.okkt_last_error(h._h).decode()


def test_set_scaling_argument_refusals():
    A = sp.identity(5, format="csc")
    h = host_handle()
    lib = h._lib
    ones = np.ones(5)
    assert lib.okkt_set_scaling(None, L.OKKT_SCALE_RUIZ, 0, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_set_scaling(h._h, 3, 0, None) == L.OKKT_ERR_INVALID and "mode" in err(h)
    assert lib.okkt_set_scaling(h._h, -1, 0, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_set_scaling(h._h, L.OKKT_SCALE_RUIZ, 65, None) == L.OKKT_ERR_INVALID and "sweeps" in err(h)
    # USER needs the analysed dimension and a finite, positive vector
    assert lib.okkt_set_scaling(h._h, L.OKKT_SCALE_USER, 0, L.p_f64(ones)) == L.OKKT_ERR_INVALID and "okkt_analyze" in err(h)
    h.analyze(A)
    assert lib.okkt_set_scaling(h._h, L.OKKT_SCALE_USER, 0, None) == L.OKKT_ERR_INVALID and "NULL" in err(h)
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = ones.copy()
        v[3] = bad
        assert lib.okkt_set_scaling(h._h, L.OKKT_SCALE_USER, 0, L.p_f64(v)) == L.OKKT_ERR_INVALID and "s_user[3]" in err(h), bad
    # the setting is configuration: stored without a device, every valid form accepted
    for mode, sweeps, vec in ((L.OKKT_SCALE_RUIZ, 0, None), (L.OKKT_SCALE_RUIZ, 1, None), (L.OKKT_SCALE_RUIZ, 64, None),
                              (L.OKKT_SCALE_USER, 0, ones), (L.OKKT_SCALE_NONE, 0, None)):
        assert lib.okkt_set_scaling(h._h, mode, sweeps, None if vec is None else L.p_f64(vec)) == L.OKKT_OK, (mode, sweeps)
    h.set_scaling("ruiz", 3)
    with pytest.raises(OkktError):
        h.set_scaling("user")
    finalize_b(h)


def test_getters_without_a_device():
    h = host_handle(sp.identity(5, format="csc"))
    h.set_scaling("ruiz")
    out = np.zeros(5)
    info = L.OkktScalingInfo()
    assert h._lib.okkt_get_scaling(h._h, L.p_f64(out), C.byref(info)) == L.OKKT_ERR_NO_DEVICE
    assert h._lib.okkt_get_scaling_dev(h._h, None) == L.OKKT_ERR_NO_DEVICE
    assert h._lib.okkt_get_scaling(None, L.p_f64(out), None) == L.OKKT_ERR_INVALID
    finalize_b(h)


def test_schur_mode_excludes_scaling_in_both_orders():
    A = sp.identity(6, format="csc")
    idx = np.array([1, 4], dtype=np.int64)
    # the set first: a scaling is refused, and accepted once the set is cleared
    h = host_handle()
    h.set_schur(idx)
    h.analyze(A)
    assert h._lib.okkt_set_scaling(h._h, L.OKKT_SCALE_RUIZ, 0, None) == L.OKKT_ERR_INVALID and "Schur mode" in err(h)
    assert h._lib.okkt_set_scaling(h._h, L.OKKT_SCALE_NONE, 0, None) == L.OKKT_OK
    h.set_schur(np.array([], dtype=np.int64))
    h.set_scaling("ruiz")
    finalize_b(h)
    # the scaling first: a set is refused, clearing an empty set is not, and the set is accepted once the scaling is off
    h = host_handle(A)
    h.set_scaling("ruiz")
    assert h._lib.okkt_set_schur(h._h, 2, L.p_i64(idx)) == L.OKKT_ERR_INVALID and "scaling" in err(h)
    assert h._lib.okkt_set_schur(h._h, 0, None) == L.OKKT_OK
    h.set_scaling("none")
    h.set_schur(idx)
    finalize_b(h)


def test_partition_excludes_scaling_in_both_orders():
    prob = synth.make_config("S-small", seed=1, well_scaled=True)
    A = synth.augmented_matrix(prob, delta=1e-4)
    h = host_handle(A)
    h.set_scaling("ruiz")
    assert h._lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_ERR_INVALID and "scaling" in err(h)
    assert h._lib.okkt_dist_set_partition(h._h, 1, 0) == L.OKKT_OK
    h.set_scaling("none")
    assert h._lib.okkt_dist_set_partition(h._h, 2, 0) == L.OKKT_OK
    assert h._lib.okkt_set_scaling(h._h, L.OKKT_SCALE_RUIZ, 0, None) == L.OKKT_ERR_INVALID and "partitioned" in err(h)
    assert h._lib.okkt_dist_set_partition(h._h, 1, 0) == L.OKKT_OK
    h.set_scaling("ruiz")
    finalize_b(h)


def test_kkt_options_and_refusals():
    pars = KS.Class_parameters()
    assert pars.kkt.hip_ls_scaling == 0 and pars.kkt.hip_ls_scaling_sweeps == 0
    assert "ls_scaling" not in "".join(KS.okkt_opts_from_pars(pars.kkt))
    pars.kkt.hip_ls_scaling = 1
    pars.kkt.hip_ls_scaling_sweeps = 5
    pars.kkt.kkt_solver_type = "symmetric"
    k = KS.pick_KKT_solver(pars)
    assert (k.ls_scaling, k.ls_scaling_sweeps) == (1, 5) and "hip_ls_scaling" not in k._opts
    k2 = KS.HIP_KKT_solver("schur", hip_ls_scaling=1, hip_ls_scaling_sweeps=7, ordering=3)
    assert (k2.ls_scaling, k2.ls_scaling_sweeps) == (1, 7) and k2._opts == {"ordering": 3}
    lib = L.load()
    assert lib.okkt_kkt_set_ls_scaling(None, L.OKKT_SCALE_RUIZ, 0) == L.OKKT_ERR_INVALID
    o = L.OkktOpts()
    lib.okkt_default_opts(C.byref(o))
    o.host_symbolic_only = 1
    for kind, ok in ((L.OKKT_KKT_SCHUR, True), (L.OKKT_KKT_SCHUR_DIRECT, True), (L.OKKT_KKT_SYMMETRIC, True), (L.OKKT_KKT_CLEVER_SYMMETRIC, False)):
        kk = C.c_void_p()
        assert lib.okkt_kkt_create(C.byref(kk), C.byref(o), kind) == L.OKKT_OK
        rc = lib.okkt_kkt_set_ls_scaling(kk, L.OKKT_SCALE_RUIZ, 0)
        assert rc == (L.OKKT_OK if ok else L.OKKT_ERR_INVALID), kind
        if not ok:
            assert b"okkt_kkt_set_rescale" in lib.okkt_kkt_last_error(kk)
        assert lib.okkt_kkt_set_ls_scaling(kk, L.OKKT_SCALE_USER, 0) == L.OKKT_ERR_INVALID
        assert lib.okkt_kkt_set_ls_scaling(kk, L.OKKT_SCALE_NONE, 0) == (L.OKKT_OK if ok else L.OKKT_ERR_INVALID)
        lib.okkt_kkt_destroy(kk)
