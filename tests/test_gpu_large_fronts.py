"""Fronts of more than 2^31 entries: S-metric-5x (n + m = 5e5) has a largest front of 47 255 rows, 47 255^2 = 2.23e9 > 2^31.
Until the front-local offsets became 64-bit (symbolic.h aent_dst, the assembly kernels) the single-GPU plan refused every front above
46 000 rows; the partitioned plan (okkt_dist_*) still does, with an explicit message.

The CPU oracle cannot serve as the reference at 5.6e13 flops, so the factor is judged by what it does: the inertia of a quasi-definite
matrix, the normwise backward error of its solutions against the same figure at S-metric-4x (largest front 37 860 rows, below the old
limit), and iterative refinement with long-double residuals -- a factor corrupted past 2^31 elements would make refinement stagnate."""
import numpy as np
import pytest

from onephase_jl_amd import synth
from onephase_jl_amd import kkt_system_solver as KS
from onephase_jl_amd.linear_system_solvers import OkktError, finalize_b, initialize_b, linear_solver_HIP

OFFSET_ROWS = 46_341          # the least f with f * f > 2^31 - 1
PARTED_REFUSAL = "partitioned plans take fronts of at most 46000 rows"
# normwise backward error ||Kx - b|| / (||K|| ||x|| + ||b||) (inf-norms) of the two seed-7 right-hand sides, measured on an MI355X:
# 2.7e-16 / 1.4e-16 at S-metric-4x, 2.0e-16 / 4.1e-16 at S-metric-5x.  Asserted: within 10 x the worst 4x figure
BACKWARD_BOUND = 10 * 2.7e-16
NERR_FACTOR = 10.0        # N err of the 5x direction against the metric size's (measured 1.3e-11 and 4.7e-10)


def hip_solver(sym, **o):
    s = linear_solver_HIP(sym, False, False, **o)
    initialize_b(s)
    return s


def residual(M, x, b):
    """b - M x with the products and the sums in long double (M: CSR of the full symmetric matrix)"""
    prod = M.data.astype(np.longdouble) * x.astype(np.longdouble)[M.indices]
    return (b.astype(np.longdouble) - np.add.reduceat(prod, M.indptr[:-1])).astype(np.float64)


def five_times():
    prob = synth.make_config("S-metric-5x", seed=0)
    return prob, synth.augmented_matrix(prob, delta=1e-8)


def test_partitioned_plan_refuses_fronts_past_the_32_bit_offsets():
    """Host only (a host_symbolic_only handle): the partition request itself is refused, with the explicit message -- the partitioned
    path keeps f x f buffers and does not inherit the lifted limit."""
    prob, K = five_times()
    h = linear_solver_HIP("symmetric", host_symbolic_only=1)
    initialize_b(h)
    h.analyze(K)
    assert h.stats()["max_front"] >= OFFSET_ROWS
    with pytest.raises(OkktError, match=PARTED_REFUSAL):
        h._check(h._lib.okkt_dist_set_partition(h._h, 2, 0), "okkt_dist_set_partition")
    # a one-part "partition" is the single-GPU plan: accepted
    h._check(h._lib.okkt_dist_set_partition(h._h, 1, 0), "okkt_dist_set_partition")
    finalize_b(h)


@pytest.mark.gpu
def test_five_times_metric_factors_past_two_to_the_31_entries_per_front():
    """Inertia (n, m, 0), an arena below the f x f bound (measured 80.5 of 118.6 GB), the backward error within BACKWARD_BOUND, and two
    steps of refinement with long-double residuals: the second correction at least 1e3 x smaller than the first (measured: 6.6e-9 then
    1.1e-16 of max|x|, and 6.3e-9 then 5.7e-16)."""
    prob, K = five_times()
    n, m = prob["n"], prob["m"]
    M = synth.symmetrize_lower(K).tocsr()
    k_inf = float(np.max(np.asarray(abs(M).sum(axis=1)).ravel()))
    h = hip_solver("symmetric")
    assert h.ls_factor_b(K, n, m) == 1
    st = h.stats()
    assert st["max_front"] >= OFFSET_ROWS, st["max_front"]
    assert tuple(h.inertia[:3]) == (n, m, 0), h.inertia
    assert st["arena_bytes"] < st["arena_dense_bytes"], (st["arena_bytes"], st["arena_dense_bytes"])
    for b in np.random.default_rng(7).normal(size=(2, n + m)):
        x = h.ls_solve(b)
        assert np.all(np.isfinite(x))
        r = residual(M, x, b)
        bw = np.max(np.abs(r)) / (k_inf * np.max(np.abs(x)) + np.max(np.abs(b)))
        assert bw <= BACKWARD_BOUND, bw
        d1 = h.ls_solve(r)
        x1 = x + d1
        d2 = h.ls_solve(residual(M, x1, b))
        c1, c2 = np.max(np.abs(d1)), np.max(np.abs(d2))
        assert c2 <= 1e-3 * c1, (c1, c2)
    finalize_b(h)


def kkt_direction(name):
    """form_system! -> factor! -> compute_direction! of HIP_KKT_solver("symmetric") on the iterate bench.py's kkt_level uses"""
    prob = synth.make_config(name, seed=0)
    n, m = prob["n"], prob["m"]
    rng = np.random.default_rng(1)
    it = KS.Class_iterate(x=rng.normal(size=n), y=prob["y"], s=prob["s"], mu=float(prob["mu"]), J=prob["J"], H=prob["H"],
                          grad=rng.normal(size=n), cons=prob["s"] + 1e-3 * rng.normal(size=m))
    pars = KS.Class_parameters()
    pars.kkt.kkt_solver_type = "symmetric"
    k = KS.HIP_KKT_solver("symmetric", pars)
    k.initialize_b(it)
    k.form_system_b(it)
    flag = k.factor_b(1e-8)
    k.kkt_associate_rhs_b(it, KS.Reduct_affine())
    k.compute_direction_b()
    out = int(flag), float(k.kkt_err_norm.ratio), k.linear_solver_stats()["max_front"]
    k.finalize_b()
    return out


@pytest.mark.gpu
def test_kkt_direction_at_five_times_the_metric_size():
    """The KKT level on the 5x problem: inertia accepted and an N err of the order of the metric size's (both measured here)."""
    flag1, err1, _ = kkt_direction("S-metric")
    flag5, err5, maxf = kkt_direction("S-metric-5x")
    assert flag1 == 1 and flag5 == 1
    assert maxf >= OFFSET_ROWS, maxf
    assert np.isfinite(err5) and err5 <= NERR_FACTOR * max(err1, 1e-14), (err5, err1)


@pytest.mark.gpu
def test_partitioned_handle_on_the_five_times_pattern_is_refused():
    """The sharded solver (two virtual ranks on one GPU) on the 5x pattern: the partition is refused with the explicit message,
    before any factorisation is set up."""
    from onephase_jl_amd.distributed import LocalComm, ShardedLinearSolver
    prob, K = five_times()
    sh = ShardedLinearSolver(LocalComm(2), "symmetric")
    try:
        with pytest.raises(OkktError, match=PARTED_REFUSAL):
            sh.analyze(K)
    finally:
        sh.finalize()
