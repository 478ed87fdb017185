"""ctypes binding of libonephase_kkt.so (C ABI: include/okkt.h).

This is the Python counterpart of the `ccall` stubs in julia/linear_solver_hip.jl: plain
pointers and sizes, no torch types.  The library is built in-tree by `__graft_entry__.build()`
(hipcc, gfx950); there is no CPU fallback -- if the shared object is missing or no HIP device is
present the compute entry points raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OKKT_LIB_PATH", os.path.join(_HERE, "libonephase_kkt.so"))   # override: A/B builds

OKKT_SYM_DEFINITE = 0
OKKT_SYM_SYMMETRIC = 1
OKKT_KKT_SCHUR = 0
OKKT_KKT_SYMMETRIC = 1
OKKT_KKT_CLEVER_SYMMETRIC = 2
OKKT_KKT_SCHUR_DIRECT = 3
OKKT_RESCALE = {"none": 0, "u_only": 1, "u_and_x": 2}
OKKT_SCALE_NONE = 0
OKKT_SCALE_RUIZ = 1
OKKT_SCALE_USER = 2
OKKT_SCALE = {"none": OKKT_SCALE_NONE, "ruiz": OKKT_SCALE_RUIZ, "user": OKKT_SCALE_USER}

OKKT_OP_L = 1
OKKT_OP_LT = 2
OKKT_OP_LDLT = 3
OKKT_OP_ABS_LDLT = 4
OKKT_OP = {"L": OKKT_OP_L, "LT": OKKT_OP_LT, "LDLT": OKKT_OP_LDLT, "ABS_LDLT": OKKT_OP_ABS_LDLT}

# uniform batches: why a plan takes none (okkt_batch_info.reason), and the launch shapes
OKKT_BATCH_OK = 0
OKKT_BATCH_NOT_ANALYZED = 1
OKKT_BATCH_PARTITIONED = 2
OKKT_BATCH_SCHUR = 3
OKKT_BATCH_SCALING = 4
OKKT_BATCH_BIG_FRONTS = 5
OKKT_BATCH_MODE = {"auto": 0, "level": 1, "item": 2}
OKKT_KKT_ITEMS_OK = 0
OKKT_KKT_ITEMS_NO_STRUCTURE = 1
OKKT_KKT_ITEMS_CLEVER = 2
OKKT_KKT_ITEMS_SCHUR_DIRECT = 3
OKKT_KKT_ITEMS_DENSE_ROWS = 4
OKKT_KKT_ITEMS_SCALING = 5
OKKT_KKT_ITEMS_LS_REFINE = 6
OKKT_KKT_ITEMS_PLAN = 16
# scenario batches: why a plan takes none (okkt_schur_batch_info.reason), and the group size of the sums over the items
OKKT_SBATCH_OK = 0
OKKT_SBATCH_NOT_ANALYZED = 1
OKKT_SBATCH_PARTITIONED = 2
OKKT_SBATCH_NO_SET = 3
OKKT_SBATCH_BIG_FRONTS = 4
OKKT_SBATCH_SET_TOO_LARGE = 5
OKKT_SBATCH_GROUP = 32

OKKT_OK = 0
OKKT_ERR_INVALID = -1
OKKT_ERR_NO_DEVICE = -2
OKKT_ERR_HIP = -3
OKKT_ERR_ALLOC = -4
OKKT_ERR_INTERNAL = -5


class OkktOpts(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("host_symbolic_only", C.c_int32),
        ("ordering", C.c_int32),
        ("relax_always", C.c_int32),
        ("relax_small", C.c_int32),
        ("relax_mid", C.c_int32),
        ("relax_small_frac", C.c_double),
        ("relax_mid_frac", C.c_double),
        ("relax_any_frac", C.c_double),
        ("inertia_tol", C.c_double),
        ("small_front_max", C.c_int32),
        ("panel_nb", C.c_int32),
        ("early_exit", C.c_int32),
        ("schur_dense_rows", C.c_int32),
    ]


class OkktInertia(C.Structure):
    _fields_ = [("pos", C.c_int64), ("neg", C.c_int64), ("zero", C.c_int64), ("nonfinite", C.c_int64)]

    def as_tuple(self):
        return (self.pos, self.neg, self.zero, self.nonfinite)


class OkktStats(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("nnz_lower", C.c_int64),
        ("nnzL", C.c_int64),
        ("nnzL_stored", C.c_int64),
        ("flops_exact", C.c_double),
        ("flops_stored", C.c_double),
        ("arena_bytes", C.c_int64),
        ("nsuper", C.c_int64),
        ("nlevels", C.c_int64),
        ("max_front", C.c_int64),
        ("n_small_fronts", C.c_int64),
        ("n_big_fronts", C.c_int64),
        ("sum_rowidx", C.c_int64),
        ("analyze_seconds", C.c_double),
        ("last_factor_ms", C.c_double),
        ("last_solve_ms", C.c_double),
        ("pattern_hash", C.c_uint64),
        ("n_analyze_calls", C.c_int64),
        ("ordering_used", C.c_int64),
        ("critical_pivots", C.c_int64),
        ("top_separator", C.c_int64),
        ("amd_skipped", C.c_int64),
        ("flops_other", C.c_double),
        ("arena_dense_bytes", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktKktPars(C.Structure):
    _fields_ = [
        ("delta_start", C.c_double),
        ("delta_min", C.c_double),
        ("delta_max", C.c_double),
        ("delta_inc", C.c_double),
        ("delta_dec", C.c_double),
        ("delta_zero", C.c_double),
        ("ItRefine_Num", C.c_int32),
        ("max_it", C.c_int32),
    ]


class OkktKktError(C.Structure):
    _fields_ = [
        ("error_D", C.c_double),
        ("error_P", C.c_double),
        ("error_mu", C.c_double),
        ("overall", C.c_double),
        ("rhs_norm", C.c_double),
        ("ratio", C.c_double),
    ]


class OkktKktTimers(C.Structure):
    _fields_ = [
        ("assemble_ms", C.c_double),
        ("upload_ms", C.c_double),
        ("shift_ms", C.c_double),
        ("factor_ms", C.c_double),
        ("rhs_ms", C.c_double),
        ("solve_ms", C.c_double),
        ("refine_ms", C.c_double),
        ("kkt_err_ms", C.c_double),
        ("direction_ms", C.c_double),
        ("n_solves", C.c_int32),
        ("reserved", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class OkktRefineInfo(C.Structure):
    """okkt_refine_info: outcome of okkt_solve_refine (status 0 omega <= tol, 1 step limit, 2 stagnated, 3 non-finite)."""
    _fields_ = [
        ("steps", C.c_int32),
        ("status", C.c_int32),
        ("omega0", C.c_double),
        ("omega", C.c_double),
        ("resid_inf", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktGmresInfo(C.Structure):
    """okkt_gmres_info: outcome of okkt_solve_gmres (status 0 omega <= tol, 1 iteration limit, 2 stagnated, 3 non-finite)."""
    _fields_ = [
        ("iterations", C.c_int32),
        ("cycles", C.c_int32),
        ("status", C.c_int32),
        ("solves", C.c_int32),
        ("omega0", C.c_double),
        ("omega", C.c_double),
        ("resid_inf", C.c_double),
        ("work_bytes", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktCondestInfo(C.Structure):
    """okkt_condest_info: ||F||_1, the estimate of ||F^-1||_1, their product (status 0 converged, 1 iteration limit, 3 non-finite)."""
    _fields_ = [
        ("norm1", C.c_double),
        ("inv_norm1", C.c_double),
        ("cond1", C.c_double),
        ("iterations", C.c_int32),
        ("solves", C.c_int32),
        ("status", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktSelinvInfo(C.Structure):
    """okkt_selinv_info: device seconds, bytes held for Z, non-finite entries of Z (status 1 when there are any)."""
    _fields_ = [
        ("seconds_device", C.c_double),
        ("arena_bytes", C.c_int64),
        ("nonfinite", C.c_int64),
        ("status", C.c_int32),
        ("flops", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktPivotInfo(C.Structure):
    """okkt_pivot_info: the threshold u, the columns with g > 1/u, the non-finite columns, max g and its column (original index)."""
    _fields_ = [
        ("u", C.c_double),
        ("rejected", C.c_int64),
        ("nonfinite_cols", C.c_int64),
        ("max_multiplier", C.c_double),
        ("max_col", C.c_int64),
        ("seconds_device", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktFactorErrorInfo(C.Structure):
    """okkt_factor_error_info: the growth factor rho = || |L||D||L^T| e ||_inf / ||F||_inf with its two norms, the sampled backward error
    eta of the factor with the row that attains it (original index), and the probes used."""
    _fields_ = [
        ("rho", C.c_double),
        ("norm_abs_ldlt", C.c_double),
        ("norm_f", C.c_double),
        ("eta", C.c_double),
        ("eta_row", C.c_int64),
        ("probes", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktSparseInfo(C.Structure):
    """okkt_sparse_info: the sets of a sparse solve (union over the call's columns) -- supernodes in the closures, supernodes the launches
    visit, the fringe, the bytes of the panels visited, the groups, pruned (0: the ordinary sweeps ran), device seconds."""
    _fields_ = [
        ("nsuper", C.c_int64),
        ("fwd_reach", C.c_int64),
        ("bwd_reach", C.c_int64),
        ("fwd_run", C.c_int64),
        ("bwd_run", C.c_int64),
        ("fringe", C.c_int64),
        ("fringe_entries", C.c_int64),
        ("fwd_panel_bytes", C.c_int64),
        ("bwd_panel_bytes", C.c_int64),
        ("factor_panel_bytes", C.c_int64),
        ("batches", C.c_int32),
        ("pruned", C.c_int32),
        ("seconds_device", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktBatchInfo(C.Structure):
    """okkt_batch_info: whether the analysed plan takes a uniform batch (reason: OKKT_BATCH_*), the HBM of one item's slot, the tasks and
    levels of the task tree, the kernel launches of a batched factorisation / solve in level and in item mode."""
    _fields_ = [
        ("eligible", C.c_int32),
        ("reason", C.c_int32),
        ("bytes_per_item", C.c_int64),
        ("tasks_per_item", C.c_int64),
        ("levels", C.c_int32),
        ("max_front", C.c_int32),
        ("launches_factor_level", C.c_int32),
        ("launches_solve_level", C.c_int32),
        ("launches_factor_item", C.c_int32),
        ("launches_solve_item", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktKktItemsInfo(C.Structure):
    """okkt_kkt_items_info: whether the KKT handle takes a batch of iterates (reason: OKKT_KKT_ITEMS_*), the HBM of one item's slot (the
    linear solver's included), the kernel launches of one batched form_system / compute_direction."""
    _fields_ = [
        ("eligible", C.c_int32),
        ("reason", C.c_int32),
        ("bytes_per_item", C.c_int64),
        ("launches_form", C.c_int32),
        ("launches_direction", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktKktItemsLsInfo(C.Structure):
    """okkt_kkt_items_ls_info: eligible / reason as okkt_kkt_items_info, the HBM of one item's line-search slots, the kernel launches of the
    norm pass and of each batched step-side call (launches_dual_range: one pass)."""
    _fields_ = [
        ("eligible", C.c_int32),
        ("reason", C.c_int32),
        ("extra_bytes_per_item", C.c_int64),
        ("launches_dx_norm", C.c_int32),
        ("launches_max_step", C.c_int32),
        ("launches_s_bound", C.c_int32),
        ("launches_dual_range", C.c_int32),
        ("launches_predicted_reduction", C.c_int32),
        ("launches_dual_step", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktSchurBatchInfo(C.Structure):
    """okkt_schur_batch_info: whether the analysed plan takes a scenario batch (reason: OKKT_SBATCH_*), the order of the Schur set, the
    HBM of one item and of what the items share, the tasks and levels of the interior, the batch's own kernel launches."""
    _fields_ = [
        ("eligible", C.c_int32),
        ("reason", C.c_int32),
        ("ns", C.c_int64),
        ("bytes_per_item", C.c_int64),
        ("bytes_shared", C.c_int64),
        ("tasks_per_item", C.c_int64),
        ("levels", C.c_int32),
        ("max_front", C.c_int32),
        ("launches_factor", C.c_int32),
        ("launches_solve", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktScalingInfo(C.Structure):
    """okkt_scaling_info: mode and sweeps of the current factor's scaling, the extrema of the row maxima of |S F S| over its non-zero
    rows, and the number of zero rows."""
    _fields_ = [
        ("mode", C.c_int32),
        ("sweeps", C.c_int32),
        ("rowmax_min", C.c_double),
        ("rowmax_max", C.c_double),
        ("zero_rows", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktKktEigInfo(C.Structure):
    """okkt_kkt_eig_info: the Lanczos estimate of lambda_min(H + J' Sigma J) (status 0 converged, 1 step limit, 2 invariant subspace,
    3 non-finite); attempts of the delta loop with delta <= -rho - rho_margin are certified to fail."""
    _fields_ = [
        ("theta_min", C.c_double),
        ("theta_max", C.c_double),
        ("bound", C.c_double),
        ("rho", C.c_double),
        ("rho_abs", C.c_double),
        ("rho_margin", C.c_double),
        ("resid", C.c_double),
        ("steps", C.c_int32),
        ("status", C.c_int32),
        ("seconds_device", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OkktEigsOpts(C.Structure):
    """okkt_eigs_opts: nev, block, max_basis (0: default), max_restarts, tol (0: 2^-26), nlead (0 or dim: standard problem), seed."""
    _fields_ = [
        ("nev", C.c_int32),
        ("block", C.c_int32),
        ("max_basis", C.c_int32),
        ("max_restarts", C.c_int32),
        ("tol", C.c_double),
        ("nlead", C.c_int64),
        ("seed", C.c_uint64),
    ]


class OkktEigsInfo(C.Structure):
    """okkt_eigs_info: status (0 converged, 1 restart limit, 2 whole space spanned, 3 non-finite) and the counts of the iteration."""
    _fields_ = [
        ("status", C.c_int32),
        ("nconv", C.c_int32),
        ("sweeps", C.c_int32),
        ("solves", C.c_int32),
        ("restarts", C.c_int32),
        ("basis", C.c_int32),
        ("fresh_blocks", C.c_int32),
        ("dropped_columns", C.c_int32),
        ("true_residuals", C.c_int32),
        ("bytes", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/okkt.h declares, with its signature
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p
SIGNATURES = {
    "okkt_default_opts": (C.c_int, [C.POINTER(OkktOpts)]),
    "okkt_create": (C.c_int, [C.POINTER(_vp), C.POINTER(OkktOpts)]),
    "okkt_set_early_exit": (C.c_int, [_vp, C.c_int]),
    "okkt_destroy": (C.c_int, [_vp]),
    "okkt_last_error": (C.c_char_p, [_vp]),
    "okkt_version": (C.c_char_p, []),
    "okkt_set_perm": (C.c_int, [_vp, _i64p, C.c_int64]),
    "okkt_analyze": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, C.c_int]),
    "okkt_get_perm": (C.c_int, [_vp, _i64p]),
    "okkt_get_stats": (C.c_int, [_vp, C.POINTER(OkktStats)]),
    "okkt_get_etree": (C.c_int, [_vp, _i64p, _i64p]),
    "okkt_factor": (C.c_int, [_vp, _f64p, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia)]),
    "okkt_factor_dev": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia)]),
    "okkt_solve": (C.c_int, [_vp, _f64p, _f64p, C.c_int64]),
    "okkt_solve_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_residual": (C.c_int, [_vp, _f64p, _f64p, _f64p, _f64p, C.c_int64, _f64p]),
    "okkt_residual_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _f64p]),
    "okkt_debug_row_map": (C.c_int, [_vp, _i64p]),
    "okkt_solve_refine": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64, C.c_int32, C.c_double, C.POINTER(OkktRefineInfo), _f64p]),
    "okkt_solve_refine_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_double, C.POINTER(OkktRefineInfo), _f64p]),
    "okkt_solve_gmres": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(OkktGmresInfo),
                                   _f64p]),
    "okkt_solve_gmres_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(OkktGmresInfo), _f64p]),
    "okkt_condest": (C.c_int, [_vp, _f64p, C.c_int32, C.POINTER(OkktCondestInfo)]),
    "okkt_condest_dev": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(OkktCondestInfo)]),
    "okkt_condest_indices": (C.c_int64, [_vp, _i64p, C.c_int64]),
    "okkt_forward_error": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64, _f64p, _f64p]),
    "okkt_forward_error_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _f64p, _f64p]),
    "okkt_set_schur": (C.c_int, [_vp, C.c_int64, _i64p]),
    "okkt_factor_schur": (C.c_int, [_vp, _f64p, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia)]),
    "okkt_factor_schur_dev": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia)]),
    "okkt_get_schur": (C.c_int, [_vp, _f64p, C.c_int64]),
    "okkt_get_schur_dev": (C.c_int, [_vp, _vp, C.c_int64]),
    "okkt_schur_condense": (C.c_int, [_vp, _f64p, _f64p, C.c_int64]),
    "okkt_schur_condense_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_schur_expand": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64]),
    "okkt_schur_expand_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64]),
    "okkt_schur_factor": (C.c_int, [_vp, _f64p, C.c_int64, C.POINTER(OkktInertia), C.POINTER(OkktInertia)]),
    "okkt_schur_factor_dev": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(OkktInertia), C.POINTER(OkktInertia)]),
    "okkt_schur_dense_solve": (C.c_int, [_vp, _f64p, _f64p, C.c_int64]),
    "okkt_schur_dense_solve_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_schur_solve": (C.c_int, [_vp, _f64p, _f64p, C.c_int64]),
    "okkt_schur_solve_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_schur_get_factor": (C.c_int, [_vp, _f64p, C.c_int64, C.POINTER(C.c_int32)]),
    "okkt_selinv": (C.c_int, [_vp, C.POINTER(OkktSelinvInfo)]),
    "okkt_get_inverse_diag": (C.c_int, [_vp, _f64p]),
    "okkt_get_inverse_diag_dev": (C.c_int, [_vp, _vp]),
    "okkt_get_inverse_on_pattern": (C.c_int, [_vp, _f64p, _i64p]),
    "okkt_get_inverse_on_pattern_dev": (C.c_int, [_vp, _vp]),
    "okkt_get_inverse_csc": (C.c_int, [_vp, _i64p, _i64p, _f64p, _i64p]),
    "okkt_logdet": (C.c_int, [_vp, _f64p, C.POINTER(C.c_int32)]),
    "okkt_pivot_report": (C.c_int, [_vp, C.c_double, C.POINTER(OkktPivotInfo)]),
    "okkt_get_multipliers": (C.c_int, [_vp, _f64p, _i64p]),
    "okkt_get_multipliers_dev": (C.c_int, [_vp, _vp, _vp]),
    "okkt_get_rejected_pivots": (C.c_int64, [_vp, _i64p, _i64p, C.c_int64]),
    "okkt_solve_forward": (C.c_int, [_vp, _f64p, _f64p, C.c_int64]),
    "okkt_solve_forward_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_solve_backward": (C.c_int, [_vp, _f64p, _f64p, C.c_int64]),
    "okkt_solve_backward_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_quadform": (C.c_int, [_vp, _f64p, C.c_int64, _f64p, _f64p]),
    "okkt_quadform_dev": (C.c_int, [_vp, _vp, C.c_int64, _f64p, _f64p]),
    "okkt_factor_multiply": (C.c_int, [_vp, C.c_int, _f64p, _f64p, C.c_int64]),
    "okkt_factor_multiply_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int64]),
    "okkt_factor_error": (C.c_int, [_vp, _f64p, C.c_int32, C.POINTER(OkktFactorErrorInfo)]),
    "okkt_factor_error_dev": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(OkktFactorErrorInfo)]),
    "okkt_solve_sparse": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _f64p, C.c_int64, _i64p, _f64p, C.POINTER(OkktSparseInfo)]),
    "okkt_solve_sparse_dev": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _vp, C.c_int64, _i64p, _vp, C.POINTER(OkktSparseInfo)]),
    "okkt_get_inverse_columns": (C.c_int, [_vp, C.c_int64, _i64p, C.c_int64, _i64p, _f64p, C.POINTER(OkktSparseInfo)]),
    "okkt_get_inverse_columns_dev": (C.c_int, [_vp, C.c_int64, _i64p, C.c_int64, _i64p, _vp, C.POINTER(OkktSparseInfo)]),
    "okkt_sparse_reach": (C.c_int, [_vp, C.c_int64, _i64p, C.c_int64, _i64p, C.POINTER(OkktSparseInfo), C.POINTER(C.c_uint8)]),
    "okkt_schur_solve_refine": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64, C.c_int32, C.c_double, C.POINTER(OkktRefineInfo), _f64p]),
    "okkt_schur_solve_refine_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_double, C.POINTER(OkktRefineInfo), _f64p]),
    "okkt_schur_get_inverse": (C.c_int, [_vp, _f64p, C.c_int64]),
    "okkt_schur_get_inverse_dev": (C.c_int, [_vp, _vp, C.c_int64]),
    "okkt_schur_inverse_nonfinite": (C.c_int64, [_vp]),
    "okkt_schur_selinv": (C.c_int, [_vp, C.POINTER(OkktSelinvInfo)]),
    "okkt_schur_logdet": (C.c_int, [_vp, _f64p, C.POINTER(C.c_int32)]),
    "okkt_schur_condest": (C.c_int, [_vp, _f64p, C.c_int32, C.POINTER(OkktCondestInfo)]),
    "okkt_schur_condest_dev": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(OkktCondestInfo)]),
    "okkt_schur_forward_error": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64, _f64p, _f64p]),
    "okkt_schur_forward_error_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _f64p, _f64p]),
    "okkt_schur_solve_gmres": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(OkktGmresInfo),
                                         _f64p]),
    "okkt_schur_solve_gmres_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(OkktGmresInfo),
                                             _f64p]),
    "okkt_batch_query": (C.c_int, [_vp, C.c_int64, C.POINTER(OkktBatchInfo)]),
    "okkt_batch_reserve": (C.c_int, [_vp, C.c_int64, C.c_int64]),
    "okkt_batch_release": (C.c_int, [_vp]),
    "okkt_batch_set_mode": (C.c_int, [_vp, C.c_int]),
    "okkt_batch_mode_used": (C.c_int, [_vp]),
    "okkt_factor_batch": (C.c_int, [_vp, C.c_int64, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia),
                                    C.POINTER(C.c_int32)]),
    "okkt_factor_batch_dev": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _f64p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia),
                                        C.POINTER(C.c_int32)]),
    "okkt_solve_batch": (C.c_int, [_vp, C.c_int64, _f64p, _f64p, C.c_int64]),
    "okkt_solve_batch_dev": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_int64]),
    "okkt_batch_select": (C.c_int, [_vp, C.c_int64]),
    "okkt_schur_batch_query": (C.c_int, [_vp, C.c_int64, C.POINTER(OkktSchurBatchInfo)]),
    "okkt_schur_batch_reserve": (C.c_int, [_vp, C.c_int64, C.c_int64]),
    "okkt_schur_batch_release": (C.c_int, [_vp]),
    "okkt_factor_schur_batch": (C.c_int, [_vp, C.c_int64, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia),
                                          C.POINTER(C.c_int32)]),
    "okkt_factor_schur_batch_dev": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _f64p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia),
                                              C.POINTER(C.c_int32)]),
    "okkt_schur_batch_get": (C.c_int, [_vp, C.c_int64, _f64p, C.c_int64]),
    "okkt_schur_batch_get_dev": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64]),
    "okkt_schur_batch_factor": (C.c_int, [_vp, _f64p, C.c_int64, C.POINTER(OkktInertia), C.POINTER(OkktInertia)]),
    "okkt_schur_batch_factor_dev": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(OkktInertia), C.POINTER(OkktInertia)]),
    "okkt_schur_batch_condense": (C.c_int, [_vp, C.c_int64, _f64p, _f64p, _f64p, C.c_int64]),
    "okkt_schur_batch_condense_dev": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int64]),
    "okkt_schur_batch_expand": (C.c_int, [_vp, C.c_int64, _f64p, _f64p, _f64p, C.c_int64]),
    "okkt_schur_batch_expand_dev": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int64]),
    "okkt_schur_batch_solve": (C.c_int, [_vp, C.c_int64, _f64p, _f64p, _f64p, C.c_int64]),
    "okkt_schur_batch_solve_dev": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int64]),
    "okkt_schur_batch_select": (C.c_int, [_vp, C.c_int64]),
    "okkt_set_scaling": (C.c_int, [_vp, C.c_int, C.c_int32, _f64p]),
    "okkt_get_scaling": (C.c_int, [_vp, _f64p, C.POINTER(OkktScalingInfo)]),
    "okkt_get_scaling_dev": (C.c_int, [_vp, _vp]),
    "okkt_get_diag": (C.c_int, [_vp, _f64p]),
    "okkt_get_factor_csc": (C.c_int, [_vp, _i64p, _i64p, _f64p, _i64p]),
    "okkt_dev_alloc": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    "okkt_dev_free": (C.c_int, [_vp, _vp]),
    "okkt_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "okkt_get_stream": (_vp, [_vp]),
    "okkt_profile_dominant": (C.c_int, [_vp, C.c_int]),
    "okkt_get_profile": (C.c_int, [_vp, _i64p, _f64p, _f64p]),
    "okkt_debug_dataflow_queue": (C.c_int64, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64, _f64p]),
    "okkt_debug_dataflow_fragment": (C.c_int64, [C.c_int32] * 6),
    "okkt_dist_set_partition": (C.c_int, [_vp, C.c_int, C.c_int]),
    "okkt_dist_info": (C.c_int, [_vp, _i64p, _i64p, _i64p, _f64p, _f64p]),
    "okkt_dist_get_owner": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "okkt_dist_factor_local": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int]),
    "okkt_dist_cb": (C.c_int, [_vp, _vp, C.c_int]),
    "okkt_dist_factor_top": (C.c_int, [_vp]),
    "okkt_dist_counts": (C.c_int, [_vp, _i64p]),
    "okkt_dist_finish": (C.c_int, [_vp, _i64p]),
    "okkt_dist_solve_begin": (C.c_int, [_vp, _vp]),
    "okkt_dist_cv": (C.c_int, [_vp, _vp, C.c_int]),
    "okkt_dist_solve_top": (C.c_int, [_vp]),
    "okkt_dist_x": (C.c_int, [_vp, _vp, C.c_int]),
    "okkt_dist_solve_end": (C.c_int, [_vp]),
    "okkt_dist_unique_id": (C.c_int, [_vp]),
    "okkt_dist_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "okkt_dist_comm_destroy": (C.c_int, [_vp]),
    "okkt_dist_factor": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, C.POINTER(OkktInertia)]),
    "okkt_dist_solve": (C.c_int, [_vp, _vp, _vp]),
    "okkt_kkt_default_pars": (C.c_int, [C.POINTER(OkktKktPars)]),
    "okkt_kkt_create": (C.c_int, [C.POINTER(_vp), C.POINTER(OkktOpts), C.c_int]),
    "okkt_kkt_destroy": (C.c_int, [_vp]),
    "okkt_kkt_last_error": (C.c_char_p, [_vp]),
    "okkt_kkt_linear_solver": (_vp, [_vp]),
    "okkt_kkt_set_structure": (C.c_int, [_vp, C.c_int64, C.c_int64, _i64p, _i64p, _i64p, _i64p, C.c_int]),
    "okkt_kkt_form_system": (C.c_int, [_vp, _f64p, _f64p, _f64p, _f64p]),
    "okkt_kkt_diag_min": (C.c_int, [_vp, _f64p]),
    "okkt_kkt_factor": (C.c_int, [_vp, C.c_double, C.POINTER(OkktInertia)]),
    "okkt_kkt_factor_trial": (C.c_int, [_vp, C.c_double, C.POINTER(OkktInertia)]),
    "okkt_kkt_get_timers": (C.c_int, [_vp, C.POINTER(OkktKktTimers)]),
    "okkt_kkt_get_direction": (C.c_int, [_vp, _f64p, _f64p, _f64p]),
    "okkt_kkt_ipopt_strategy": (C.c_int, [_vp, C.c_double, C.POINTER(OkktKktPars), C.POINTER(C.c_int32), _f64p]),
    "okkt_kkt_min_eig": (C.c_int, [_vp, C.c_int32, C.c_double, C.c_int32, C.POINTER(OkktKktEigInfo), _f64p]),
    "okkt_kkt_ipopt_strategy_batch": (C.c_int, [_vp, C.c_double, C.POINTER(OkktKktPars), C.c_int32, C.POINTER(C.c_int32), _f64p,
                                                 C.POINTER(C.c_int32)]),
    "okkt_kkt_ipopt_strategy_eig": (C.c_int, [_vp, C.c_double, C.POINTER(OkktKktPars), C.c_int32, C.c_int32, C.POINTER(C.c_int32), _f64p,
                                              C.POINTER(C.c_int32), C.POINTER(OkktKktEigInfo)]),
    "okkt_kkt_items_query": (C.c_int, [_vp, C.POINTER(OkktKktItemsInfo)]),
    "okkt_kkt_items_reserve": (C.c_int, [_vp, C.c_int64]),
    "okkt_kkt_items_release": (C.c_int, [_vp]),
    "okkt_kkt_items_form_system": (C.c_int, [_vp, C.c_int64, _f64p, C.c_int64, _f64p, C.c_int64, _f64p, _f64p]),
    "okkt_kkt_items_diag_min": (C.c_int, [_vp, C.c_int64, _f64p]),
    "okkt_kkt_items_factor": (C.c_int, [_vp, C.c_int64, _f64p, C.POINTER(OkktInertia), C.POINTER(C.c_int32)]),
    "okkt_kkt_items_ipopt_strategy": (C.c_int, [_vp, C.c_int64, _f64p, C.POINTER(OkktKktPars), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _f64p,
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "okkt_kkt_items_system_rhs": (C.c_int, [_vp, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, C.c_double, C.c_double, C.c_double,
                                             _f64p, _f64p, _f64p]),
    "okkt_kkt_items_compute_direction": (C.c_int, [_vp, C.c_int64, C.c_int32, _f64p, _f64p, _f64p, C.POINTER(OkktKktError)]),
    "okkt_kkt_items_select": (C.c_int, [_vp, C.c_int64]),
    "okkt_kkt_items_set_direction": (C.c_int, [_vp, C.c_int64, _f64p, _f64p, _f64p]),
    "okkt_kkt_items_max_step_primal": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f64p, C.c_int64, C.c_double, _f64p, _f64p]),
    "okkt_kkt_items_s_bound_ok": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f64p, _f64p, C.c_int64, C.c_double, C.POINTER(C.c_int32)]),
    "okkt_kkt_items_dual_step_range": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f64p, _f64p, _f64p, C.c_double, _f64p, C.c_int64,
                                                 _f64p, _f64p]),
    "okkt_kkt_items_predicted_reduction": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]),
    "okkt_kkt_items_dual_step": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f64p, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p,
                                           _f64p, _f64p, _f64p, _f64p, C.c_int, _f64p]),
    "okkt_kkt_items_ls_query": (C.c_int, [_vp, C.POINTER(OkktKktItemsLsInfo)]),
    "okkt_debug_kkt_items_factor_list": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f64p, C.POINTER(C.c_int32)]),
    "okkt_debug_items_loop_model": (C.c_int, [C.c_int64, _f64p, _f64p, _f64p, C.POINTER(OkktKktPars), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                               _f64p, C.POINTER(C.c_int32)]),
    "okkt_debug_tridiag_eig": (C.c_int, [C.c_int32, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]),
    "okkt_kkt_compute_directions": (C.c_int, [_vp, C.c_int32, _f64p, C.c_int32, _f64p, _f64p, _f64p, C.POINTER(OkktKktError)]),
    "okkt_kkt_is_diag_dom": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "okkt_kkt_diag_dom_warnings": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "okkt_kkt_estimate_y_tilde": (C.c_int, [_vp, _f64p, _f64p]),
    "okkt_kkt_system_rhs": (C.c_int, [_vp, _f64p, _f64p, _f64p, _f64p, _f64p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _f64p, _f64p, _f64p]),
    "okkt_kkt_compute_direction": (C.c_int, [_vp, _f64p, _f64p, _f64p, C.c_int32, _f64p, _f64p, _f64p, C.POINTER(OkktKktError)]),
    "okkt_kkt_get_matrix": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i64p, _f64p]),
    "okkt_kkt_get_schur_diag": (C.c_int, [_vp, _f64p]),
    "okkt_kkt_get_dense_rows": (C.c_int, [_vp, _i64p, _i64p]),
    "okkt_kkt_set_ls_refine": (C.c_int, [_vp, C.c_int32, C.c_double]),
    "okkt_kkt_set_ls_scaling": (C.c_int, [_vp, C.c_int, C.c_int32]),
    "okkt_kkt_condest": (C.c_int, [_vp, C.c_int32, C.POINTER(OkktCondestInfo)]),
    "okkt_kkt_direction_error_bound": (C.c_int, [_vp, _f64p]),
    "okkt_eigs": (C.c_int, [_vp, C.POINTER(OkktEigsOpts), _f64p, _f64p, _f64p, _f64p, C.POINTER(OkktEigsInfo)]),
    "okkt_eigs_dev": (C.c_int, [_vp, C.POINTER(OkktEigsOpts), _vp, _f64p, _vp, _f64p, C.POINTER(OkktEigsInfo)]),
    "okkt_kkt_eigs": (C.c_int, [_vp, C.POINTER(OkktEigsOpts), _f64p, _f64p, _f64p, C.POINTER(OkktEigsInfo)]),
    "okkt_debug_sym_eig": (C.c_int, [C.c_int32, _f64p, _f64p, _f64p]),
    "okkt_kkt_compute_indicies": (C.c_int, [_vp, _f64p, C.POINTER(C.c_int64)]),
    "okkt_kkt_get_indicies": (C.c_int, [_vp, _i64p, _i64p, _i64p, _f64p, _f64p, _f64p, _f64p]),
    "okkt_kkt_get_clever_vectors": (C.c_int, [_vp, _f64p, _f64p, _f64p, _f64p, _f64p]),
    "okkt_kkt_set_rescale": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "okkt_kkt_set_direction": (C.c_int, [_vp, _f64p, _f64p, _f64p]),
    "okkt_kkt_max_step_primal": (C.c_int, [_vp, _f64p, C.c_double, _f64p, _f64p]),
    "okkt_kkt_s_bound_ok": (C.c_int, [_vp, _f64p, _f64p, C.c_double, C.POINTER(C.c_int32)]),
    "okkt_kkt_dual_step_range": (C.c_int, [_vp, _f64p, _f64p, C.c_double, C.c_double, _f64p, _f64p, _f64p]),
    "okkt_kkt_predicted_reduction": (C.c_int, [_vp, _f64p, C.c_double, C.c_double, C.c_double, C.c_double, _f64p]),
    "okkt_kkt_dual_step": (C.c_int, [_vp, _f64p, _f64p, _f64p, _f64p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.c_int, C.c_double, C.c_double, _f64p]),
}

_lib = None
MISSING = []


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the KKT path."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:  # reported by tests/test_abi.py; calling it raises AttributeError
            MISSING.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def p_i64(a):
    return a.ctypes.data_as(_i64p)


def p_f64(a):
    return a.ctypes.data_as(_f64p)
