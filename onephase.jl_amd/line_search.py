"""Host-side mirror of the step-side functions of the reference's line search, bound to the HIP library.

Mirrors /root/reference/src/line_search/frac_boundary.jl (lb_s_predict + simple_max_step as used by simple_ls,
line_search.jl:40-41), move.jl (the s-bound test of move_primal :15-17, dual_bounds :28-80, move_dual's step size
:82-118) and src/utils/eval.jl:236-273 (merit_function_predicted_reduction and its parts).  `iter` is always the
iterate the KKT solver was formed at (`kkt_solver.factor_it`) and `dir` the direction of its last
compute_direction_b: both are already resident on the device, so the functions take the KKT solver where the
reference takes (iter, dir).  Everything numeric happens in libonephase_kkt.so (okkt_kkt_max_step_primal, ...);
there is no host fallback.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .kkt_system_solver import _csc
from .linear_system_solvers import OkktError


@dataclass
class Class_ls_parameters:      # parameters.jl:50-105 (the entries these functions read)
    fraction_to_boundary_predict_exp: float = 0.5
    comp_feas: float = 1.0 / 100.0
    move_primal_seperate_to_dual: bool = True
    dual_ls: int = 1


def _need_dir(kkt_solver):
    if kkt_solver.factor_it is None or kkt_solver.dir.x is None:
        raise OkktError("no direction: form_system_b / factor_b / compute_direction_b first")


def set_direction(kkt_solver, dir):
    """Make `dir` the resident direction (scale_direction, line_search.jl:10-19; corrections): kkt_solver.dir follows."""
    if kkt_solver.factor_it is None:
        raise OkktError("form_system_b first")
    dx, dy, ds = L.f64(dir.x), L.f64(dir.y), L.f64(dir.s)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_set_direction(kkt_solver._k, L.p_f64(dx), L.p_f64(dy), L.p_f64(ds)), "okkt_kkt_set_direction")
    kkt_solver.dir.x, kkt_solver.dir.y, kkt_solver.dir.s = dx.copy(), dy.copy(), ds.copy()
    kkt_solver.dir.mu, kkt_solver.dir.primal_scale = dir.mu, dir.primal_scale


def max_step_primal(kkt_solver, frac_bd_predict, pars=None):
    """step_size_P = simple_max_step(iter.point.s, dir.s, lb_s_predict(iter, dir, pars)) (line_search.jl:40-41).
    Returns (step_size_P, norm(dir.x, Inf))."""
    pars = pars or Class_ls_parameters()
    _need_dir(kkt_solver)
    step, nx = C.c_double(), C.c_double()
    f = L.f64(frac_bd_predict)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_max_step_primal(kkt_solver._k, L.p_f64(f), pars.fraction_to_boundary_predict_exp,
                                                               C.byref(step), C.byref(nx)), "okkt_kkt_max_step_primal")
    return step.value, nx.value


def s_bound_ok(kkt_solver, s_new, frac_bd, pars=None):
    """all(new_it.point.s .>= lb_s(it, dir, pars)) -- move_primal's :s_bound test (move.jl:15-17)."""
    pars = pars or Class_ls_parameters()
    _need_dir(kkt_solver)
    ok = C.c_int32()
    s_new, f = L.f64(s_new), L.f64(frac_bd)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_s_bound_ok(kkt_solver._k, L.p_f64(s_new), L.p_f64(f), pars.fraction_to_boundary_predict_exp,
                                                          C.byref(ok)), "okkt_kkt_s_bound_ok")
    return bool(ok.value)


def dual_step_range(kkt_solver, candidate, frac_bd, pars=None):
    """lb, ub = dual_bounds(candidate, candidate.point.y, dir.y, comp_feas); ub = min(ub, simple_max_step(candidate.point.y,
    dir.y, lb_y(iter, dir, pars))) (line_search.jl:84-86)."""
    pars = pars or Class_ls_parameters()
    _need_dir(kkt_solver)
    lb, ub = C.c_double(), C.c_double()
    s, y, f = L.f64(candidate.s), L.f64(candidate.y), L.f64(frac_bd)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_dual_step_range(kkt_solver._k, L.p_f64(s), L.p_f64(y), float(candidate.mu), pars.comp_feas,
                                                               L.p_f64(f), C.byref(lb), C.byref(ub)), "okkt_kkt_dual_step_range")
    return lb.value, ub.value


def predicted_reduction_terms(kkt_solver, step_size):
    """(phi_predicted_reduction_primal_dual, norm(comp(iter), Inf), norm(comp_predicted(iter, dir, step_size), Inf),
    merit_function_predicted_reduction) (eval.jl:236-273)."""
    _need_dir(kkt_solver)
    it = kkt_solver.factor_it
    out = np.zeros(4)
    g = L.f64(it.grad)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_predicted_reduction(kkt_solver._k, L.p_f64(g), float(it.mu), float(kkt_solver.dir.mu),
                                                                   float(it.a_norm_penalty_par), float(step_size), L.p_f64(out)),
                      "okkt_kkt_predicted_reduction")
    return tuple(float(v) for v in out)


def merit_function_predicted_reduction(kkt_solver, step_size):   # eval.jl:257-273
    return predicted_reduction_terms(kkt_solver, step_size)[3]


def phi_predicted_reduction_primal_dual(kkt_solver, step_size):  # eval.jl:236-249
    return predicted_reduction_terms(kkt_solver, step_size)[0]


def move_dual_step(kkt_solver, new_it, step_size_P, lb, ub, scale_D, scale_mu, pars=None):
    """step_size_D of move_dual (move.jl:82-118); new_it = the candidate with J and grad re-evaluated, y not yet moved."""
    pars = pars or Class_ls_parameters()
    _need_dir(kkt_solver)
    if not pars.move_primal_seperate_to_dual:
        return float(step_size_P)
    if pars.dual_ls == 2:
        raise OkktError("dual_ls == 2 evaluates the KKT error at trial points on the host (eval_kkt_err): not a device function")
    Jx = None if new_it is kkt_solver.factor_it else L.f64(_csc(new_it.J).data)
    g, s, y = L.f64(new_it.grad), L.f64(new_it.s), L.f64(new_it.y)
    out = C.c_double()
    kkt_solver._check(kkt_solver._lib.okkt_kkt_dual_step(kkt_solver._k, L.p_f64(Jx) if Jx is not None else None, L.p_f64(g), L.p_f64(s), L.p_f64(y),
                                                         float(new_it.mu), float(new_it.a_norm_penalty_par), float(step_size_P), float(lb),
                                                         float(ub), int(pars.dual_ls), float(scale_D), float(scale_mu), C.byref(out)),
                      "okkt_kkt_dual_step")
    return out.value


# ---- line-search batches (okkt_kkt_items_*): the same functions for the items of a KKT batch.  The iterates are
# those of form_system_items, the directions those of compute_direction_items or set_direction_items; item b's numbers are bit for bit
# what the functions above return for that iterate and direction on a solver of its own.  `items` (None: every item) lists the slots
# a call covers: inputs and outputs stay indexed by slot, an unlisted slot's output is NaN (-1 for s_bound_ok_items).
_i32p = C.POINTER(C.c_int32)


def _need_dir_items(kkt_solver):
    B = getattr(kkt_solver, "_items_dir_B", 0)
    if not getattr(kkt_solver, "_items_B", 0) or not B:
        raise OkktError("no direction: form_system_items / compute_direction_items (or set_direction_items) first")
    return B


def _item_list(items):
    if items is None:
        return None, 0, None
    a = np.ascontiguousarray(items, dtype=np.int32)
    return a.ctypes.data_as(_i32p), len(a), a


def _rows(a, B, width, what):
    a = L.f64(np.stack([np.asarray(v, dtype=float) for v in a]) if isinstance(a, (list, tuple)) else a)
    if a.shape != (B, width):
        raise OkktError(f"{what}: one row of {width} entries per item")
    return a


def _frac(frac, B, m):
    """One fraction vector for every item (stride 0) or one per item."""
    f = L.f64(frac)
    if f.shape == (m,):
        return f, 0
    if f.shape != (B, m):
        raise OkktError("frac: a vector of m entries or [B][m]")
    return f, m


def _per_item(v, B):
    a = L.f64(np.full(B, float(v)) if np.ndim(v) == 0 else v)
    if a.shape != (B,):
        raise OkktError("one scalar per item")
    return a


def set_direction_items(kkt_solver, dirs):
    """Make dirs[b] the resident direction of item b, for the first len(dirs) items of the last form_system_items."""
    if not getattr(kkt_solver, "_items_B", 0):
        raise OkktError("form_system_items first")
    its = kkt_solver._items_its
    B, n, m = len(dirs), its[0].dim(), its[0].ncon()
    dx = _rows([d.x for d in dirs], B, n, "dx")
    dy, ds = _rows([d.y for d in dirs], B, m, "dy"), _rows([d.s for d in dirs], B, m, "ds")
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_set_direction(kkt_solver._k, B, L.p_f64(dx), L.p_f64(dy), L.p_f64(ds)), "okkt_kkt_items_set_direction")
    kkt_solver._items_dir_B = B
    kkt_solver._items_dirs = list(dirs)
    kkt_solver._items_dir_mu = [float(d.mu) for d in dirs]


def max_step_primal_items(kkt_solver, frac_bd_predict, pars=None, items=None):
    """(step_size_P [B], norm(dir_b.x, Inf) [B])."""
    pars = pars or Class_ls_parameters()
    B = _need_dir_items(kkt_solver)
    m = kkt_solver._items_its[0].ncon()
    f, fs = _frac(frac_bd_predict, B, m)
    ip, ni, _keep = _item_list(items)
    step, nx = np.full(B, np.nan), np.full(B, np.nan)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_max_step_primal(kkt_solver._k, B, ip, ni, L.p_f64(f), fs, pars.fraction_to_boundary_predict_exp,
                                                                     L.p_f64(step), L.p_f64(nx)), "okkt_kkt_items_max_step_primal")
    return step, nx


def s_bound_ok_items(kkt_solver, s_new, frac_bd, pars=None, items=None):
    """[B] int32: 1 / 0 per listed item (-1: not listed)."""
    pars = pars or Class_ls_parameters()
    B = _need_dir_items(kkt_solver)
    m = kkt_solver._items_its[0].ncon()
    f, fs = _frac(frac_bd, B, m)
    s_new = _rows(s_new, B, m, "s_new")
    ip, ni, _keep = _item_list(items)
    ok = np.full(B, -1, dtype=np.int32)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_s_bound_ok(kkt_solver._k, B, ip, ni, L.p_f64(s_new), L.p_f64(f), fs, pars.fraction_to_boundary_predict_exp,
                                                                ok.ctypes.data_as(_i32p)), "okkt_kkt_items_s_bound_ok")
    return ok


def dual_step_range_items(kkt_solver, candidates, frac_bd, pars=None, items=None):
    """(lb [B], ub [B]) for the candidates (objects with s, y, mu), one per item."""
    pars = pars or Class_ls_parameters()
    B = _need_dir_items(kkt_solver)
    m = kkt_solver._items_its[0].ncon()
    f, fs = _frac(frac_bd, B, m)
    s, y = _rows([c.s for c in candidates], B, m, "s_cand"), _rows([c.y for c in candidates], B, m, "y_cand")
    mu = _per_item([float(c.mu) for c in candidates], B)
    ip, ni, _keep = _item_list(items)
    lb, ub = np.full(B, np.nan), np.full(B, np.nan)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_dual_step_range(kkt_solver._k, B, ip, ni, L.p_f64(s), L.p_f64(y), L.p_f64(mu), pars.comp_feas, L.p_f64(f), fs,
                                                                     L.p_f64(lb), L.p_f64(ub)), "okkt_kkt_items_dual_step_range")
    return lb, ub


def predicted_reduction_terms_items(kkt_solver, step_sizes, items=None):
    """[B][4]: the four numbers of predicted_reduction_terms per item, at step_sizes (a scalar or [B])."""
    B = _need_dir_items(kkt_solver)
    its = kkt_solver._items_its[:B]
    n = its[0].dim()
    grad = _rows([it.grad for it in its], B, n, "grad")
    mu = _per_item([float(it.mu) for it in its], B)
    dmu = _per_item(kkt_solver._items_dir_mu[:B], B)
    pen = _per_item([float(it.a_norm_penalty_par) for it in its], B)
    step = _per_item(step_sizes, B)
    ip, ni, _keep = _item_list(items)
    out = np.full((B, 4), np.nan)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_predicted_reduction(kkt_solver._k, B, ip, ni, L.p_f64(grad), L.p_f64(mu), L.p_f64(dmu), L.p_f64(pen),
                                                                         L.p_f64(step), L.p_f64(out)), "okkt_kkt_items_predicted_reduction")
    return out


def move_dual_step_items(kkt_solver, new_its, step_size_P, lb, ub, scale_D, scale_mu, pars=None, items=None):
    """step_size_D [B] of move_dual; new_its[b] = item b's candidate with J and grad re-evaluated, y not yet moved.  Candidates that are
    the formed iterates themselves read the resident J; one J object shared by all candidates goes in once."""
    pars = pars or Class_ls_parameters()
    B = _need_dir_items(kkt_solver)
    if not pars.move_primal_seperate_to_dual:
        return _per_item(step_size_P, B).copy()
    if pars.dual_ls == 2:
        raise OkktError("dual_ls == 2 evaluates the KKT error at trial points on the host (eval_kkt_err): not a device function")
    its = kkt_solver._items_its[:B]
    n, m = its[0].dim(), its[0].ncon()
    if all(c is it for c, it in zip(new_its, its)):
        Jx, js = None, 0
    elif all(c.J is new_its[0].J for c in new_its):
        Jx, js = L.f64(_csc(new_its[0].J).data), 0
    else:
        Jx = L.f64(np.stack([_csc(c.J).data for c in new_its]))
        js = Jx.shape[1]
    g = _rows([c.grad for c in new_its], B, n, "grad_cand")
    s, y = _rows([c.s for c in new_its], B, m, "s_cand"), _rows([c.y for c in new_its], B, m, "y_cand")
    mu = _per_item([float(c.mu) for c in new_its], B)
    pen = _per_item([float(c.a_norm_penalty_par) for c in new_its], B)
    sP, lb, ub, sD, sM = (_per_item(v, B) for v in (step_size_P, lb, ub, scale_D, scale_mu))
    ip, ni, _keep = _item_list(items)
    out = np.full(B, np.nan)
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_dual_step(kkt_solver._k, B, ip, ni, L.p_f64(Jx) if Jx is not None else None, js, L.p_f64(g), L.p_f64(s),
                                                               L.p_f64(y), L.p_f64(mu), L.p_f64(pen), L.p_f64(sP), L.p_f64(lb), L.p_f64(ub), L.p_f64(sD),
                                                               L.p_f64(sM), int(pars.dual_ls), L.p_f64(out)), "okkt_kkt_items_dual_step")
    return out


def items_ls_query(kkt_solver):
    """okkt_kkt_items_ls_query as a dict (host only)."""
    if kkt_solver._k is None:
        raise OkktError("initialize_b has not been called")
    info = L.OkktKktItemsLsInfo()
    kkt_solver._check(kkt_solver._lib.okkt_kkt_items_ls_query(kkt_solver._k, C.byref(info)), "okkt_kkt_items_ls_query")
    return info.as_dict()
