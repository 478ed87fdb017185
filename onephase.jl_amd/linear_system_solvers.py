"""Host-side mirror of the reference's linear-solver plug-in interface, bound to the HIP library.

Mirrors /root/reference/src/linear_system_solvers/linear_system_solvers.jl (abstract type,
initialize!/finalize!, inertia_status) and the back-end pattern of hsl.jl / julia.jl
(`X(sym, safe_mode, recycle)`, ls_factor!, ls_solve!, ls_solve).  Julia's `f!` becomes `f_b`
("bang") here; argument order and meaning are the reference's.  The Julia glue a maintainer
would add is julia/linear_solver_hip.jl; this Python class calls the same C ABI through ctypes
so that the parity tests can read like test/linear_system_solvers.jl.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib as L


class OkktError(RuntimeError):
    pass


class abstract_linear_system_solver:  # linear_system_solvers.jl:11
    pass


def initialize_b(solver):  # linear_system_solvers.jl:40
    solver._initialize()


def finalize_b(solver):  # linear_system_solvers.jl:44
    solver._finalize()


def inertia_status(pos_eigs, neg_eigs, zero_eigs, num_vars, num_constraints):
    """linear_system_solvers.jl:48-91 -- is the inertia (num_vars, num_constraints, 0)?"""
    if pos_eigs + neg_eigs + zero_eigs != num_vars + num_constraints:
        raise OkktError("pos_eigs + neg_eigs + zero_eigs != num_vars + num_constraints")
    return pos_eigs == num_vars and neg_eigs == num_constraints


def csc_arrays(A):
    """(dim, colptr, rowval, nzval, index_base) of a square sparse matrix, SparseMatrixCSC-like."""
    if isinstance(A, tuple):
        dim, colptr, rowval, nzval, base = A
        return int(dim), L.i64(colptr), L.i64(rowval), L.f64(nzval), int(base)
    A = sp.csc_matrix(A)
    if A.shape[0] != A.shape[1]:
        raise OkktError("matrix must be square")
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    return A.shape[0], L.i64(A.indptr), L.i64(A.indices), L.f64(A.data), 0


class linear_solver_HIP(abstract_linear_system_solver):
    """`linear_solver_HIP(sym, safe_mode, recycle)` -- constructor shape of julia.jl:11 / hsl.jl:17."""

    def __init__(self, sym, safe_mode=False, recycle=False, **opts):
        if sym not in ("definite", "symmetric"):
            # julia.jl:95: error("this.options.sym = ... not supported")
            raise OkktError(f"this.options.sym = {sym} not supported")
        self.sym = sym
        self.safe_mode = safe_mode
        self.recycle = recycle
        self._opts = opts
        self._h = None
        self._lib = None
        self.inertia = None  # (pos, neg, zero, nonfinite) of the last factorisation
        self._dim = 0
        self._ns = 0  # Schur set size (set_schur)
        self.schur_inertia = None  # counts over D of the last schur_factor
        self.total_inertia = None  # A11's counts + S's: the whole matrix's
        self._borrowed = False  # a view on a handle another object owns (of_kkt): finalize does not destroy it
        self._scale_mode = L.OKKT_SCALE_NONE  # the mode of the last set_scaling (ls_factor_robust refuses scaled handles)
        self._robust_mode = None  # "plain" | "schur": the mode the last ls_factor_robust ended in

    # -- initialize! / finalize!
    def _initialize(self):
        if self._h is not None:
            return
        self._lib = L.load()
        o = L.OkktOpts()
        self._lib.okkt_default_opts(C.byref(o))
        for k, v in self._opts.items():
            if not hasattr(o, k):
                raise OkktError(f"unknown option {k}")
            setattr(o, k, v)
        h = C.c_void_p()
        rc = self._lib.okkt_create(C.byref(h), C.byref(o))
        if rc != L.OKKT_OK:
            raise OkktError(
                f"okkt_create failed with code {rc}"
                + (" (no HIP device: the KKT path has no CPU fallback)" if rc == L.OKKT_ERR_NO_DEVICE else "")
            )
        self._h = h

    def _finalize(self):
        if self._h is not None:
            if not self._borrowed:
                self._lib.okkt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._finalize()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            msg = self._lib.okkt_last_error(self._h)
            raise OkktError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        return rc

    def _need(self):
        if self._h is None:
            raise OkktError("initialize_b(solver) has not been called")

    # -- analysis helpers (not part of the reference interface)
    def set_perm(self, perm):
        self._need()
        p = L.i64(perm)
        self._check(self._lib.okkt_set_perm(self._h, L.p_i64(p), len(p)), "okkt_set_perm")

    def analyze(self, A):
        self._need()
        dim, colptr, rowval, _, base = csc_arrays(A)
        self._check(self._lib.okkt_analyze(self._h, dim, L.p_i64(colptr), L.p_i64(rowval), base), "okkt_analyze")
        self._dim = dim

    def perm(self):
        out = np.zeros(self._dim, dtype=np.int64)
        self._check(self._lib.okkt_get_perm(self._h, L.p_i64(out)), "okkt_get_perm")
        return out

    def etree(self):
        par = np.zeros(self._dim, dtype=np.int64)
        cnt = np.zeros(self._dim, dtype=np.int64)
        self._check(self._lib.okkt_get_etree(self._h, L.p_i64(par), L.p_i64(cnt)), "okkt_get_etree")
        return par, cnt

    def stats(self):
        st = L.OkktStats()
        self._check(self._lib.okkt_get_stats(self._h, C.byref(st)), "okkt_get_stats")
        return st.as_dict()

    def diag(self):
        """diag(F) (julia.jl:72): D in pivot order."""
        out = np.zeros(self._dim)
        self._check(self._lib.okkt_get_diag(self._h, L.p_f64(out)), "okkt_get_diag")
        return out

    def factor_csc(self):
        """L (strictly lower, permuted numbering) as scipy CSC -- parity tests only."""
        nnz = C.c_int64()
        self._check(self._lib.okkt_get_factor_csc(self._h, None, None, None, C.byref(nnz)), "okkt_get_factor_csc")
        colptr = np.zeros(self._dim + 1, dtype=np.int64)
        rowval = np.zeros(max(nnz.value, 1), dtype=np.int64)
        val = np.zeros(max(nnz.value, 1))
        self._check(self._lib.okkt_get_factor_csc(self._h, L.p_i64(colptr), L.p_i64(rowval), L.p_f64(val), C.byref(nnz)),
                    "okkt_get_factor_csc")
        return sp.csc_matrix((val[: nnz.value], rowval[: nnz.value], colptr), shape=(self._dim, self._dim))

    # -- device-resident variants: inputs already in HBM (bench.py, the KKT layer)
    def dev_upload(self, arr):
        """Copy a contiguous numpy array into a fresh HBM buffer; returns the device pointer (int)."""
        self._need()
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        self._check(self._lib.okkt_dev_alloc(self._h, arr.nbytes, C.byref(p)), "okkt_dev_alloc")
        self._check(self._lib.okkt_dev_upload(self._h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "okkt_dev_upload")
        return p.value

    def dev_alloc(self, nbytes):
        self._need()
        p = C.c_void_p()
        self._check(self._lib.okkt_dev_alloc(self._h, nbytes, C.byref(p)), "okkt_dev_alloc")
        return p.value

    def dev_download(self, ptr, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        self._check(self._lib.okkt_dev_download(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes), "okkt_dev_download")
        return out

    def dev_free(self, ptr):
        self._check(self._lib.okkt_dev_free(self._h, C.c_void_p(ptr)), "okkt_dev_free")

    def ls_factor_dev(self, d_nzval, n, m):
        """ls_factor! with nzval resident in HBM (pattern analysed beforehand with analyze())."""
        self._need()
        inert = L.OkktInertia()
        kind = L.OKKT_SYM_DEFINITE if self.sym == "definite" else L.OKKT_SYM_SYMMETRIC
        rc = self._check(self._lib.okkt_factor_dev(self._h, C.c_void_p(d_nzval), n, m, kind, C.byref(inert)), "okkt_factor_dev")
        self.inertia = inert.as_tuple()
        return int(rc)

    def ls_solve_dev(self, d_rhs, d_sol, nrhs=1):
        self._need()
        self._check(self._lib.okkt_solve_dev(self._h, C.c_void_p(d_rhs), C.c_void_p(d_sol), nrhs), "okkt_solve_dev")

    def ls_solve_refine_dev(self, d_nzval, d_rhs, d_sol, nrhs=1, max_steps=3, tol=0.0):
        """ls_solve_refine with every array resident in HBM (device pointers); returns (info dict, omega per rhs)."""
        self._need()
        info = L.OkktRefineInfo()
        om = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_solve_refine_dev(self._h, C.c_void_p(d_nzval), C.c_void_p(d_rhs), C.c_void_p(d_sol), int(nrhs),
                                                     int(max_steps), float(tol), C.byref(info), L.p_f64(om)), "okkt_solve_refine_dev")
        return info.as_dict(), om[:nrhs]

    def residual_dev(self, d_nzval, d_rhs, d_x, d_r, nrhs=1):
        """r = b - A x (double-double, rounded once) with device pointers; returns omega per rhs."""
        self._need()
        om = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_residual_dev(self._h, C.c_void_p(d_nzval), C.c_void_p(d_rhs), C.c_void_p(d_x), C.c_void_p(d_r),
                                                 int(nrhs), L.p_f64(om)), "okkt_residual_dev")
        return om[:nrhs]

    def profile_dominant(self, enable):
        self._check(self._lib.okkt_profile_dominant(self._h, 1 if enable else 0), "okkt_profile_dominant")

    def get_profile(self):
        n = C.c_int64(); ms = C.c_double(); fl = C.c_double()
        self._check(self._lib.okkt_get_profile(self._h, C.byref(n), C.byref(ms), C.byref(fl)), "okkt_get_profile")
        return n.value, ms.value, fl.value

    # -- the reference interface
    def ls_factor_b(self, SparseMatrix, n, m, timer=None):
        """ls_factor!(solver, A, n, m, timer) -> 1 if the inertia is (n, m, 0), else 0 (julia.jl:21-97)."""
        self._need()
        dim, colptr, rowval, nzval, base = csc_arrays(SparseMatrix)
        if timer is not None:
            timer.start("HIP/factorize")
        try:
            self._check(self._lib.okkt_analyze(self._h, dim, L.p_i64(colptr), L.p_i64(rowval), base), "okkt_analyze")
            self._dim = dim
            inert = L.OkktInertia()
            kind = L.OKKT_SYM_DEFINITE if self.sym == "definite" else L.OKKT_SYM_SYMMETRIC
            rc = self._check(self._lib.okkt_factor(self._h, L.p_f64(nzval), n, m, kind, C.byref(inert)), "okkt_factor")
            self.inertia = inert.as_tuple()
        finally:
            if timer is not None:
                timer.pause("HIP/factorize")
        return int(rc)

    def ls_solve_b(self, my_rhs, my_sol, timer=None):
        """ls_solve!(solver, rhs, sol, timer): sol[1:end] = F \\ rhs (julia.jl:99-103)."""
        self._need()
        rhs = L.f64(my_rhs)
        if rhs.shape != (self._dim,) or my_sol.shape != (self._dim,) or my_sol.dtype != np.float64:
            raise OkktError("rhs/sol must be float64 vectors of the factorised dimension")
        if timer is not None:
            timer.start("HIP/ls_solve")
        try:
            out = np.empty(self._dim)
            self._check(self._lib.okkt_solve(self._h, L.p_f64(rhs), L.p_f64(out), 1), "okkt_solve")
            my_sol[:] = out
        finally:
            if timer is not None:
                timer.pause("HIP/ls_solve")

    def ls_solve(self, my_rhs, timer=None):
        """ls_solve(solver, rhs, timer) -> F \\ Vector(rhs); sparse vectors are densified (julia.jl:105-113)."""
        if sp.issparse(my_rhs):
            my_rhs = np.asarray(my_rhs.todense()).ravel()
        sol = np.empty(self._dim)
        self.ls_solve_b(np.asarray(my_rhs, dtype=np.float64).ravel(), sol, timer)
        return sol

    # -- uniform batches: B systems on the analysed pattern (not part of the reference interface)
    def batch_query(self, nrhs_max=1):
        """Whether the analysed plan takes a batch, and what one costs: dict of okkt_batch_info (host only)."""
        self._need()
        info = L.OkktBatchInfo()
        self._check(self._lib.okkt_batch_query(self._h, int(nrhs_max), C.byref(info)), "okkt_batch_query")
        return info.as_dict()

    def batch_reserve(self, B, nrhs_max=1, mode=None):
        """Slots for B items with solve work for nrhs_max columns; mode: None (keep), "auto", "level" or "item"."""
        self._need()
        if mode is not None:
            self._check(self._lib.okkt_batch_set_mode(self._h, L.OKKT_BATCH_MODE[mode]), "okkt_batch_set_mode")
        self._check(self._lib.okkt_batch_reserve(self._h, int(B), int(nrhs_max)), "okkt_batch_reserve")

    def batch_release(self):
        self._need()
        self._check(self._lib.okkt_batch_release(self._h), "okkt_batch_release")

    def batch_mode_used(self):
        return {v: k for k, v in L.OKKT_BATCH_MODE.items()}.get(self._lib.okkt_batch_mode_used(self._h))

    def _batch_factor(self, fn, what, B, vals, stride, shifts, nshift, n, m):
        sh = None if shifts is None else L.f64(shifts).ravel()
        if sh is not None and sh.size != B:
            raise OkktError("shifts must have one entry per item")
        inert = (L.OkktInertia * B)()
        flags = np.zeros(B, dtype=np.int32)
        kind = L.OKKT_SYM_DEFINITE if self.sym == "definite" else L.OKKT_SYM_SYMMETRIC
        self._check(fn(self._h, B, vals, stride, None if sh is None else L.p_f64(sh), int(nshift), int(n), int(m), kind, inert,
                       flags.ctypes.data_as(C.POINTER(C.c_int32))), what)
        self.batch_inertia = [it.as_tuple() for it in inert]
        return flags

    def ls_factor_batch(self, vals, n, m, shifts=None, nshift=None, B=None):
        """Factor B value sets on the analysed pattern.  vals: [B, nnz] (one row per item), or [nnz] shared by all items together with
        shifts [B] (B may then be given instead of shifts).  shifts[b] is added to the first nshift (default n) diagonal entries.
        Returns the items' flags (1: inertia (n, m, 0)); the counts are left in self.batch_inertia."""
        self._need()
        v = L.f64(vals)
        if v.ndim == 1:
            B = int(B if B is not None else len(shifts))
            stride = 0
        else:
            B, stride = v.shape[0], v.shape[1]
        return self._batch_factor(self._lib.okkt_factor_batch, "okkt_factor_batch", B, L.p_f64(v), stride, shifts,
                                  n if nshift is None else nshift, n, m)

    def ls_factor_batch_dev(self, d_nzval, B, val_stride, n, m, shifts=None, nshift=None):
        self._need()
        return self._batch_factor(self._lib.okkt_factor_batch_dev, "okkt_factor_batch_dev", int(B), C.c_void_p(d_nzval), int(val_stride), shifts,
                                  n if nshift is None else nshift, n, m)

    def ls_solve_batch(self, rhs):
        """rhs [B, dim] or [B, nrhs, dim] -> the items' solutions, same shape."""
        self._need()
        b = L.f64(rhs)
        if b.ndim not in (2, 3) or b.shape[-1] != self._dim:
            raise OkktError("rhs must be [B, dim] or [B, nrhs, dim] of the analysed dimension")
        nrhs = 1 if b.ndim == 2 else b.shape[1]
        out = np.empty_like(b)
        self._check(self._lib.okkt_solve_batch(self._h, b.shape[0], L.p_f64(b), L.p_f64(out), nrhs), "okkt_solve_batch")
        return out

    def ls_solve_batch_dev(self, d_rhs, d_sol, B, nrhs=1):
        self._need()
        self._check(self._lib.okkt_solve_batch_dev(self._h, int(B), C.c_void_p(d_rhs), C.c_void_p(d_sol), int(nrhs)), "okkt_solve_batch_dev")

    def batch_select(self, b):
        """Slot b becomes the handle's own factor: every other call then behaves as after ls_factor of that item."""
        self._need()
        self._check(self._lib.okkt_batch_select(self._h, int(b)), "okkt_batch_select")
        if getattr(self, "batch_inertia", None) and 0 <= b < len(self.batch_inertia):
            self.inertia = self.batch_inertia[b]

    # -- refinement with extra-precise residuals (not part of the reference interface)
    def _values(self, nzval_or_matrix):
        if isinstance(nzval_or_matrix, np.ndarray) and nzval_or_matrix.ndim == 1:
            return L.f64(nzval_or_matrix)
        return csc_arrays(nzval_or_matrix)[3]

    @staticmethod
    def _rhs_block(rhs, dim):
        b = L.f64(rhs)
        single = b.ndim == 1
        B = L.f64(b.reshape(1, -1) if single else b)
        if B.shape[1] != dim:
            raise OkktError("rhs must have the factorised dimension (one right-hand side per row)")
        return B, single

    def ls_solve_refine(self, nzval_or_matrix, rhs, max_steps=3, tol=0.0):
        """x with at most max_steps corrections from double-double residuals against A (its values in the analysed order, or
        the matrix itself with the analysed pattern; the factor may be of a nearby matrix).  rhs: a vector or one right-hand
        side per row.  Returns (x, info) with info = okkt_refine_info as a dict plus "omega_per_rhs"."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        X = np.zeros_like(B)
        om = np.zeros(B.shape[0])
        info = L.OkktRefineInfo()
        self._check(self._lib.okkt_solve_refine(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(X), B.shape[0], int(max_steps), float(tol),
                                                 C.byref(info), L.p_f64(om)), "okkt_solve_refine")
        d = info.as_dict()
        d["omega_per_rhs"] = om
        return (X[0] if single else X), d

    def ls_solve_gmres(self, nzval_or_matrix, rhs, restart=30, max_iters=200, tol=0.0):
        """GMRES-based refinement (okkt_solve_gmres): x for A x = b with the held factor F ~ A as the
        preconditioner of GMRES(restart) cycles on the correction equation, the residual in double-double.  A as for ls_solve_refine
        (its values in the analysed order, or the matrix itself).  rhs: a vector or one right-hand side per row.  Returns (x, info)
        with info = okkt_gmres_info as a dict plus "omega_per_rhs"."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        X = np.zeros_like(B)
        om = np.zeros(B.shape[0])
        info = L.OkktGmresInfo()
        self._check(self._lib.okkt_solve_gmres(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(X), B.shape[0], int(restart), int(max_iters),
                                                float(tol), C.byref(info), L.p_f64(om)), "okkt_solve_gmres")
        d = info.as_dict()
        d["omega_per_rhs"] = om
        return (X[0] if single else X), d

    def ls_solve_gmres_dev(self, d_nzval, d_rhs, d_sol, nrhs=1, restart=30, max_iters=200, tol=0.0):
        """ls_solve_gmres with every array resident in HBM (device pointers); returns (info dict, omega per rhs)."""
        self._need()
        info = L.OkktGmresInfo()
        om = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_solve_gmres_dev(self._h, C.c_void_p(d_nzval), C.c_void_p(d_rhs), C.c_void_p(d_sol), int(nrhs),
                                                    int(restart), int(max_iters), float(tol), C.byref(info), L.p_f64(om)),
                    "okkt_solve_gmres_dev")
        return info.as_dict(), om[: int(nrhs)]

    def residual(self, nzval_or_matrix, rhs, x):
        """(r, omega): r = b - A x accumulated in double-double and rounded once, omega the componentwise backward error
        max_i |r_i| / (|A||x| + |b|)_i, per right-hand side."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        Xv, _ = self._rhs_block(x, self._dim)
        if Xv.shape != B.shape:
            raise OkktError("rhs and x must have the same shape")
        R = np.zeros_like(B)
        om = np.zeros(B.shape[0])
        self._check(self._lib.okkt_residual(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(Xv), L.p_f64(R), B.shape[0], L.p_f64(om)),
                    "okkt_residual")
        return (R[0] if single else R), (om[0] if single else om)

    # -- condition estimation and forward error bounds (not part of the reference interface)
    def condest(self, nzval_or_matrix, t=2):
        """okkt_condest: ||F||_1 (exact), the Higham-Tisseur estimate of ||F^-1||_1 (a lower bound) and their product cond1, for the
        factored F (these values plus the factorisation's diagonal shift).  Returns okkt_condest_info as a dict."""
        self._need()
        vals = self._values(nzval_or_matrix)
        info = L.OkktCondestInfo()
        self._check(self._lib.okkt_condest(self._h, L.p_f64(vals), int(t), C.byref(info)), "okkt_condest")
        return info.as_dict()

    def condest_indices(self):
        """The unit vectors e_j the last estimate used, in order (0-based)."""
        self._need()
        cnt = int(self._lib.okkt_condest_indices(self._h, None, 0))
        if cnt < 0:
            raise OkktError("okkt_condest_indices failed")
        out = np.zeros(max(cnt, 1), dtype=np.int64)
        self._lib.okkt_condest_indices(self._h, L.p_i64(out), cnt)
        return out[:cnt]

    def forward_error(self, nzval_or_matrix, rhs, x):
        """(ferr, berr): LAPACK's forward error bound || |F^-1| f ||_inf / ||x||_inf with f = |r| + (nz_i + 1) eps (|A||x| + |b|), and the
        componentwise backward error of the same residual pass, per right-hand side.  A bound only when A is the factored matrix."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        Xv, _ = self._rhs_block(x, self._dim)
        if Xv.shape != B.shape:
            raise OkktError("rhs and x must have the same shape")
        ferr = np.zeros(B.shape[0])
        berr = np.zeros(B.shape[0])
        self._check(self._lib.okkt_forward_error(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(Xv), B.shape[0], L.p_f64(ferr), L.p_f64(berr)),
                    "okkt_forward_error")
        return (ferr[0], berr[0]) if single else (ferr, berr)

    # -- eigenpairs nearest zero through the factor (not part of the reference interface)
    @staticmethod
    def _eigs_opts(nev, block, max_basis, max_restarts, tol, nlead, seed):
        o = L.OkktEigsOpts()
        o.nev, o.block, o.max_basis, o.max_restarts = int(nev), int(block), int(max_basis), int(max_restarts)
        o.tol, o.nlead, o.seed = float(tol), int(nlead), int(seed)
        return o

    def eigs(self, nev, nzval_or_matrix=None, block=4, max_basis=0, max_restarts=20, tol=0.0, nlead=0, seed=1, vectors=True):
        """okkt_eigs: the nev eigenvalues of smallest modulus of the factored F (nlead = 0 or dim), or of the pencil F v = lambda B v
        with B = diag(I_nlead, 0), by block shift-invert Krylov-Schur through the factor.  Returns (lam, V, resid, info): lam by
        ascending |lambda|, V with one full-length vector per row (None with vectors=False), resid the true residuals
        ||lambda B v - F v||_2 when the values (or the matrix) are given, else the Ritz residuals, info = okkt_eigs_info as a dict.  On
        `linear_solver_HIP.of_kkt(kkt)` F is the matrix okkt_kkt_factor last factored."""
        self._need()
        o = self._eigs_opts(nev, block, max_basis, max_restarts, tol, nlead, seed)
        vals = None if nzval_or_matrix is None else self._values(nzval_or_matrix)
        cnt = max(int(nev), 1)
        lam = np.zeros(cnt)
        res = np.zeros(cnt)
        V = np.zeros((cnt, max(self._dim, 1))) if vectors else None
        info = L.OkktEigsInfo()
        self._check(self._lib.okkt_eigs(self._h, C.byref(o), None if vals is None else L.p_f64(vals), L.p_f64(lam),
                                        None if V is None else L.p_f64(V), L.p_f64(res), C.byref(info)), "okkt_eigs")
        return lam[: int(nev)], (None if V is None else V[: int(nev), : self._dim]), res[: int(nev)], info.as_dict()

    def eigs_dev(self, nev, d_nzval=None, d_vecs=None, block=4, max_basis=0, max_restarts=20, tol=0.0, nlead=0, seed=1):
        """eigs with the values and the vectors (dim x nev, or None) in HBM (device pointers); returns (lam, resid, info)."""
        self._need()
        o = self._eigs_opts(nev, block, max_basis, max_restarts, tol, nlead, seed)
        cnt = max(int(nev), 1)
        lam = np.zeros(cnt)
        res = np.zeros(cnt)
        info = L.OkktEigsInfo()
        self._check(self._lib.okkt_eigs_dev(self._h, C.byref(o), None if d_nzval is None else C.c_void_p(d_nzval), L.p_f64(lam),
                                            None if d_vecs is None else C.c_void_p(d_vecs), L.p_f64(res), C.byref(info)), "okkt_eigs_dev")
        return lam[: int(nev)], res[: int(nev)], info.as_dict()

    # -- symmetric equilibration before the factorisation (not part of the reference interface)
    def set_scaling(self, mode, sweeps=0, s=None):
        """okkt_set_scaling: mode "none" | "ruiz" | "user" (or OKKT_SCALE_*).  "ruiz": every factorisation computes s by `sweeps`
        Jacobi sweeps (0 = 10) rounded to powers of two and factors S F S; "user": the vector s (analysed dimension, original order,
        finite and > 0) as given.  Solves, refinement and the estimates keep describing the unscaled matrix."""
        self._need()
        mode = L.OKKT_SCALE[mode] if isinstance(mode, str) else int(mode)
        v = None if s is None else L.f64(s)
        if v is not None and self._dim and v.shape != (self._dim,):
            raise OkktError("s must have the analysed dimension")
        self._check(self._lib.okkt_set_scaling(self._h, mode, int(sweeps), None if v is None else L.p_f64(v)), "okkt_set_scaling")
        self._scale_mode = mode

    def scaling(self):
        """s of the current factor (original order)."""
        self._need()
        out = np.zeros(self._dim)
        self._check(self._lib.okkt_get_scaling(self._h, L.p_f64(out), None), "okkt_get_scaling")
        return out

    def scaling_info(self):
        """okkt_scaling_info of the current factor as a dict (mode, sweeps, rowmax_min, rowmax_max, zero_rows)."""
        self._need()
        out = np.zeros(max(self._dim, 1))
        info = L.OkktScalingInfo()
        self._check(self._lib.okkt_get_scaling(self._h, L.p_f64(out), C.byref(info)), "okkt_get_scaling")
        return info.as_dict()

    def scaling_dev(self, d_s_out):
        self._need()
        self._check(self._lib.okkt_get_scaling_dev(self._h, C.c_void_p(d_s_out)), "okkt_get_scaling_dev")

    # -- Schur mode: partial factorisation with a dense Schur complement (not part of the reference interface)
    def set_schur(self, idx):
        """Hold the variables idx (0-based, distinct) back: the next analyze() orders the rest and puts them last as one front that
        ls_factor_schur assembles into S = A22 - A21 A11^-1 A12 and does not factor.  An empty idx clears the set."""
        self._need()
        p = L.i64(np.asarray(idx, dtype=np.int64).ravel())
        self._check(self._lib.okkt_set_schur(self._h, len(p), L.p_i64(p) if len(p) else None), "okkt_set_schur")
        self._ns = len(p)

    def _kind(self):
        return L.OKKT_SYM_DEFINITE if self.sym == "definite" else L.OKKT_SYM_SYMMETRIC

    def ls_factor_schur(self, nzval_or_matrix, n1, m1):
        """Factor A11 (n1 + m1 = dim - ns) and assemble S; 1 / 0 under the contract of ls_factor_b applied to A11.  The values in
        the analysed order, or the matrix itself with the analysed pattern."""
        self._need()
        vals = self._values(nzval_or_matrix)
        inert = L.OkktInertia()
        rc = self._check(self._lib.okkt_factor_schur(self._h, L.p_f64(vals), n1, m1, self._kind(), C.byref(inert)), "okkt_factor_schur")
        self.inertia = inert.as_tuple()
        return int(rc)

    def ls_factor_schur_dev(self, d_nzval, n1, m1):
        self._need()
        inert = L.OkktInertia()
        rc = self._check(self._lib.okkt_factor_schur_dev(self._h, C.c_void_p(d_nzval), n1, m1, self._kind(), C.byref(inert)), "okkt_factor_schur_dev")
        self.inertia = inert.as_tuple()
        return int(rc)

    def schur(self):
        """S as a dense symmetric ns x ns NumPy array, rows and columns in the order of the set."""
        self._need()
        ns = self._ns
        S = np.zeros((ns, ns))
        self._check(self._lib.okkt_get_schur(self._h, L.p_f64(S), ns), "okkt_get_schur")
        return S      # column-major with ld = ns is the transpose of this C-order array, and S is symmetric

    def schur_dev(self, d_S, ld):
        self._need()
        self._check(self._lib.okkt_get_schur_dev(self._h, C.c_void_p(d_S), int(ld)), "okkt_get_schur_dev")

    def schur_condense(self, rhs):
        """r2 = b2 - A21 A11^-1 b1 (set order); rhs: a vector or one right-hand side per row, original order."""
        self._need()
        B, single = self._rhs_block(rhs, self._dim)
        R2 = np.zeros((B.shape[0], self._ns))
        self._check(self._lib.okkt_schur_condense(self._h, L.p_f64(B), L.p_f64(R2), B.shape[0]), "okkt_schur_condense")
        return R2[0] if single else R2

    def schur_condense_dev(self, d_rhs, d_r2, nrhs=1):
        self._need()
        self._check(self._lib.okkt_schur_condense_dev(self._h, C.c_void_p(d_rhs), C.c_void_p(d_r2), int(nrhs)), "okkt_schur_condense_dev")

    def schur_expand(self, rhs, x2):
        """x with x[idx] = x2 and x1 = A11^-1 (b1 - A12 x2); rhs as in schur_condense, x2 one row of ns per right-hand side."""
        self._need()
        B, single = self._rhs_block(rhs, self._dim)
        X2 = L.f64(np.asarray(x2, dtype=np.float64).reshape(B.shape[0], self._ns))
        X = np.zeros_like(B)
        self._check(self._lib.okkt_schur_expand(self._h, L.p_f64(B), L.p_f64(X2), L.p_f64(X), B.shape[0]), "okkt_schur_expand")
        return X[0] if single else X

    def schur_expand_dev(self, d_rhs, d_x2, d_x, nrhs=1):
        self._need()
        self._check(self._lib.okkt_schur_expand_dev(self._h, C.c_void_p(d_rhs), C.c_void_p(d_x2), C.c_void_p(d_x), int(nrhs)), "okkt_schur_expand_dev")

    # -- the dense factor of S: Bunch-Kaufman L D L' on the device
    def _schur_factor(self, fn, what, S, ld):
        self._need()
        si, ti = L.OkktInertia(), L.OkktInertia()
        rc = self._check(fn(self._h, S, int(ld), C.byref(si), C.byref(ti)), what)
        self.schur_inertia = si.as_tuple()
        self.total_inertia = ti.as_tuple()
        return int(rc)

    def schur_factor(self, S=None):
        """Factor S with pivoting: the assembled S of the last ls_factor_schur, or a symmetric ns x ns array (its lower triangle is
        read).  1 when no pivot is zero or non-finite, else 0; sets schur_inertia (S's counts) and total_inertia (A11's + S's)."""
        if S is None:
            return self._schur_factor(self._lib.okkt_schur_factor, "okkt_schur_factor", None, self._ns)
        A = L.f64(np.asarray(S, dtype=np.float64).T)      # column-major for the library
        if A.shape != (self._ns, self._ns):
            raise OkktError(f"S must be {self._ns} x {self._ns}")
        return self._schur_factor(self._lib.okkt_schur_factor, "okkt_schur_factor", L.p_f64(A), self._ns)

    def schur_factor_dev(self, d_S=None, ld=None):
        return self._schur_factor(self._lib.okkt_schur_factor_dev, "okkt_schur_factor_dev", None if d_S is None else C.c_void_p(d_S),
                                  self._ns if ld is None else ld)

    def schur_dense_solve(self, r2):
        """x2 = S^-1 r2 with the factor of schur_factor; r2: a vector of ns or one right-hand side per row, set order."""
        self._need()
        B, single = self._rhs_block(r2, self._ns)
        X = np.zeros_like(B)
        self._check(self._lib.okkt_schur_dense_solve(self._h, L.p_f64(B), L.p_f64(X), B.shape[0]), "okkt_schur_dense_solve")
        return X[0] if single else X

    def schur_dense_solve_dev(self, d_r2, d_x2, nrhs=1):
        self._need()
        self._check(self._lib.okkt_schur_dense_solve_dev(self._h, C.c_void_p(d_r2), C.c_void_p(d_x2), int(nrhs)), "okkt_schur_dense_solve_dev")

    def schur_solve(self, rhs):
        """x with A x = rhs for the whole matrix: one forward sweep over the interior, the dense solve with the factor of S, the
        backward sweep; rhs as in schur_condense."""
        self._need()
        B, single = self._rhs_block(rhs, self._dim)
        X = np.zeros_like(B)
        self._check(self._lib.okkt_schur_solve(self._h, L.p_f64(B), L.p_f64(X), B.shape[0]), "okkt_schur_solve")
        return X[0] if single else X

    def schur_solve_dev(self, d_rhs, d_sol, nrhs=1):
        self._need()
        self._check(self._lib.okkt_schur_solve_dev(self._h, C.c_void_p(d_rhs), C.c_void_p(d_sol), int(nrhs)), "okkt_schur_solve_dev")

    # -- scenario batches: B items in Schur mode on one pattern, their S summed on the device
    def schur_batch_query(self, nrhs_max=1):
        """Whether the analysed plan takes a scenario batch, and what one costs: dict of okkt_schur_batch_info (host only)."""
        self._need()
        info = L.OkktSchurBatchInfo()
        self._check(self._lib.okkt_schur_batch_query(self._h, int(nrhs_max), C.byref(info)), "okkt_schur_batch_query")
        return info.as_dict()

    def schur_batch_reserve(self, B, nrhs_max=1):
        """Slots for B items, the sum buffers and the batch's own dense factor; solve work for nrhs_max columns."""
        self._need()
        self._check(self._lib.okkt_schur_batch_reserve(self._h, int(B), int(nrhs_max)), "okkt_schur_batch_reserve")

    def schur_batch_release(self):
        self._need()
        self._check(self._lib.okkt_schur_batch_release(self._h), "okkt_schur_batch_release")

    def _schur_batch_factor_items(self, fn, what, B, vals, stride, shifts, nshift, n1, m1):
        sh = None if shifts is None else L.f64(shifts).ravel()
        if sh is not None and sh.size != B:
            raise OkktError("shifts must have one entry per item")
        inert = (L.OkktInertia * B)()
        flags = np.zeros(B, dtype=np.int32)
        self._check(fn(self._h, B, vals, stride, None if sh is None else L.p_f64(sh), int(nshift), int(n1), int(m1), self._kind(), inert,
                       flags.ctypes.data_as(C.POINTER(C.c_int32))), what)
        self.schur_batch_inertia = [it.as_tuple() for it in inert]
        return flags

    def ls_factor_schur_batch(self, vals, n1, m1, shifts=None, nshift=None):
        """Factor A11 of every item and assemble its S_b.  vals: [B, nnz], one row per item, in the analysed order; n1 + m1 = dim - ns;
        shifts[b] is added to the first nshift (default n1) diagonal entries.  Returns the items' flags (1: inertia (n1, m1, 0) of
        A11_b); the counts are left in self.schur_batch_inertia."""
        self._need()
        v = L.f64(vals)
        if v.ndim != 2:
            raise OkktError("vals must be [B, nnz]")
        return self._schur_batch_factor_items(self._lib.okkt_factor_schur_batch, "okkt_factor_schur_batch", v.shape[0], L.p_f64(v), v.shape[1], shifts,
                                              n1 if nshift is None else nshift, n1, m1)

    def ls_factor_schur_batch_dev(self, d_nzval, B, val_stride, n1, m1, shifts=None, nshift=None):
        self._need()
        return self._schur_batch_factor_items(self._lib.okkt_factor_schur_batch_dev, "okkt_factor_schur_batch_dev", int(B), C.c_void_p(d_nzval),
                                              int(val_stride), shifts, n1 if nshift is None else nshift, n1, m1)

    def schur_batch(self, b=-1):
        """S_b of item b, or (b = -1) the sum of the items' S_b in the order the header states: dense symmetric ns x ns."""
        self._need()
        ns = self._ns
        S = np.zeros((ns, ns))
        self._check(self._lib.okkt_schur_batch_get(self._h, int(b), L.p_f64(S), ns), "okkt_schur_batch_get")
        return S

    def schur_batch_dev(self, d_S, ld, b=-1):
        self._need()
        self._check(self._lib.okkt_schur_batch_get_dev(self._h, int(b), C.c_void_p(d_S), int(ld)), "okkt_schur_batch_get_dev")

    def schur_batch_factor(self, S_add=None):
        """Dense factor of sum_b S_b (+ S_add, symmetric ns x ns, added last).  1 when no pivot is zero or non-finite, else 0; sets
        schur_inertia (the sum's counts) and total_inertia (the items' A11 counts + the sum's: the arrowhead matrix's)."""
        if S_add is None:
            return self._schur_factor(self._lib.okkt_schur_batch_factor, "okkt_schur_batch_factor", None, self._ns)
        A = L.f64(np.asarray(S_add, dtype=np.float64).T)
        if A.shape != (self._ns, self._ns):
            raise OkktError(f"S_add must be {self._ns} x {self._ns}")
        return self._schur_factor(self._lib.okkt_schur_batch_factor, "okkt_schur_batch_factor", L.p_f64(A), self._ns)

    def schur_batch_factor_dev(self, d_S_add=None, ld=None):
        return self._schur_factor(self._lib.okkt_schur_batch_factor_dev, "okkt_schur_batch_factor_dev", None if d_S_add is None else C.c_void_p(d_S_add),
                                  self._ns if ld is None else ld)

    def _sb_rhs(self, rhs):
        b = L.f64(rhs)
        if b.ndim not in (2, 3) or b.shape[-1] != self._dim:
            raise OkktError("rhs must be [B, dim] or [B, nrhs, dim] of the analysed dimension")
        return b, (1 if b.ndim == 2 else b.shape[1])

    def schur_batch_condense(self, rhs, items=False):
        """rhs [B, dim] or [B, nrhs, dim] -> the summed r2 ([ns] or [nrhs, ns]); items: also the items' r2_b ([B, ns] or [B, nrhs, ns])."""
        self._need()
        b, nrhs = self._sb_rhs(rhs)
        B, ns = b.shape[0], self._ns
        r2 = np.zeros((nrhs, ns))
        ri = np.zeros((B, nrhs, ns)) if items else None
        self._check(self._lib.okkt_schur_batch_condense(self._h, B, L.p_f64(b), L.p_f64(r2), None if ri is None else L.p_f64(ri), nrhs),
                    "okkt_schur_batch_condense")
        if b.ndim == 2:
            r2 = r2[0]
            ri = None if ri is None else ri[:, 0]
        return (r2, ri) if items else r2

    def schur_batch_condense_dev(self, d_rhs, d_r2_sum, B, nrhs=1, d_r2_items=None):
        self._need()
        self._check(self._lib.okkt_schur_batch_condense_dev(self._h, int(B), C.c_void_p(d_rhs), C.c_void_p(d_r2_sum),
                                                            None if d_r2_items is None else C.c_void_p(d_r2_items), int(nrhs)), "okkt_schur_batch_condense_dev")

    def schur_batch_expand(self, rhs, x2):
        """The one x2 ([ns] or [nrhs, ns]) put into every item: x_b = A11_b^-1 (b_b - A12_b x2), x[b][idx] = x2; same shape as rhs."""
        self._need()
        b, nrhs = self._sb_rhs(rhs)
        X2 = L.f64(np.asarray(x2, dtype=np.float64).reshape(nrhs, self._ns))
        out = np.empty_like(b)
        self._check(self._lib.okkt_schur_batch_expand(self._h, b.shape[0], L.p_f64(b), L.p_f64(X2), L.p_f64(out), nrhs), "okkt_schur_batch_expand")
        return out

    def schur_batch_expand_dev(self, d_rhs, d_x2, d_sol, B, nrhs=1):
        self._need()
        self._check(self._lib.okkt_schur_batch_expand_dev(self._h, int(B), C.c_void_p(d_rhs), C.c_void_p(d_x2), C.c_void_p(d_sol), int(nrhs)),
                    "okkt_schur_batch_expand_dev")

    def schur_batch_solve(self, rhs, rhs0=None):
        """The arrowhead system: rhs [B, dim] or [B, nrhs, dim] (the entries at idx are the items' shares of the linking right-hand side),
        rhs0 ([ns] or [nrhs, ns]) added to their sum last.  Returns the solutions, same shape; [b][idx] is x_L in every item."""
        self._need()
        b, nrhs = self._sb_rhs(rhs)
        r0 = None if rhs0 is None else L.f64(np.asarray(rhs0, dtype=np.float64).reshape(nrhs, self._ns))
        out = np.empty_like(b)
        self._check(self._lib.okkt_schur_batch_solve(self._h, b.shape[0], L.p_f64(b), None if r0 is None else L.p_f64(r0), L.p_f64(out), nrhs),
                    "okkt_schur_batch_solve")
        return out

    def schur_batch_solve_dev(self, d_rhs, d_sol, B, nrhs=1, d_rhs0=None):
        self._need()
        self._check(self._lib.okkt_schur_batch_solve_dev(self._h, int(B), C.c_void_p(d_rhs), None if d_rhs0 is None else C.c_void_p(d_rhs0),
                                                         C.c_void_p(d_sol), int(nrhs)), "okkt_schur_batch_solve_dev")

    def schur_batch_select(self, b):
        """Slot b becomes the handle's own state: every other call then behaves as after ls_factor_schur of that item."""
        self._need()
        self._check(self._lib.okkt_schur_batch_select(self._h, int(b)), "okkt_schur_batch_select")
        if getattr(self, "schur_batch_inertia", None) and 0 <= b < len(self.schur_batch_inertia):
            self.inertia = self.schur_batch_inertia[b]

    def schur_get_factor(self):
        """(LD, ipiv) as LAPACK's dsytrf(lower) returns them: LD[i, j] with unit L below the diagonal and D on it, ipiv 1-based with
        negative pairs for the 2 x 2 blocks."""
        self._need()
        ns = self._ns
        LD = np.zeros((ns, ns))
        ipiv = np.zeros(ns, dtype=np.int32)
        self._check(self._lib.okkt_schur_get_factor(self._h, L.p_f64(LD), ns, ipiv.ctypes.data_as(C.POINTER(C.c_int32))), "okkt_schur_get_factor")
        return np.ascontiguousarray(LD.T), ipiv

    # -- selected inversion: entries of F^-1 on the pattern of the factor (not part of the reference interface)
    @classmethod
    def of_kkt(cls, kkt):
        """The level-1 handle of a KKT solver (okkt_kkt_linear_solver) as a linear_solver_HIP that does not own it: its selected
        inverse, inverse diagonal and log-determinant are those of the matrix okkt_kkt_factor last factored."""
        self = cls("symmetric")
        self._lib = kkt._lib
        self._h = C.c_void_p(kkt._lib.okkt_kkt_linear_solver(kkt._k))
        self._borrowed = True
        self._dim = kkt.linear_solver_stats()["n"]
        return self

    def selinv(self):
        """okkt_selinv: Z = F^-1 on the stored pattern of L, kept on the device for the exports below.  Returns okkt_selinv_info as a
        dict (seconds_device, arena_bytes, nonfinite, status)."""
        self._need()
        info = L.OkktSelinvInfo()
        self._check(self._lib.okkt_selinv(self._h, C.byref(info)), "okkt_selinv")
        return info.as_dict()

    def inverse_diag(self):
        """diag(F^-1), original order."""
        self._need()
        out = np.zeros(self._dim)
        self._check(self._lib.okkt_get_inverse_diag(self._h, L.p_f64(out)), "okkt_get_inverse_diag")
        return out

    def inverse_diag_dev(self, d_out):
        self._need()
        self._check(self._lib.okkt_get_inverse_diag_dev(self._h, C.c_void_p(d_out)), "okkt_get_inverse_diag_dev")

    def inverse_on_pattern(self):
        """(F^-1)_ij at every entry of the analysed input pattern, nzval layout (NaN for an upper-triangle entry whose mirror is
        outside the pattern of L)."""
        self._need()
        nnz = C.c_int64()
        self._check(self._lib.okkt_get_inverse_on_pattern(self._h, None, C.byref(nnz)), "okkt_get_inverse_on_pattern")
        out = np.zeros(max(nnz.value, 1))
        self._check(self._lib.okkt_get_inverse_on_pattern(self._h, L.p_f64(out), C.byref(nnz)), "okkt_get_inverse_on_pattern")
        return out[: nnz.value]

    def inverse_on_pattern_dev(self, d_zval):
        self._need()
        self._check(self._lib.okkt_get_inverse_on_pattern_dev(self._h, C.c_void_p(d_zval)), "okkt_get_inverse_on_pattern_dev")

    def inverse_csc(self):
        """The lower triangle of F^-1 (diagonal included, permuted numbering) on the pattern of L, as scipy CSC."""
        self._need()
        nnz = C.c_int64()
        self._check(self._lib.okkt_get_inverse_csc(self._h, None, None, None, C.byref(nnz)), "okkt_get_inverse_csc")
        colptr = np.zeros(self._dim + 1, dtype=np.int64)
        rowval = np.zeros(max(nnz.value, 1), dtype=np.int64)
        val = np.zeros(max(nnz.value, 1))
        self._check(self._lib.okkt_get_inverse_csc(self._h, L.p_i64(colptr), L.p_i64(rowval), L.p_f64(val), C.byref(nnz)),
                    "okkt_get_inverse_csc")
        return sp.csc_matrix((val[: nnz.value], rowval[: nnz.value], colptr), shape=(self._dim, self._dim))

    def logdet(self):
        """(log |det F|, sign) from D."""
        self._need()
        v = C.c_double()
        s = C.c_int32()
        self._check(self._lib.okkt_logdet(self._h, C.byref(v), C.byref(s)), "okkt_logdet")
        return v.value, int(s.value)

    # -- threshold pivot report and the robust route through the Schur set (not part of the reference interface)
    def pivot_report(self, u=1e-8):
        """okkt_pivot_report: scan the stored L for g_j = max_i |L_ij| and count the pivots MA97's threshold test with ma97_u = u would
        have rejected (g_j > 1/u).  Returns okkt_pivot_info as a dict.  On `linear_solver_HIP.of_kkt(kkt)` it describes the matrix
        okkt_kkt_factor last factored."""
        self._need()
        info = L.OkktPivotInfo()
        self._check(self._lib.okkt_pivot_report(self._h, float(u), C.byref(info)), "okkt_pivot_report")
        return info.as_dict()

    def multipliers(self):
        """(g, partner) of the last report, original order: g[c] of the column that eliminates variable c and the original index of the
        row that attains it (-1: no row below the diagonal)."""
        self._need()
        g = np.zeros(self._dim)
        p = np.zeros(self._dim, dtype=np.int64)
        self._check(self._lib.okkt_get_multipliers(self._h, L.p_f64(g) if self._dim else L.p_f64(np.zeros(1)), L.p_i64(p) if self._dim else None),
                    "okkt_get_multipliers")
        return g, p

    def multipliers_dev(self, d_g_out, d_partner_out=None):
        self._need()
        self._check(self._lib.okkt_get_multipliers_dev(self._h, C.c_void_p(d_g_out), None if d_partner_out is None else C.c_void_p(d_partner_out)),
                    "okkt_get_multipliers_dev")

    def rejected_pivots(self):
        """(idx, partner): the rejected columns of the last report (original indices) by descending g, ties by ascending index, and
        their partners."""
        self._need()
        cnt = int(self._check(self._lib.okkt_get_rejected_pivots(self._h, None, None, 0), "okkt_get_rejected_pivots"))
        idx = np.zeros(max(cnt, 1), dtype=np.int64)
        par = np.zeros(max(cnt, 1), dtype=np.int64)
        self._check(self._lib.okkt_get_rejected_pivots(self._h, L.p_i64(idx), L.p_i64(par), cnt), "okkt_get_rejected_pivots")
        return idx[:cnt], par[:cnt]

    # -- the factor as an operator: half solves, products, the growth factor (not part of the reference interface)
    def _half(self, fn, what, v):
        self._need()
        B, single = self._rhs_block(v, self._dim)
        X = np.zeros_like(B)
        self._check(fn(self._h, L.p_f64(B), L.p_f64(X), B.shape[0]), what)
        return X[0] if single else X

    def ls_solve_forward(self, rhs):
        """okkt_solve_forward: z = D^-1 L^-1 P S b in factor order (index j is original index perm()[j]) -- okkt_solve stopped behind its
        forward sweep.  rhs: a vector or one right-hand side per row.  On `linear_solver_HIP.of_kkt(kkt)` (here and below) the factor is
        that of the matrix okkt_kkt_factor last factored."""
        return self._half(self._lib.okkt_solve_forward, "okkt_solve_forward", rhs)

    def ls_solve_backward(self, z):
        """okkt_solve_backward: x = S P^T L^-T z in the original order; ls_solve_backward(ls_solve_forward(b)) is ls_solve(b) bit for bit."""
        return self._half(self._lib.okkt_solve_backward, "okkt_solve_backward", z)

    def ls_solve_forward_dev(self, d_rhs, d_z, nrhs=1):
        self._need()
        self._check(self._lib.okkt_solve_forward_dev(self._h, C.c_void_p(d_rhs), C.c_void_p(d_z), int(nrhs)), "okkt_solve_forward_dev")

    def ls_solve_backward_dev(self, d_z, d_sol, nrhs=1):
        self._need()
        self._check(self._lib.okkt_solve_backward_dev(self._h, C.c_void_p(d_z), C.c_void_p(d_sol), int(nrhs)), "okkt_solve_backward_dev")

    def quadform(self, rhs):
        """okkt_quadform: (q_pos, q_neg) per right-hand side from one forward sweep: the sums of d_j z_j^2 over the positive and over the
        negative pivots; b' F^-1 b = q_pos + q_neg."""
        self._need()
        B, single = self._rhs_block(rhs, self._dim)
        qp = np.zeros(B.shape[0])
        qn = np.zeros(B.shape[0])
        self._check(self._lib.okkt_quadform(self._h, L.p_f64(B), B.shape[0], L.p_f64(qp), L.p_f64(qn)), "okkt_quadform")
        return (qp[0], qn[0]) if single else (qp, qn)

    def quadform_dev(self, d_rhs, nrhs=1):
        """quadform with the right-hand sides resident in HBM; the results come back to the host."""
        self._need()
        qp = np.zeros(max(int(nrhs), 1))
        qn = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_quadform_dev(self._h, C.c_void_p(d_rhs), int(nrhs), L.p_f64(qp), L.p_f64(qn)), "okkt_quadform_dev")
        return qp[: int(nrhs)], qn[: int(nrhs)]

    @staticmethod
    def _op(op):
        return L.OKKT_OP[op] if isinstance(op, str) else int(op)

    def factor_multiply(self, op, x):
        """okkt_factor_multiply: op "L" | "LT" (factor coordinates, unit diagonal included, no scaling) | "LDLT" | "ABS_LDLT" (original
        coordinates: S^-1 P^T L D L^T P S^-1 x, and the same with absolute values throughout).  x: a vector or one per row."""
        self._need()
        B, single = self._rhs_block(x, self._dim)
        Y = np.zeros_like(B)
        self._check(self._lib.okkt_factor_multiply(self._h, self._op(op), L.p_f64(B), L.p_f64(Y), B.shape[0]), "okkt_factor_multiply")
        return Y[0] if single else Y

    def factor_multiply_dev(self, op, d_x, d_y, nrhs=1):
        self._need()
        self._check(self._lib.okkt_factor_multiply_dev(self._h, self._op(op), C.c_void_p(d_x), C.c_void_p(d_y), int(nrhs)),
                    "okkt_factor_multiply_dev")

    def factor_error(self, nzval_or_matrix, probes=2):
        """okkt_factor_error: the growth factor rho = || |L||D||L^T| e ||_inf / ||F||_inf of the static-pivot factor and the sampled
        backward error eta of the factor against these values.  Returns okkt_factor_error_info as a dict."""
        self._need()
        vals = self._values(nzval_or_matrix)
        info = L.OkktFactorErrorInfo()
        self._check(self._lib.okkt_factor_error(self._h, L.p_f64(vals), int(probes), C.byref(info)), "okkt_factor_error")
        return info.as_dict()

    def factor_error_dev(self, d_nzval, probes=2):
        self._need()
        info = L.OkktFactorErrorInfo()
        self._check(self._lib.okkt_factor_error_dev(self._h, C.c_void_p(d_nzval), int(probes), C.byref(info)), "okkt_factor_error_dev")
        return info.as_dict()

    # -- sparse right-hand sides: tree-pruned solves and entries of the inverse (not part of the reference interface)
    def _sparse_columns(self, B):
        """(colptr, rowidx, val, nrhs) of a scipy.sparse matrix with one right-hand side per column, or of an (idx, val) pair (one column)."""
        if isinstance(B, tuple):
            idx, val = L.i64(np.atleast_1d(B[0])), L.f64(np.atleast_1d(B[1]))
            if idx.shape != val.shape or idx.ndim != 1:
                raise OkktError("ls_solve_sparse: (idx, val) must be two vectors of one length")
            return np.array([0, len(idx)], dtype=np.int64), idx, val, 1
        M = sp.csc_matrix(B)
        if M.shape[0] != self._dim:
            raise OkktError(f"ls_solve_sparse: B has {M.shape[0]} rows, the analysed dimension is {self._dim}")
        M.sum_duplicates()
        return L.i64(M.indptr), L.i64(M.indices), L.f64(M.data), M.shape[1]

    @staticmethod
    def _opt_i64(a):
        return (None, None) if a is None else (lambda v: (v, L.p_i64(v)))(L.i64(np.atleast_1d(a)))

    def ls_solve_sparse(self, B, rows=None):
        """okkt_solve_sparse: F x = b for sparse right-hand sides, visiting only the supernodes between the non-zeros of b, the wanted
        rows and the roots of the elimination forest.  B: scipy.sparse, one right-hand side per column, or an (idx, val) pair.  rows
        (None: all): the entries of x that are wanted.  Returns (X, info): X[q, t] = x_q[rows[t]] (a vector for an (idx, val) pair),
        equal to ls_solve of the densified b at those entries, and okkt_sparse_info as a dict.  On `linear_solver_HIP.of_kkt(kkt)`
        (here and below) the factor is that of the matrix okkt_kkt_factor last factored."""
        self._need()
        colptr, rowidx, val, nrhs = self._sparse_columns(B)
        xi, xp = self._opt_i64(rows)
        nx = self._dim if xi is None else len(xi)
        X = np.zeros((nrhs, nx))
        info = L.OkktSparseInfo()
        self._check(self._lib.okkt_solve_sparse(self._h, nrhs, L.p_i64(colptr), L.p_i64(rowidx) if len(rowidx) else None,
                                                L.p_f64(val) if len(val) else None, nx, xp, L.p_f64(X) if X.size else None, C.byref(info)),
                    "okkt_solve_sparse")
        return (X[0] if isinstance(B, tuple) else X), info.as_dict()

    def ls_solve_sparse_dev(self, colptr, rowidx, d_val, d_x_out, rows=None):
        """ls_solve_sparse with the values and the result (nrhs x len(rows), or nrhs x dim) resident in HBM; the indices stay on the
        host, where the sets are computed.  Returns okkt_sparse_info as a dict."""
        self._need()
        colptr, rowidx = L.i64(colptr), L.i64(rowidx)
        xi, xp = self._opt_i64(rows)
        info = L.OkktSparseInfo()
        self._check(self._lib.okkt_solve_sparse_dev(self._h, len(colptr) - 1, L.p_i64(colptr), L.p_i64(rowidx) if len(rowidx) else None, C.c_void_p(d_val),
                                                    0 if xi is None else len(xi), xp, C.c_void_p(d_x_out), C.byref(info)), "okkt_solve_sparse_dev")
        return info.as_dict()

    def inverse_columns(self, cols, rows=None, with_info=False):
        """okkt_get_inverse_columns: (F^-1)[rows, cols] as a len(rows) x len(cols) array (rows None: all), from sparse solves with the
        unit columns -- entries off the pattern of L included."""
        self._need()
        ci, cp = self._opt_i64(cols)
        xi, xp = self._opt_i64(rows)
        nr = self._dim if xi is None else len(xi)
        out = np.zeros((len(ci), nr))
        info = L.OkktSparseInfo()
        self._check(self._lib.okkt_get_inverse_columns(self._h, len(ci), cp, nr, xp, L.p_f64(out) if out.size else None, C.byref(info)),
                    "okkt_get_inverse_columns")
        Z = np.ascontiguousarray(out.T)
        return (Z, info.as_dict()) if with_info else Z

    def inverse_columns_dev(self, cols, d_out, rows=None):
        self._need()
        ci, cp = self._opt_i64(cols)
        xi, xp = self._opt_i64(rows)
        info = L.OkktSparseInfo()
        self._check(self._lib.okkt_get_inverse_columns_dev(self._h, len(ci), cp, 0 if xi is None else len(xi), xp, C.c_void_p(d_out), C.byref(info)),
                    "okkt_get_inverse_columns_dev")
        return info.as_dict()

    def inverse_block(self, idx):
        """(F^-1)[idx, idx]: inverse_columns(idx, idx)."""
        return self.inverse_columns(idx, idx)

    def sparse_reach(self, b_rows, x_rows=None):
        """okkt_sparse_reach (host only; works on host_symbolic_only handles after analyze): the sets ls_solve_sparse would use for
        non-zero rows b_rows and wanted rows x_rows.  Returns (info, active): okkt_sparse_info as a dict and dim bytes in factor order,
        bit 0 = the column's supernode runs in the forward sweep, bit 1 = in the backward sweep, bit 2 = it is fringe."""
        self._need()
        bi, bp = self._opt_i64([] if b_rows is None else b_rows)
        xi, xp = self._opt_i64(x_rows)
        active = np.zeros(max(self._dim, 1), dtype=np.uint8)
        info = L.OkktSparseInfo()
        self._check(self._lib.okkt_sparse_reach(self._h, len(bi), bp if len(bi) else None, 0 if xi is None else len(xi), xp, C.byref(info),
                                                active.ctypes.data_as(C.POINTER(C.c_uint8))), "okkt_sparse_reach")
        return info.as_dict(), active[: self._dim]

    def schur_solve_refine(self, nzval_or_matrix, rhs, max_steps=3, tol=0.0):
        """ls_solve_refine through the Schur route (okkt_schur_solve_refine): every solve is schur_solve's, the residuals are against
        the whole A.  Needs ls_factor_schur and schur_factor() of the handle's own S.  Returns (x, info) as ls_solve_refine."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        X = np.zeros_like(B)
        om = np.zeros(B.shape[0])
        info = L.OkktRefineInfo()
        self._check(self._lib.okkt_schur_solve_refine(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(X), B.shape[0], int(max_steps), float(tol),
                                                       C.byref(info), L.p_f64(om)), "okkt_schur_solve_refine")
        d = info.as_dict()
        d["omega_per_rhs"] = om
        return (X[0] if single else X), d

    def schur_solve_refine_dev(self, d_nzval, d_rhs, d_sol, nrhs=1, max_steps=3, tol=0.0):
        self._need()
        info = L.OkktRefineInfo()
        om = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_schur_solve_refine_dev(self._h, C.c_void_p(d_nzval), C.c_void_p(d_rhs), C.c_void_p(d_sol), int(nrhs),
                                                           int(max_steps), float(tol), C.byref(info), L.p_f64(om)), "okkt_schur_solve_refine_dev")
        return info.as_dict(), om[: int(nrhs)]

    def ls_factor_robust(self, A, n, m, u=1e-8, max_rounds=3, max_set=None):
        """Factor A (inertia (n, m, 0) wanted) so that no pivot of the static-pivot part fails the threshold test with ma97_u = u.
        Round 1 is ls_factor_b and a pivot report; while columns are rejected, they and their partners (the row a rejected 1 x 1
        pivot lost to: Bunch-Kaufman pairs the two into a 2 x 2 block) join the Schur set, the pattern is analysed again,
        ls_factor_schur factors the interior and the report runs on it.  At most max_rounds rounds, at most max_set set variables
        (default max(64, ceil(sqrt(dim)))): past either an OkktError carries the last report and the handle is left without a set.
        When a set was needed, schur_factor() factors S with pivoting and the flag is inertia_status of total_inertia against (n, m)
        and of the dense factor's own flag; otherwise the handle stays in its ordinary mode and the flag is ls_factor_b's.
        Returns (flag, info): info["rounds"], info["set"] (sorted original indices), info["rejected"] and info["max_multiplier"] per
        round, info["mode"] ("plain" | "schur").  Symmetric kind only; refused while a scaling is set (Schur mode refuses scalings)."""
        self._need()
        if self.sym != "symmetric":
            raise OkktError("ls_factor_robust: symmetric kind only")
        if self._scale_mode != L.OKKT_SCALE_NONE:
            raise OkktError("ls_factor_robust: a scaling is set on this handle and Schur mode does not factor a scaled matrix")
        if max_rounds < 1:
            raise OkktError("ls_factor_robust: max_rounds < 1")
        dim = csc_arrays(A)[0]
        if max_set is None:
            max_set = max(64, int(np.ceil(np.sqrt(dim))))
        if self._ns:
            self.set_schur([])
        self._robust_mode = None
        cur = np.zeros(0, dtype=np.int64)
        rejected, biggest = [], []
        flag = 0
        for rnd in range(1, max_rounds + 1):
            if len(cur) == 0:
                flag = self.ls_factor_b(A, n, m)
            else:
                self.set_schur(cur)
                self.analyze(A)
                n_in = int(np.count_nonzero(cur < n))
                self.ls_factor_schur(A, n - n_in, m - (len(cur) - n_in))
            rep = self.pivot_report(u)
            rejected.append(int(rep["rejected"]))
            biggest.append(float(rep["max_multiplier"]))
            if rep["rejected"] == 0:
                break
            idx, par = self.rejected_pivots()
            grown = np.union1d(cur, np.union1d(idx, par[par >= 0])).astype(np.int64)
            why = None
            if rnd == max_rounds:
                why = f"columns are still rejected after {max_rounds} rounds"
            elif len(grown) > max_set or len(grown) >= dim:
                why = f"the Schur set would grow to {len(grown)} variables (max_set = {max_set})"
            if why is not None:
                self.set_schur([])
                raise OkktError(f"ls_factor_robust: {why}; last report: {rep}, rejected per round {rejected}")
            cur = grown
        info = {"rounds": len(rejected), "set": cur, "rejected": rejected, "max_multiplier": biggest, "mode": "schur" if len(cur) else "plain"}
        if len(cur):
            dense_flag = self.schur_factor()
            pos, neg, zero, nonfinite = self.total_inertia
            flag = int(dense_flag == 1 and nonfinite == 0 and inertia_status(pos, neg, zero, n, m))
        self._robust_mode = info["mode"]
        return flag, info

    def ls_solve_robust(self, A_or_nzval, rhs, max_steps=5):
        """Solve with the factorisation of ls_factor_robust and refine against A: ls_solve_refine when it ended in the ordinary mode,
        schur_solve_refine when it ended in Schur mode.  Returns (x, info) as ls_solve_refine."""
        mode = self._robust_mode
        if mode is None:
            raise OkktError("ls_solve_robust: ls_factor_robust has not succeeded on this solver")
        if mode == "schur":
            return self.schur_solve_refine(A_or_nzval, rhs, max_steps=max_steps)
        return self.ls_solve_refine(A_or_nzval, rhs, max_steps=max_steps)

    # -- the Schur route made whole: what judges a doubtful factor, through the set (not part of the reference interface; DESIGN.md
    #    section 8.10).  Except schur_inverse every call needs ls_factor_schur and schur_factor() of the handle's own S
    def schur_inverse(self):
        """S^-1 (ns x ns, set order) from the dense factor of schur_factor, of the handle's own S or of a caller's.  Both triangles
        are the same bits.  schur_inverse_nonfinite holds the number of its non-finite entries afterwards."""
        self._need()
        ns = self._ns
        buf = np.zeros(max(ns * ns, 1))      # (never a NULL pointer: outside Schur mode the library says so itself)
        self._check(self._lib.okkt_schur_get_inverse(self._h, L.p_f64(buf), ns), "okkt_schur_get_inverse")
        self.schur_inverse_nonfinite = int(self._lib.okkt_schur_inverse_nonfinite(self._h))
        return np.ascontiguousarray(buf[: ns * ns].reshape(ns, ns).T)      # the library writes column-major

    def schur_inverse_dev(self, d_Z, ld=None):
        self._need()
        self._check(self._lib.okkt_schur_get_inverse_dev(self._h, C.c_void_p(d_Z), self._ns if ld is None else int(ld)), "okkt_schur_get_inverse_dev")
        self.schur_inverse_nonfinite = int(self._lib.okkt_schur_inverse_nonfinite(self._h))

    def schur_selinv(self):
        """okkt_schur_selinv: Z = A^-1 on the pattern of the whole factor (the interior's panels and the full lower triangle on the
        set), kept on the device: inverse_diag / inverse_csc / inverse_on_pattern serve it until the next ls_factor_schur or
        schur_factor.  Returns okkt_selinv_info as a dict."""
        self._need()
        info = L.OkktSelinvInfo()
        self._check(self._lib.okkt_schur_selinv(self._h, C.byref(info)), "okkt_schur_selinv")
        return info.as_dict()

    def schur_logdet(self):
        """(log |det A|, sign) from the interior's D and the 1 x 1 and 2 x 2 blocks of the dense D."""
        self._need()
        v = C.c_double()
        s = C.c_int32()
        self._check(self._lib.okkt_schur_logdet(self._h, C.byref(v), C.byref(s)), "okkt_schur_logdet")
        return v.value, int(s.value)

    def schur_condest(self, nzval_or_matrix, t=2):
        """condest through the Schur route: ||A||_1 of the whole matrix and the estimate of ||A^-1||_1 with schur_solve's solves."""
        self._need()
        vals = self._values(nzval_or_matrix)
        info = L.OkktCondestInfo()
        self._check(self._lib.okkt_schur_condest(self._h, L.p_f64(vals), int(t), C.byref(info)), "okkt_schur_condest")
        return info.as_dict()

    def schur_condest_dev(self, d_nzval, t=2):
        self._need()
        info = L.OkktCondestInfo()
        self._check(self._lib.okkt_schur_condest_dev(self._h, C.c_void_p(d_nzval), int(t), C.byref(info)), "okkt_schur_condest_dev")
        return info.as_dict()

    def schur_forward_error(self, nzval_or_matrix, rhs, x):
        """(ferr, berr) as forward_error, with |A^-1| f estimated through the Schur route."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        Xv, _ = self._rhs_block(x, self._dim)
        if Xv.shape != B.shape:
            raise OkktError("rhs and x must have the same shape")
        ferr = np.zeros(B.shape[0])
        berr = np.zeros(B.shape[0])
        self._check(self._lib.okkt_schur_forward_error(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(Xv), B.shape[0], L.p_f64(ferr),
                                                        L.p_f64(berr)), "okkt_schur_forward_error")
        return (ferr[0], berr[0]) if single else (ferr, berr)

    def schur_forward_error_dev(self, d_nzval, d_rhs, d_x, nrhs=1):
        self._need()
        ferr = np.zeros(max(int(nrhs), 1))
        berr = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_schur_forward_error_dev(self._h, C.c_void_p(d_nzval), C.c_void_p(d_rhs), C.c_void_p(d_x), int(nrhs),
                                                            L.p_f64(ferr), L.p_f64(berr)), "okkt_schur_forward_error_dev")
        return ferr[: int(nrhs)], berr[: int(nrhs)]

    def schur_solve_gmres(self, nzval_or_matrix, rhs, restart=30, max_iters=200, tol=0.0):
        """ls_solve_gmres through the Schur route: the initial solve and every preconditioner application are schur_solve's.
        Returns (x, info) as ls_solve_gmres; max_iters = 0 returns schur_solve's x."""
        self._need()
        vals = self._values(nzval_or_matrix)
        B, single = self._rhs_block(rhs, self._dim)
        X = np.zeros_like(B)
        om = np.zeros(B.shape[0])
        info = L.OkktGmresInfo()
        self._check(self._lib.okkt_schur_solve_gmres(self._h, L.p_f64(vals), L.p_f64(B), L.p_f64(X), B.shape[0], int(restart), int(max_iters),
                                                      float(tol), C.byref(info), L.p_f64(om)), "okkt_schur_solve_gmres")
        d = info.as_dict()
        d["omega_per_rhs"] = om
        return (X[0] if single else X), d

    def schur_solve_gmres_dev(self, d_nzval, d_rhs, d_sol, nrhs=1, restart=30, max_iters=200, tol=0.0):
        self._need()
        info = L.OkktGmresInfo()
        om = np.zeros(max(int(nrhs), 1))
        self._check(self._lib.okkt_schur_solve_gmres_dev(self._h, C.c_void_p(d_nzval), C.c_void_p(d_rhs), C.c_void_p(d_sol), int(nrhs),
                                                          int(restart), int(max_iters), float(tol), C.byref(info), L.p_f64(om)),
                    "okkt_schur_solve_gmres_dev")
        return info.as_dict(), om[: int(nrhs)]

    # the dispatchers beside ls_solve_robust: the plain or the Schur form, according to the mode ls_factor_robust ended in
    def _robust(self, what, plain, schur):
        mode = self._robust_mode
        if mode is None:
            raise OkktError(f"{what}: ls_factor_robust has not succeeded on this solver")
        return schur if mode == "schur" else plain

    def condest_robust(self, A_or_nzval, t=2):
        return self._robust("condest_robust", self.condest, self.schur_condest)(A_or_nzval, t=t)

    def forward_error_robust(self, A_or_nzval, rhs, x):
        return self._robust("forward_error_robust", self.forward_error, self.schur_forward_error)(A_or_nzval, rhs, x)

    def selinv_robust(self):
        return self._robust("selinv_robust", self.selinv, self.schur_selinv)()

    def logdet_robust(self):
        return self._robust("logdet_robust", self.logdet, self.schur_logdet)()

    def ls_solve_gmres_robust(self, A_or_nzval, rhs, restart=30, max_iters=200, tol=0.0):
        return self._robust("ls_solve_gmres_robust", self.ls_solve_gmres, self.schur_solve_gmres)(A_or_nzval, rhs, restart=restart,
                                                                                                  max_iters=max_iters, tol=tol)
