/*
 * okkt.h -- C ABI of libonephase_kkt.so: the MI355X-native KKT linear-system path of the
 * one-phase interior point method (reference behaviour: ohinder/OnePhase.jl).
 *
 * Two drop-in levels:
 *
 *  (1) linear-solver level -- what a `linear_solver_HIP <: abstract_linear_system_solver`
 *      binds in place of `linear_solver_JULIA` (CHOLMOD):
 *        initialize!  src/linear_system_solvers/linear_system_solvers.jl:40   -> okkt_create
 *        ls_factor!   src/linear_system_solvers/julia.jl:21-97                -> okkt_analyze + okkt_factor
 *        ls_solve!    src/linear_system_solvers/julia.jl:99-103               -> okkt_solve
 *        ls_solve     src/linear_system_solvers/julia.jl:105-113              -> okkt_solve
 *        finalize!    src/linear_system_solvers/linear_system_solvers.jl:44   -> okkt_destroy
 *        inertia_status  src/linear_system_solvers/linear_system_solvers.jl:48-91 -> okkt_inertia + return code
 *
 *  (2) KKT-system level -- what a `HIP_KKT_solver <: abstract_KKT_system_solver` binds in
 *      place of Schur_KKT_solver / Symmetric_KKT_solver, keeping everything device-resident:
 *        form_system!                      src/kkt_system_solver/schur.jl:47-62, symmetric.jl:35-53 -> okkt_kkt_form_system
 *        update_delta_vecs! + factor!      schur.jl:64-87, symmetric.jl:55-57,85-102, kkt_system_solver.jl:98-113,190-204 -> okkt_kkt_factor
 *        compute_direction_implementation! schur.jl:89-182, symmetric.jl:59-83 (+ update_kkt_error! kkt_system_solver.jl:67-96) -> okkt_kkt_compute_direction
 *        ipopt_strategy!                   src/IPM/delta_strategy.jl:37-114 -> okkt_kkt_ipopt_strategy
 *
 * Conventions: plain pointers and sizes only; no exceptions cross the boundary.  Functions
 * return OKKT_OK (0) or a negative okkt_status; the factor calls return 1 (inertia correct),
 * 0 (inertia wrong / zero or non-finite pivot) or a negative error -- the same 1/0 contract as
 * ls_factor!.  All calls are blocking (the handle's HIP stream is synchronised before return).
 * A handle is not thread-safe; several handles may coexist.
 *
 * There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 * OKKT_ERR_NO_DEVICE (okkt_create succeeds only with opts.host_symbolic_only = 1, which permits
 * okkt_analyze and the query functions and nothing else).
 */
#ifndef OKKT_H
#define OKKT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct okkt_solver_s* okkt_handle;
typedef struct okkt_kkt_s* okkt_kkt_handle;

typedef enum {
  OKKT_OK = 0,
  OKKT_ERR_INVALID = -1,     /* bad argument / call out of order */
  OKKT_ERR_NO_DEVICE = -2,   /* no HIP device, or handle is host_symbolic_only */
  OKKT_ERR_HIP = -3,         /* a HIP runtime call failed (see okkt_last_error) */
  OKKT_ERR_ALLOC = -4,
  OKKT_ERR_INTERNAL = -5
} okkt_status;

/* sym_kind: the `sym` symbol of the reference's solver constructors (julia.jl:11) */
#define OKKT_SYM_DEFINITE 0   /* :definite  -- Cholesky semantics: success <=> every pivot > 0     */
#define OKKT_SYM_SYMMETRIC 1  /* :symmetric -- LDL^T, inertia from sign(D) with tolerance 1e-20   */

/* kkt_kind: pars.kkt.kkt_solver_type (parameters.jl:30) */
#define OKKT_KKT_SCHUR 0      /* Q = H + J' diag(y/s) J       (n x n),     Cholesky semantics */
#define OKKT_KKT_SYMMETRIC 1  /* K = [[H J'];[J -diag(s/y)]]  (n+m square), LDL^T inertia (n,m,0) */
#define OKKT_KKT_CLEVER_SYMMETRIC 2  /* parallel rows of J merged first: M = [[H 0];[J_new -U_new]] (n+m_new square),
                                      * inertia (n, m_new, 0); Clever_Symmetric_KKT_solver, clever_symmetric.jl:25-519 */
#define OKKT_KKT_SCHUR_DIRECT 3      /* Schur_KKT_solver_direct (schur_direct.jl:3-66, kkt_system_solver.jl:270-276): the Schur system of the
                                      * FACTORISED iterate, but rhs terms, dy and ds = (comp_r - dy .* s) ./ y from the CURRENT iterate
                                      * (the one of the last okkt_kkt_system_rhs) */
/* kkt_system_rescale of the clever-symmetric system (parameters.jl:24-28, clever_symmetric.jl:307-325) */
#define OKKT_RESCALE_NONE 0
#define OKKT_RESCALE_U_ONLY 1
#define OKKT_RESCALE_U_AND_X 2

typedef struct {
  int32_t device;             /* HIP device ordinal; -1 = current device */
  int32_t host_symbolic_only; /* 1: never touch the GPU (analysis + queries only; CPU-side tests) */
  int32_t ordering;           /* 0 automatic (default): AMD, replaced by level-structure nested dissection when the AMD
                                 elimination tree is a path of small fronts (banded KKT systems: a dependent pivot chain on a
                                 GPU), and by multilevel nested dissection when that needs at least 10 % fewer factor flops (n >= 10 000; both candidates are
                                 computed side by side); 1 natural, 2 user permutation (okkt_set_perm), 3 AMD always, 4 level-structure nested
                                 dissection always, 5 multilevel nested dissection always */
  int32_t relax_always;       /* supernode amalgamation knobs, <=0 = default */
  int32_t relax_small;
  int32_t relax_mid;
  double relax_small_frac;
  double relax_mid_frac;
  double relax_any_frac;
  double inertia_tol;         /* |d| <= tol counts as a zero pivot (julia.jl:73); default 1e-20 */
  int32_t small_front_max;    /* fronts of order <= this use the LDS-resident kernel; <=0 default */
  int32_t panel_nb;           /* block-column width in the big-front kernels; <=0 default */
  int32_t early_exit;         /* 1: a factorisation may stop once its inertia is decided wrong (see okkt_set_early_exit); default 0 */
  int32_t schur_dense_rows;   /* Schur KKT kinds only (OKKT_KKT_SCHUR, OKKT_KKT_SCHUR_DIRECT): rows of J kept out of J' Sigma J.
                                 0 (default) off; > 0: a row with more than this many entries is dense; -1 automatic: dense when
                                 nnz(row) > max(64, 10 sqrt(n)); other negative values are refused by okkt_kkt_create.  The k dense rows
                                 J_d become the border of A = [[H + J_s' Sigma_s J_s + delta I, J_d'], [J_d, -diag(s_d / y_d)]] (order
                                 n + k), whose Schur complement of the (2,2) block is Q.  Ignored by the other kinds and by level 1. */
} okkt_opts;

typedef struct {
  int64_t pos, neg, zero, nonfinite; /* counts over diag(D); julia.jl:72-78 */
} okkt_inertia;

typedef struct {
  int64_t n;              /* order of the analysed matrix */
  int64_t nnz_lower;      /* input entries with row >= col */
  int64_t nnzL;           /* sum_j c_j (structural, no relaxation zeros) */
  int64_t nnzL_stored;    /* panel entries actually stored (with relaxation zeros) */
  double flops_exact;     /* sum_j c_j^2  (SURVEY 8d factor flops) */
  double flops_stored;    /* dense-front flops executed */
  int64_t arena_bytes;    /* HBM bytes of the front arena as allocated (before the device plan exists: sum f^2 * 8) */
  int64_t nsuper;
  int64_t nlevels;
  int64_t max_front;
  int64_t n_small_fronts, n_big_fronts;
  int64_t sum_rowidx;     /* sum_s f_s (row-index entries) */
  double analyze_seconds; /* host time of the last analysis */
  double last_factor_ms;  /* device time of the last numeric factorisation (hipEvent) */
  double last_solve_ms;   /* device time of the last solve */
  uint64_t pattern_hash;
  int64_t n_analyze_calls; /* how many times a new pattern forced a re-analysis */
  int64_t ordering_used;   /* 0 AMD, 1 natural, 2 user, 4 level-structure nested dissection, 5 multilevel nested dissection */
  int64_t critical_pivots; /* pivots on the longest leaf-to-root path of the supernodal elimination tree */
  int64_t top_separator;   /* multilevel dissection: vertices of the top-level separator (-1: none) */
  int64_t amd_skipped;     /* automatic ordering: 1 = minimum degree was abandoned (small top separator), no flop comparison was made */
  double flops_other;      /* automatic ordering: factor flops of the candidate that lost the comparison (0: none, or skipped) */
  int64_t arena_dense_bytes; /* what the front arena would take with a dense f x f buffer per front (sum f^2 * 8: the layout of rounds 1 - 5);
                              * arena_bytes is the arena as allocated -- L panels + the region the contribution blocks share by lifetime */
} okkt_stats;

/* ---- level 1: linear solver ------------------------------------------------------------ */
int okkt_default_opts(okkt_opts* opts);
int okkt_create(okkt_handle* out, const okkt_opts* opts /* NULL = defaults */);
int okkt_destroy(okkt_handle h);
const char* okkt_last_error(okkt_handle h);
const char* okkt_version(void);

/* user permutation for opts.ordering == 2: perm[new] = old, 0-based; call before okkt_analyze */
int okkt_set_perm(okkt_handle h, const int64_t* perm, int64_t n);
/* pattern of a square CSC matrix (only row >= col is used; upper entries are ignored, as under
 * Symmetric(A,:L), julia.jl:34,52).  Cached by pattern (exact comparison with the analysed colptr/rowval): re-calling with the same pattern
 * is free, so the reference-shaped ls_factor!(A,...) can call it every time. */
int okkt_analyze(okkt_handle h, int64_t dim, const int64_t* colptr, const int64_t* rowval, int index_base);
int okkt_get_perm(okkt_handle h, int64_t* perm_out /* [dim], perm[new]=old, 0-based */);
int okkt_get_stats(okkt_handle h, okkt_stats* out);
int okkt_get_etree(okkt_handle h, int64_t* parent_out /* [dim] */, int64_t* colcount_out /* [dim] */);

/* numeric factorisation of the analysed pattern with values nzval (same order as rowval).
 * n + m must equal dim.  Returns 1 / 0 / <0 like ls_factor! (julia.jl:21-97). */
int okkt_factor(okkt_handle h, const double* nzval, int64_t n, int64_t m, int sym_kind, okkt_inertia* inertia_out);
/* same, nzval already resident in HBM (device pointer) */
int okkt_factor_dev(okkt_handle h, const double* d_nzval, int64_t n, int64_t m, int sym_kind, okkt_inertia* inertia_out);
/* sol = F \ rhs for nrhs right-hand sides stored one after another (julia.jl:101,110).  rhs may alias sol. */
int okkt_solve(okkt_handle h, const double* rhs, double* sol, int64_t nrhs);
int okkt_solve_dev(okkt_handle h, const double* d_rhs, double* d_sol, int64_t nrhs);
/* Iterative refinement with extra-precise residuals.  A is the symmetric matrix whose lower triangle the
 * analysed CSC holds with the values nzval (same order as rowval; upper-triangle entries ignored, duplicates summed, as the
 * factorisation reads them); nzval need not be the factored values (refining A with the factor of A + delta I is legitimate).
 * The residual r = b - A x is accumulated in double-double and rounded once; omega = max_i |r_i| / (|A||x| + |b|)_i is the
 * componentwise backward error (0 / 0 = 0; NaN when r or x holds a non-finite value).  The first call after an analysis builds a row-wise map of the pattern on the host
 * (O(nnz)) and keeps it, with a workspace of 8 B per entry, on the device until the next analysis.  Partitioned handles
 * (okkt_dist_set_partition with nparts > 1) are refused with OKKT_ERR_INVALID.
 * okkt_solve_refine: x = F \ b, then for each right-hand side on its own (Arioli-Demmel-Duff): compute r and omega, stop when
 * omega <= tol (<= 0: 2^-52), when omega > omega_prev / 2 (stagnation), when a value is non-finite or after max_steps corrections,
 * else x += F \ r.  Each right-hand side returns the iterate with the smallest finite omega it reached; max_steps = 0 returns the
 * x of okkt_solve and omega0.  One small device-to-host read per step decides.  Returns OKKT_OK whenever it ran: the outcome is in
 * info.status.  rhs may alias sol. */
typedef struct {
  int32_t steps;      /* corrections applied, max over the right-hand sides */
  int32_t status;     /* worst over the right-hand sides: 0 omega <= tol, 1 step limit, 2 stagnated, 3 non-finite */
  double omega0;      /* max over rhs: componentwise backward error of the plain solve */
  double omega;       /* max over rhs: ... of the returned solutions */
  double resid_inf;   /* max over rhs: ||b - A x||_inf of the returned solutions */
} okkt_refine_info;

int okkt_residual(okkt_handle h, const double* nzval, const double* rhs, const double* x, double* r, int64_t nrhs,
                  double* omega_out /* [nrhs] or NULL */);
/* the same with device pointers for nzval, rhs, x and r; omega_out is host memory */
int okkt_residual_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, double* d_r, int64_t nrhs,
                      double* omega_out);
/* read-only, for tests: the partition of the row map that the residual, scaling and ||F||_1 passes share (csrc/refine.hip):
 * out = { lanes per short row, long_min (rows with more entries take a workgroup each), workgroups of the short rows, long rows,
 * entries that sum duplicates, entries of the full symmetric pattern }.  Builds the map when no call has built it yet, as
 * okkt_residual does, and carries okkt_residual's refusals; OKKT_ERR_INVALID for a NULL out. */
int okkt_debug_row_map(okkt_handle h, int64_t out[6]);
int okkt_solve_refine(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps,
                      double tol, okkt_refine_info* info /* or NULL */, double* omega_out /* [nrhs] or NULL */);
int okkt_solve_refine_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                          double tol, okkt_refine_info* info, double* omega_out);
/* GMRES-based iterative refinement (GMRES-IR; Carson and Higham, SIAM J. Sci. Comput. 2017/2018): solves
 * A x = b accurately when the handle holds the factor of a nearby F (A + delta I, a static-pivot factor, the factor of an earlier
 * iterate), where okkt_solve_refine converges only when rho(I - F^-1 A) < 1 and then only at that rate.  A, nzval and the residual
 * are as for okkt_solve_refine.  Per right-hand side: x = F \ b; then outer steps, each one double-double residual r = b - A x with
 * omega, stopping at omega <= tol (<= 0: 2^-52; status 0), at a non-finite value (3), at omega > omega_prev / 2 after a cycle (2) or
 * when the iterations reach max_iters (1); otherwise one cycle of right-preconditioned GMRES on A d = r: v_1 = r / ||r||_2, each
 * iteration w = A (F^-1 v_j) with A z accumulated in double-double and rounded once, classical Gram-Schmidt with one full
 * reorthogonalisation, Givens rotations on the host.  A cycle ends when the Arnoldi residual estimate is <= OKKT_GMRES_INNER_TOL times
 * ||r||_2, at restart iterations, on a happy breakdown or at the iteration cap; then x += F^-1 (V y) (one more solve per cycle).
 * Right-hand sides run in lockstep in groups of up to four (one multi-right-hand-side solve pass per preconditioner application);
 * one small device-to-host read per iteration decides.  Deterministic (no floating-point atomics, fixed summation orders): two calls
 * give identical bits.  Each right-hand side returns the iterate with the smallest finite omega it reached; max_iters = 0 returns
 * the x of okkt_solve and omega0.  Returns OKKT_OK whenever it ran: the outcome is in info.status.  rhs may alias sol.  The device
 * workspace ((restart + 1) x 4 + 8 vectors of dim doubles) is allocated on the first call after an analysis, grown for a larger
 * restart and released with the analysis.  Refusals as okkt_solve_refine: OKKT_ERR_INVALID for nrhs < 0, max_iters < 0,
 * restart > 64, before a factorisation, after an early-exit factorisation that stopped short, on partitioned handles and in Schur
 * mode (the handle stays usable); OKKT_ERR_NO_DEVICE on host_symbolic_only handles. */
#define OKKT_GMRES_INNER_TOL 1e-10   /* relative tolerance of a GMRES cycle on ||A d - r||_2 / ||r||_2 */
typedef struct {
  int32_t iterations; /* preconditioned operator applications inside GMRES cycles, max over the right-hand sides */
  int32_t cycles;     /* outer steps (one double-double residual + one GMRES cycle each), max over the right-hand sides */
  int32_t status;     /* worst over the right-hand sides: 0 omega <= tol, 1 iteration limit, 2 stagnated, 3 non-finite */
  int32_t solves;     /* solve passes with the factor (each carries up to 4 right-hand sides) */
  double omega0;      /* max over rhs: omega of the plain solve x0 = F \ b */
  double omega;       /* max over rhs: omega of the returned solutions */
  double resid_inf;   /* max over rhs: ||b - A x||_inf of the returned solutions */
  int64_t work_bytes; /* device workspace the call held */
} okkt_gmres_info;
int okkt_solve_gmres(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs,
                     int32_t restart /* 1..64, <= 0: 30 */, int32_t max_iters /* >= 0 */, double tol /* <= 0: 2^-52 */,
                     okkt_gmres_info* info /* or NULL */, double* omega_out /* [nrhs] or NULL */);
/* the same with device pointers for nzval, rhs and sol; info and omega_out are host memory */
int okkt_solve_gmres_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                         int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out);
/* Condition estimation and forward error bounds.  F is the matrix the handle factored: the symmetric matrix
 * whose lower triangle nzval holds (read as the factorisation reads it: upper-triangle entries ignored, duplicates summed) plus the
 * diagonal shift the factorisation adds at assembly (the delta that okkt_kkt_factor puts on the first n pivots; none at level 1).
 * ||F^-1||_1 is estimated by the block 1-norm estimator of Higham and Tisseur (SIAM J. Matrix Anal. Appl. 21, 2000, Algorithm 2.4)
 * with t columns (1..4; <= 0: 2; clamped to the order), at most 5 iterations, every product one multi-right-hand-side solve pass
 * (F^-T = F^-1).  Deterministic: the starting block and the replacement of parallel sign columns come from a fixed generator, argmax
 * ties go to the lowest index; two calls on the same factor give bitwise-identical results.  One small device-to-host read after each
 * solve pass.  Refused (OKKT_ERR_INVALID) on partitioned handles, before a factorisation and after an early-exit factorisation that
 * stopped short (as okkt_solve); a factorisation whose flag was 0 is accepted.  A solve that produces a non-finite value (an exact zero
 * pivot) ends the estimate with status 3 and cond1 = inv_norm1 = Inf. */
typedef struct {
  double norm1;       /* ||F||_1 (= ||F||_inf: F symmetric), exact, computed from the values */
  double inv_norm1;   /* estimate of ||F^-1||_1: a lower bound, attained by a returned vector */
  double cond1;       /* norm1 * inv_norm1 (Inf when a solve produced a non-finite value) */
  int32_t iterations; /* estimator iterations, <= 5 */
  int32_t solves;     /* solve passes used (each carries t right-hand sides) */
  int32_t status;     /* 0 converged, 1 iteration limit, 3 non-finite */
} okkt_condest_info;

int okkt_condest(okkt_handle h, const double* nzval, int32_t t /* 1..4, <=0: 2 */, okkt_condest_info* info);
/* the same with nzval in device memory */
int okkt_condest_dev(okkt_handle h, const double* d_nzval, int32_t t, okkt_condest_info* info);
/* the unit vectors e_j the last estimate of this handle (okkt_condest or okkt_forward_error) used, in the order it used them; returns
 * how many there were (at most cap are written), or < 0 on error */
int64_t okkt_condest_indices(okkt_handle h, int64_t* ind_out, int64_t cap);
/* LAPACK's forward error bound (xSYRFS FERR) for solutions x of A x = rhs the caller already has (from okkt_solve or
 * okkt_solve_refine): ferr_q = || |F^-1| f ||_inf / ||x||_inf with f = |r| + (nz_i + 1) eps (|A||x| + |b|), r the double-double residual
 * of okkt_residual against the values nzval, nz_i the entries of row i of the full symmetric A, eps = 2^-53 (||x||_inf = 0: the
 * absolute bound).  The numerator is estimated as the 1-norm of diag(f) F^-1 (its transpose F^-1 diag(f)) with t = 2, for each
 * right-hand side on its own.  It bounds the error of A's solution only when A is the factored matrix F; refining A with the factor of
 * A + delta I gives an estimate, not a bound.  berr_out receives omega of the same residual pass (bitwise okkt_residual's).  Same
 * refusals as okkt_condest. */
int okkt_forward_error(okkt_handle h, const double* nzval, const double* rhs, const double* x, int64_t nrhs,
                       double* ferr_out /* [nrhs] */, double* berr_out /* [nrhs] or NULL */);
/* the same with device pointers for nzval, rhs and x; ferr_out and berr_out are host memory */
int okkt_forward_error_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs,
                           double* ferr_out, double* berr_out);
/* ---- Eigenpairs nearest zero: block shift-invert Krylov-Schur through the factor ----------------------
 * F is the matrix the handle factored (the unscaled one, also under okkt_set_scaling).  nlead = 0 or dim: the standard problem
 * F v = lambda v, operator Op = F^-1 of order n = dim.  0 < nlead < dim: the pencil F v = lambda B v, B = diag(I_nlead, 0) in the
 * caller's index order, operator Op = E F^-1 E' of order n = nlead (pad with zeros, solve, keep the leading part): the eigenvalues of
 * the Schur complement F11 - F12 F22^-1 F21.  The nev eigenvalues of smallest modulus are returned by ascending |lambda| (of two equal
 * moduli the positive one first) with their vectors.
 *   Method: a hashed start block of `block` columns (splitmix64 of (seed, column, row) mapped to (-1, 1)); per sweep one okkt_solve
 * pass with `block` right-hand sides, the new block column of G = V' Op V formed in full, the dense symmetric eigen-solver on G on the
 * host, the residual norms ||Op V s - theta V s||_2 / |theta| of the leading Ritz pairs on the device; the next block is Op(Q)
 * orthogonalised against the whole basis (two classical Gram-Schmidt passes; a column that shrinks below 2^-33 of its norm is dropped,
 * a block that vanishes is replaced by a fresh hashed one).  When fewer slots than the next block has columns remain in max_basis the
 * basis is compressed to the leading min(m, nev + block) Ritz vectors; the next block is taken before the compression and never
 * truncated.  Converged: the nev leading residuals are <= tol.
 *   Returned vectors: v = F^-1 E' x scaled, x the Ritz vector (in standard mode that is Op V s, which the method holds anyway; in
 * pencil mode one more solve pass over the nev vectors), full length dim, column j at vecs + j * dim.  The leading n entries have unit
 * 2-norm and the entry of largest modulus among them (lowest index among ties) is positive.  With this v, lambda B v - F v =
 * lambda E' (x - Op x / theta): a converged pair has ||lambda B v - F v||_2 <= tol |lambda| (1 + tol) plus the rounding of the solve.
 *   resid: with nzval (the values of F on the analysed pattern, as for okkt_residual) the true residuals ||lambda B v - F v||_2 from
 * the double-double residual pass, info->true_residuals = 1; with nzval = NULL the residuals of the Ritz pairs the iteration stopped on.
 *   Deterministic: no atomics, sums in an order that depends on n alone; two calls give the same bits.
 *   Eigenvalues of multiplicity above `block` are not guaranteed to be found with all their copies.
 * Refused with OKKT_ERR_INVALID (the handle stays usable): nev outside 1..32 or above n; block outside 1..4; max_basis other than 0 or
 * 2 nev + 3 block .. 128; max_restarts < 0; tol < 0 or NaN; nlead outside 0..dim; before a complete factorisation, after an early-exit
 * factorisation that stopped short, on partitioned handles and in Schur mode.  OKKT_ERR_NO_DEVICE on host_symbolic_only handles (after
 * the argument checks). */
typedef struct {
  int32_t nev;          /* 1..32, <= n */
  int32_t block;        /* 1..4: right-hand sides per solve pass */
  int32_t max_basis;    /* 2 nev + 3 block .. 128; 0: max(48, 2 nev + 3 block), at most 128 and at most max(n, 2 nev + 3 block) */
  int32_t max_restarts; /* >= 0 */
  double tol;           /* >= 0; 0: 2^-26 */
  int64_t nlead;        /* 0 or dim: standard problem; else the pencil's leading block */
  uint64_t seed;
} okkt_eigs_opts;
typedef struct {
  int32_t status;          /* 0 converged; 1 restart limit (nconv leading pairs met tol, the outputs hold the current Ritz pairs); 2 the whole
                              space was spanned (m = n); 3 an operator product was not finite (lambda and resid NaN, vecs untouched) */
  int32_t nconv;           /* leading pairs whose residual met tol */
  int32_t sweeps;          /* operator applications to a block */
  int32_t solves;          /* right-hand sides solved: the block widths summed over the sweeps, plus nev in pencil mode */
  int32_t restarts;
  int32_t basis;           /* max_basis in effect */
  int32_t fresh_blocks;    /* hashed blocks drawn after the first */
  int32_t dropped_columns; /* columns the drop rule removed */
  int32_t true_residuals;  /* 1: resid holds ||lambda B v - F v||_2; 0: the Ritz residuals */
  int64_t bytes;           /* device workspace held by the handle for this feature */
} okkt_eigs_info;
int okkt_eigs(okkt_handle h, const okkt_eigs_opts* opts, const double* nzval /* or NULL */, double* lambda /* [nev] */,
              double* vecs /* [dim x nev] or NULL */, double* resid /* [nev] */, okkt_eigs_info* info /* or NULL */);
/* the same with nzval and vecs in device memory; lambda, resid and info are host memory */
int okkt_eigs_dev(okkt_handle h, const okkt_eigs_opts* opts, const double* d_nzval, double* lambda, double* d_vecs, double* resid,
                  okkt_eigs_info* info);
/* Test hook, host only (no device, no handle): the dense symmetric eigen-solver of okkt_eigs (csrc/sym_eig.h, cyclic Jacobi) on the
 * m x m row-major matrix a, 1 <= m <= 128, of which the upper triangle is read.  theta [m]: the eigenvalues by descending modulus;
 * s [m x m] row-major: column j the unit eigenvector of theta[j].  Returns 0, 2 when the sweep limit was reached, OKKT_ERR_INVALID for
 * m out of range, a NULL pointer or a non-finite entry (the outputs untouched). */
int okkt_debug_sym_eig(int32_t m, const double* a, double* theta, double* s);
/* ---- Schur mode: partial factorisation with a dense Schur complement ----------------------------------
 * A is the analysed symmetric matrix of order dim; the Schur set is idx[0..ns), distinct 0-based original indices, and orders the
 * rows and columns of S; A11 is A without the set (the interior), A22 the set's block.  The handle factors A11 and assembles
 * S = A22 - A21 A11^-1 A12 on the device without factoring it.
 *   Definite kind: S is positive definite exactly when A is (A11 being positive definite).
 *   Symmetric kind: inertia(A) = inertia(A11) + inertia(S) (Haynsworth inertia additivity).
 *   Whenever S x2 = r2 with r2 from okkt_schur_condense, okkt_schur_expand returns the x that solves A x = b.
 * On a handle in Schur mode okkt_factor(_dev), okkt_solve(_dev), okkt_solve_refine(_dev), okkt_condest(_dev),
 * okkt_forward_error(_dev), okkt_dist_set_partition with nparts > 1 and the other okkt_dist_* calls return OKKT_ERR_INVALID (the handle
 * stays usable); the Schur calls are refused the same way on a handle without a set.  Early exit (okkt_set_early_exit) does not apply
 * to okkt_factor_schur.  A factor that completed with flag 0 can still be exported, condensed and expanded. */
/* Call before okkt_analyze.  A different set forces a re-analysis; ns = 0 clears the set, and the handle then behaves exactly as
 * one that never had a set.  Refused: duplicates, indices out of range, ns >= dim (checked by okkt_analyze), ns < 0.  The interior
 * is ordered by opts.ordering on the pattern of A11; the set follows in idx order as one final supernode.  With ordering 2 the
 * permutation must end with idx in order. */
int okkt_set_schur(okkt_handle h, int64_t ns, const int64_t* idx);
/* Factor A11 and assemble S.  n1 + m1 = dim - ns.  Returns 1 / 0 under the contract of okkt_factor applied to A11 (symmetric:
 * pos == n1 && neg == m1 and nothing non-finite; definite: every pivot > 0), or < 0 on error.  The counts cover the dim - ns pivots
 * of A11. */
int okkt_factor_schur(okkt_handle h, const double* nzval, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* inertia_out);
int okkt_factor_schur_dev(okkt_handle h, const double* d_nzval, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* inertia_out);
/* S as a full symmetric ns x ns column-major matrix, rows and columns in idx order, leading dimension ld >= ns */
int okkt_get_schur(okkt_handle h, double* S, int64_t ld);
int okkt_get_schur_dev(okkt_handle h, double* d_S, int64_t ld);
/* condense: r2 = b2 - A21 A11^-1 b1 for each right-hand side (rhs: dim x nrhs, original order; r2: ns x nrhs, idx order) */
int okkt_schur_condense(okkt_handle h, const double* rhs, double* r2, int64_t nrhs);
int okkt_schur_condense_dev(okkt_handle h, const double* d_rhs, double* d_r2, int64_t nrhs);
/* expand: x[idx] = x2 and x1 = A11^-1 (b1 - A12 x2), x in original order (dim x nrhs).  Stateless: it does not rely on an earlier
 * condense call.  rhs may alias x. */
int okkt_schur_expand(okkt_handle h, const double* rhs, const double* x2, double* x, int64_t nrhs);
int okkt_schur_expand_dev(okkt_handle h, const double* d_rhs, const double* d_x2, double* d_x, int64_t nrhs);
/* ---- the dense factor of S ----
 * Factor S on the device with Bunch-Kaufman partial pivoting: P S P' = L D L', L unit lower triangular, D block diagonal with 1 x 1 and
 * 2 x 2 blocks (the pivot choice of LAPACK's dsytrf, lower variant).  S = NULL factors the S that the last okkt_factor_schur assembled
 * (which stays intact: okkt_get_schur returns it afterwards); a non-NULL S is the caller's symmetric ns x ns column-major matrix, of
 * which the lower triangle is read, ld >= ns -- the summed S of a decomposition.  inertia_S: the counts over D (a 2 x 2 block is one
 * positive and one negative pivot; a column that is exactly zero when its turn comes is a zero pivot and is skipped).  inertia_total:
 * A11's counts of the last okkt_factor_schur plus S's, by Haynsworth additivity the inertia of the whole matrix (A11's part is zero
 * before any okkt_factor_schur).  Either may be NULL.  Returns 1 when D has neither a zero nor a non-finite pivot, 0 otherwise, < 0 on
 * error.  Refused with OKKT_ERR_INVALID: no Schur set, S = NULL before a complete okkt_factor_schur, ld < ns. */
int okkt_schur_factor(okkt_handle h, const double* S_or_NULL, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total);
/* the same with S in device memory */
int okkt_schur_factor_dev(okkt_handle h, const double* d_S_or_NULL, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total);
/* The solves below are refused with OKKT_ERR_INVALID until okkt_schur_factor has succeeded, and again after a new okkt_factor_schur
 * when the factor is of the handle's own S (a factor of a caller's S stays valid).  After a factor with zero or non-finite pivots
 * they run and return what the divisions give, as okkt_solve does after such a factor of A.
 * x2 = S^-1 r2 (ns x nrhs each, idx order); r2 may alias x2. */
int okkt_schur_dense_solve(okkt_handle h, const double* r2, double* x2, int64_t nrhs);
int okkt_schur_dense_solve_dev(okkt_handle h, const double* d_r2, double* d_x2, int64_t nrhs);
/* A x = b for the whole matrix (dim x nrhs, original order): one forward sweep over the interior, the dense solve, the backward sweep.
 * It needs a complete okkt_factor_schur besides the dense factor.  rhs may alias sol. */
int okkt_schur_solve(okkt_handle h, const double* rhs, double* sol, int64_t nrhs);
int okkt_schur_solve_dev(okkt_handle h, const double* d_rhs, double* d_sol, int64_t nrhs);
/* The factor as dsytrf(uplo = 'L') returns it: LD (ns x ns column-major, ld >= ns; the strict upper triangle is set to zero) and
 * ipiv[ns], 1-based, a 2 x 2 block at columns k, k + 1 marked by ipiv[k] = ipiv[k + 1] = -(row interchanged with k + 1). */
int okkt_schur_get_factor(okkt_handle h, double* LD, int64_t ld, int32_t* ipiv);
/* ---- Selected inversion: entries of F^-1 on the pattern of the factor ----------------------------------
 * F is the matrix the handle factored (as for okkt_condest: the values plus the factorisation's diagonal shift).  okkt_selinv computes
 * Z = F^-1 = L^-T D^-1 L^-1 at every entry of the stored supernodal pattern of L (relaxation zeros included) and at the diagonal, on
 * the device, and keeps it there; the exports below read it.  Deterministic: no floating-point atomics and fixed summation orders, so
 * two calls on one factor give bitwise-identical Z.  Z belongs to the factorisation it was computed from: the next okkt_factor* makes
 * it stale, and the exports then return OKKT_ERR_INVALID until okkt_selinv runs again.  The device memory (the Z panels and a scratch
 * region reused level by level) is allocated by the first call after an analysis and released with the analysis.
 * Refused with OKKT_ERR_INVALID (the handle stays usable): before a factorisation, after an early-exit factorisation that stopped
 * short, on a handle in Schur mode and on partitioned handles; host_symbolic_only handles get OKKT_ERR_NO_DEVICE.  A factorisation
 * whose flag was 0 is accepted: non-finite entries of Z (an exact zero pivot) are counted in info.nonfinite and status is 1.
 * No existing call changes: okkt_solve after okkt_selinv is bitwise what it was before. */
typedef struct {
  double seconds_device;   /* the device time of the computation (HIP events around it) */
  int64_t arena_bytes;     /* device memory held for Z: the Z panels, the scratch region and the plan's index arrays */
  int64_t nonfinite;       /* non-finite entries of Z on the stored pattern */
  int32_t status;          /* 0 every entry finite, 1 some entry non-finite */
  double flops;            /* floating-point operations of the block products (2 m^2 w + 2 m w^2 per block of w columns, m rows below) */
} okkt_selinv_info;
int okkt_selinv(okkt_handle h, okkt_selinv_info* info /* or NULL */);
/* diag(F^-1) in the original order (d_out: dim doubles, host / device memory) */
int okkt_get_inverse_diag(okkt_handle h, double* d_out);
int okkt_get_inverse_diag_dev(okkt_handle h, double* d_out);
/* (F^-1)_ij at every entry (i, j) of the analysed input pattern, in nzval layout (nnz of the analysed colptr / rowval).  Every entry
 * takes the value at its position mirrored into the lower triangle of the permuted matrix: a lower-triangle entry always lies on
 * the pattern of L; an upper-triangle entry (ignored at analysis) gets the value of its mirrored entry when that position is on the
 * pattern of L, NaN otherwise.  Duplicate entries get the same value at every copy.  *nnz (if given) receives the count; a NULL zval
 * asks for the count only. */
int okkt_get_inverse_on_pattern(okkt_handle h, double* zval, int64_t* nnz);
int okkt_get_inverse_on_pattern_dev(okkt_handle h, double* d_zval);
/* the lower triangle of F^-1 in the permuted numbering as 0-based CSC: the pattern of okkt_get_factor_csc plus the diagonal, each
 * column's rows ascending (diagonal first); nnz = that of okkt_get_factor_csc + dim.  NULL arrays: *nnz only. */
int okkt_get_inverse_csc(okkt_handle h, int64_t* colptr, int64_t* rowval, double* val, int64_t* nnz);
/* log |det F| and its sign from D, summed in pivot order on the host (deterministic); sign 0 and -Inf when a pivot is 0.  Needs a
 * complete factorisation (not okkt_selinv); same refusals otherwise. */
int okkt_logdet(okkt_handle h, double* logabsdet, int32_t* sign);
/* ---- Threshold pivot report: the multipliers of the static-pivot factor ----------------------------------
 * The factorisation never pivots.  okkt_pivot_report reads the stored L once, on the device, and reports for every pivot column j (of
 * the permuted matrix) g_j = max_i |L_ij| over the stored rows below the diagonal (relaxation zeros included) and the row p_j that
 * attains it (the lowest front row on a tie), both kept on the device in the ORIGINAL numbering: g_out[c] and partner_out[c] describe
 * the column that eliminates original variable c, and partner_out[c] is an original index.  A 1 x 1 pivot passes MA97's threshold test
 * |a_jj| >= u max_{i>j} |a_ij| on the reduced matrix exactly when g_j <= 1/u, so `rejected` counts the pivots a threshold-pivoting
 * code run with ma97_u = u would not have taken where they stand.  A column with no row below the diagonal has g = 0 and p = -1; a
 * column that holds a NaN or an Inf has g = +Inf and p = its first such row.  In Schur mode the Schur front (it holds S, not L) is not
 * scanned: the set's variables get g = 0, p = -1, and the interior columns keep their rows towards the set.  A scaled factor (section
 * 8.8) is reported as stored (L~).  Deterministic: no atomics, (value, row) pairs reduced in a fixed order; two calls give identical bits.
 * The report belongs to the factorisation it scanned: the next okkt_factor* / okkt_factor_schur* makes it stale, and the getters then
 * return OKKT_ERR_INVALID until okkt_pivot_report runs again.  A call with another u on an unchanged factor recounts without
 * scanning again.  The device memory (2 x dim words and the work-item lists) is allocated by the first call after an analysis and
 * released with the analysis.
 * Refused with OKKT_ERR_INVALID (the handle stays usable): before a complete factorisation, after an early-exit factorisation that
 * stopped short, on partitioned handles, for u > 1 or a non-finite u; host_symbolic_only handles get OKKT_ERR_NO_DEVICE.  Accepted: a
 * factorisation whose flag was 0, Schur mode after a complete okkt_factor_schur, scaled factors, both sym_kinds.
 * No existing call changes: okkt_solve after okkt_pivot_report is bitwise what it was before. */
typedef struct {
  double u;                 /* threshold the counts refer to */
  int64_t rejected;         /* columns with g_j > 1/u (non-finite columns included) */
  int64_t nonfinite_cols;   /* columns that hold a NaN or an Inf */
  double max_multiplier;    /* max_j g_j */
  int64_t max_col;          /* original index of that column (lowest on a tie), -1 when dim = 0 */
  double seconds_device;    /* the device time of the scan (HIP events around it; that of the last scan when only recounting) */
} okkt_pivot_info;
int okkt_pivot_report(okkt_handle h, double u /* (0, 1]; <= 0: 1e-8, the reference's ma97_u */, okkt_pivot_info* info /* or NULL */);
/* g and the partners of the last report (dim entries each, original order; host / device memory).  partner_out may be NULL. */
int okkt_get_multipliers(okkt_handle h, double* g_out, int64_t* partner_out);
int okkt_get_multipliers_dev(okkt_handle h, double* d_g_out, int64_t* d_partner_out);
/* the rejected columns of the last report (original indices) and their partners, descending g, ties by ascending original index;
 * returns their number (at most cap are written; either array may be NULL), < 0 on error */
int64_t okkt_get_rejected_pivots(okkt_handle h, int64_t* idx_out, int64_t* partner_out, int64_t cap);
/* ---- The factor as an operator: half solves, products with L, D, L^T, the growth factor -----------------
 * FACTOR COORDINATES.  With the handle's permutation P (okkt_get_perm: index j of a vector in factor order is original index perm[j])
 * and scaling S (section 8.8; the identity when the factor is not scaled) the library holds F~ = S P F P^T S = L D L^T, L unit lower
 * triangular (okkt_get_factor_csc), D diagonal (okkt_get_diag), relaxation zeros of the supernodes included.  Vectors are nrhs columns
 * of dim doubles stored one after another, as for okkt_solve; which coordinates a vector is in is said per call.
 *
 * Half solves.  okkt_solve_forward: z = D^-1 L^-1 P S b (factor order) -- the forward sweep of okkt_solve stopped where it ends.
 * okkt_solve_backward: x = S P^T L^-T z (original order) -- the backward sweep started from the caller's z.  Both run right-hand
 * sides in okkt_solve's groups of 4, 2 and 1 through okkt_solve's kernels, so okkt_solve_backward(okkt_solve_forward(b)) is okkt_solve(b)
 * BIT FOR BIT.  rhs may alias z and z may alias sol.
 * okkt_quadform: one forward sweep per group and one reduction: q_pos[r] = sum over d_j > 0 of d_j z_j^2, q_neg[r] = the same over
 * d_j < 0 (so q_pos >= 0 >= q_neg and b^T F^-1 b = q_pos + q_neg); a pivot that is 0 or NaN contributes to neither.  The products
 * d_j z_j z_j are formed error-free (fma) and summed in double-double by a fixed tree, then rounded once: each result is within
 * 2^-52 (relative) of the exact sum over the z and D of the sweep, and two calls give the same bits.  q_pos / q_neg are host memory
 * in both forms.
 *
 * Products.  okkt_factor_multiply, op:
 *   OKKT_OP_L        y = L x                                            factor coordinates in and out, unit diagonal included, no scaling
 *   OKKT_OP_LT       y = L^T x                                          the same
 *   OKKT_OP_LDLT     y = S^-1 P^T  L   D   L^T  P S^-1  x               original coordinates: F x up to the factorisation's error
 *   OKKT_OP_ABS_LDLT y = S^-1 P^T |L| |D| |L^T| P S^-1 |x|              original coordinates
 * x may alias y.  Deterministic: no floating-point atomics, every sum in a fixed order; two calls give the same bits, and a column's
 * result does not depend on the columns it shares a pass with.
 *
 * okkt_factor_error: the growth factor of the static-pivot factorisation and a sampled backward error of the factor against the
 * values nzval (the matrix okkt_residual defines, plus the diagonal shift the factorisation added at assembly):
 *   norm_abs_ldlt = || OKKT_OP_ABS_LDLT applied to the vector of ones ||_inf,  norm_f = ||F||_inf,  rho = norm_abs_ldlt / norm_f;
 *   eta = max over the probes p < probes and the rows i of |(F v_p - LDLT v_p)_i| / ((|F| + ABS_LDLT) e)_i  (0 / 0 = 0; a non-finite
 *         quotient counts as +Inf), eta_row the row that attains it (original index; the lowest on a tie, -1 when dim = 0);
 *   LDLT v_p is the OKKT_OP_LDLT product, F v_p is accumulated in double-double (okkt_residual's pass) and the difference rounded once.
 *   Probe p has entry i (original index) -1 when the top bit of mix64((p << 32) ^ i) is set and +1 otherwise, in 64-bit unsigned
 *   arithmetic, mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *   return z ^ (z >> 31)  (the finaliser of splitmix64).
 * A factorisation that never pivots is backward stable exactly when rho is modest (Higham, Accuracy and Stability of Numerical
 * Algorithms, section 11.1); g_j of okkt_pivot_report is a proxy for it.  Two calls give the same bits.
 *
 * Refused with OKKT_ERR_INVALID (the handle stays usable), as okkt_pivot_report: before a complete factorisation, after an early-exit
 * factorisation that stopped short, on partitioned handles; moreover in Schur mode, for nrhs < 0, a NULL pointer, an unknown op,
 * probes > 8.  host_symbolic_only handles get OKKT_ERR_NO_DEVICE.  The device memory (the work-item lists, two blocks of 4 x dim
 * doubles, the partial sums of the big fronts) is allocated by the first product after an analysis and released with the analysis.
 * No existing call changes: okkt_solve after any of these is bitwise what it was before. */
int okkt_solve_forward(okkt_handle h, const double* rhs, double* z, int64_t nrhs);
int okkt_solve_forward_dev(okkt_handle h, const double* d_rhs, double* d_z, int64_t nrhs);
int okkt_solve_backward(okkt_handle h, const double* z, double* sol, int64_t nrhs);
int okkt_solve_backward_dev(okkt_handle h, const double* d_z, double* d_sol, int64_t nrhs);
int okkt_quadform(okkt_handle h, const double* rhs, int64_t nrhs, double* q_pos /* [nrhs] */, double* q_neg /* [nrhs] */);
int okkt_quadform_dev(okkt_handle h, const double* d_rhs, int64_t nrhs, double* q_pos /* host */, double* q_neg /* host */);
enum { OKKT_OP_L = 1, OKKT_OP_LT = 2, OKKT_OP_LDLT = 3, OKKT_OP_ABS_LDLT = 4 };
int okkt_factor_multiply(okkt_handle h, int op, const double* x, double* y, int64_t nrhs);
int okkt_factor_multiply_dev(okkt_handle h, int op, const double* d_x, double* d_y, int64_t nrhs);
typedef struct {
  double rho, norm_abs_ldlt, norm_f, eta;
  int64_t eta_row;
  int32_t probes;      /* probes used */
} okkt_factor_error_info;
int okkt_factor_error(okkt_handle h, const double* nzval, int32_t probes /* 1..8, <= 0: 2 */, okkt_factor_error_info* info);
/* the same with nzval in device memory */
int okkt_factor_error_dev(okkt_handle h, const double* d_nzval, int32_t probes, okkt_factor_error_info* info);
/* ---- Sparse right-hand sides: tree-pruned solves and entries of the inverse -----------------------------
 * okkt_solve_sparse solves F x = b for nrhs sparse columns b and returns the entries x_idx of every x.  The forward sweep visits only
 * the supernodes on the paths from the non-zeros of P b to the roots of the elimination forest, the backward sweep only the paths from
 * the requested entries to the roots; small fronts run as the whole tasks okkt_solve runs them in.  The visited fronts go through
 * okkt_solve's kernels in okkt_solve's order, so the result is, at the requested entries, what okkt_solve returns for the densified b:
 * equal as numbers (a zero may differ in sign).  Columns are taken in okkt_solve's groups of 4, 2 and 1; a group runs on the union of
 * its columns' sets; when a sweep's set is every supernode the ordinary sweep runs.  Deterministic: two calls give the same bytes.
 *
 * b: colptr[nrhs + 1] (colptr[0] >= 0, non-decreasing), rowidx and val of the entries colptr[q] .. colptr[q + 1] of column q, 0-based
 * original numbering, any order inside a column; an empty column gives a zero column.  x_idx NULL: x_out is nrhs x dim (column q at
 * x_out + q * dim) and nx is not read; else nrhs x nx, x_out[q * nx + t] = x_q[x_idx[t]] (duplicates allowed).  The index arrays are
 * host memory in both forms (the sets are host work); the _dev form takes the values and the result in device memory.
 * okkt_get_inverse_columns: (F^-1)[rows, cols], column-major nrows x ncols (rows NULL: all dim rows, nrows not read) -- okkt_solve_sparse
 * with the unit columns e_cols[j].
 * info (or NULL), all counts for the union of the call's columns: the supernodes in the two closures (reach), the supernodes the
 * launches visit (run >= reach), the fringe (fronts that do not run forward but whose parent does: their contribution vectors are
 * zeroed) and its entries, the bytes of the panels visited and of all panels, the groups, pruned (0: every group ran the ordinary
 * sweeps), and the time on the device.
 * okkt_sparse_reach: host only, also on host_symbolic_only handles, after okkt_analyze: the sets a call with non-zero rows b_rows (the
 * union of its columns; duplicates allowed) and requested rows x_idx (NULL: all) would use.  active_out (or NULL): dim bytes in factor
 * order (okkt_get_perm), bit 0 = the column's supernode runs in the forward sweep, bit 1 = in the backward sweep, bit 2 = it is fringe.
 *
 * Refused with OKKT_ERR_INVALID (the handle stays usable): a NULL pointer that is needed, nrhs < 0, nx < 0 (ncols, nrows, nb
 * likewise), a decreasing colptr, an index out of range, a row twice in one column of b; before okkt_analyze;
 * in Schur mode; on partitioned handles; before a complete factorisation and after an early exit that stopped short (not
 * okkt_sparse_reach).  host_symbolic_only handles get OKKT_ERR_NO_DEVICE from all but okkt_sparse_reach.  nrhs = 0, and nx = 0 with
 * x_idx given, succeed and do nothing.  No existing call changes: okkt_solve after any of these is bitwise what it was before. */
typedef struct {
  int64_t nsuper;
  int64_t fwd_reach, bwd_reach;      /* supernodes in the closures (union over the call's columns) */
  int64_t fwd_run, bwd_run;          /* supernodes the launches visit (>= reach: small fronts run as whole tasks) */
  int64_t fringe, fringe_entries;    /* children zeroed; sum of f - k over them */
  int64_t fwd_panel_bytes, bwd_panel_bytes, factor_panel_bytes;
  int32_t batches, pruned;           /* pruned = 0: the ordinary sweeps ran */
  double seconds_device;
} okkt_sparse_info;
int okkt_solve_sparse(okkt_handle h, int64_t nrhs, const int64_t* b_colptr, const int64_t* b_rowidx, const double* b_val,
                      int64_t nx, const int64_t* x_idx, double* x_out, okkt_sparse_info* info /* or NULL */);
int okkt_solve_sparse_dev(okkt_handle h, int64_t nrhs, const int64_t* b_colptr, const int64_t* b_rowidx, const double* d_b_val,
                          int64_t nx, const int64_t* x_idx, double* d_x_out, okkt_sparse_info* info /* or NULL */);
int okkt_get_inverse_columns(okkt_handle h, int64_t ncols, const int64_t* cols, int64_t nrows, const int64_t* rows, double* out,
                             okkt_sparse_info* info /* or NULL */);
int okkt_get_inverse_columns_dev(okkt_handle h, int64_t ncols, const int64_t* cols, int64_t nrows, const int64_t* rows, double* d_out,
                                 okkt_sparse_info* info /* or NULL */);
int okkt_sparse_reach(okkt_handle h, int64_t nb, const int64_t* b_rows, int64_t nx, const int64_t* x_idx, okkt_sparse_info* info,
                      uint8_t* active_out /* or NULL */);
/* Refinement through the Schur route: okkt_solve_refine's loop -- the same omega, stagnation rule, best
 * iterate, masked correction and one device-to-host read per step -- with every solve the fused whole-system solve of okkt_schur_solve.
 * nzval: the values of the whole A on the analysed pattern (residuals are against the whole matrix).  It needs a complete
 * okkt_factor_schur and an okkt_schur_factor of the handle's OWN S (S = NULL): after a factor of a caller's S, A is not this handle's
 * matrix and the call is refused with OKKT_ERR_INVALID, as it is outside Schur mode and on partitioned handles.  rhs may alias sol;
 * max_steps = 0 returns okkt_schur_solve's x. */
int okkt_schur_solve_refine(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t max_steps,
                            double tol, okkt_refine_info* info /* or NULL */, double* omega_out /* [nrhs] or NULL */);
int okkt_schur_solve_refine_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t max_steps,
                                double tol, okkt_refine_info* info, double* omega_out /* host memory */);
/* ---- The Schur route made whole ---------------------------------------------------------------------------
 * What judges and rescues a doubtful factor, for a handle in Schur mode: every call below takes A^-1 to be the fused whole-system
 * solve of okkt_schur_solve (the interior's static factor and the Bunch-Kaufman factor of S).  The plain calls (okkt_selinv,
 * okkt_logdet, okkt_condest, okkt_forward_error, okkt_solve_gmres) keep refusing a handle in Schur mode.  Except okkt_schur_get_inverse
 * every call needs what okkt_schur_solve_refine needs: a complete okkt_factor_schur and a current okkt_schur_factor of the handle's OWN
 * S; outside Schur mode, before or after a stale okkt_schur_factor, after a factor of a caller's S and on partitioned handles they
 * return OKKT_ERR_INVALID, on a host_symbolic_only handle OKKT_ERR_NO_DEVICE.  Two calls on one factor give the same bits.
 *
 * okkt_schur_get_inverse: Z (ns x ns, column-major, ld >= ns, set order) = S^-1 from the current dense factor, of the handle's own S
 * or of a caller's; both triangles are written and are bitwise mirror images.  Zero or non-finite pivots divide as they divide: the call
 * succeeds and okkt_schur_inverse_nonfinite returns the number of non-finite entries of the Z handed out last.  The device time of
 * the call is left in okkt_stats.last_solve_ms. */
int okkt_schur_get_inverse(okkt_handle h, double* Z, int64_t ld);
int okkt_schur_get_inverse_dev(okkt_handle h, double* d_Z, int64_t ld);
int64_t okkt_schur_inverse_nonfinite(okkt_handle h);
/* Selected inversion through the route: Z = A^-1 on the pattern of the whole factor -- the interior supernodes' panels and the full
 * lower triangle on the set (S^-1 above seeds the Schur front's panel, the top-down schedule of okkt_selinv runs below it).
 * Afterwards okkt_get_inverse_diag / _on_pattern / _csc (and _dev) serve this Z on the Schur-mode handle, until the next
 * okkt_factor_schur or okkt_schur_factor; before it they answer that there is no selected inverse. */
int okkt_schur_selinv(okkt_handle h, okkt_selinv_info* info /* or NULL */);
/* log |det A| and its sign (0 on a zero or NaN pivot) from the interior's D and the 1 x 1 and 2 x 2 blocks of the dense D */
int okkt_schur_logdet(okkt_handle h, double* logabsdet, int32_t* sign);
/* okkt_condest / okkt_forward_error (section 8.3) with Y = A^-1 X through the route; nzval: the values of the whole A on the analysed
 * pattern, which the 1-norm and the residuals are taken of.  okkt_condest_indices reports the unit vectors as after okkt_condest. */
int okkt_schur_condest(okkt_handle h, const double* nzval, int32_t t /* 1..4, <=0: 2 */, okkt_condest_info* info);
int okkt_schur_condest_dev(okkt_handle h, const double* d_nzval, int32_t t, okkt_condest_info* info);
int okkt_schur_forward_error(okkt_handle h, const double* nzval, const double* rhs, const double* x, int64_t nrhs,
                             double* ferr_out /* [nrhs] */, double* berr_out /* [nrhs] or NULL */);
int okkt_schur_forward_error_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, const double* d_x, int64_t nrhs,
                                 double* ferr_out /* host memory */, double* berr_out /* host memory or NULL */);
/* okkt_solve_gmres (section 8.6) with the initial solve and the preconditioner applications through the route; max_iters = 0 returns
 * okkt_schur_solve's x bit for bit.  rhs may alias sol. */
int okkt_schur_solve_gmres(okkt_handle h, const double* nzval, const double* rhs, double* sol, int64_t nrhs, int32_t restart,
                           int32_t max_iters, double tol, okkt_gmres_info* info /* or NULL */, double* omega_out /* [nrhs] or NULL */);
int okkt_schur_solve_gmres_dev(okkt_handle h, const double* d_nzval, const double* d_rhs, double* d_sol, int64_t nrhs, int32_t restart,
                               int32_t max_iters, double tol, okkt_gmres_info* info, double* omega_out /* host memory */);

/* ---- Symmetric equilibration before the factorisation ----------------------------------------------------
 * The factorisation never pivots; with a scaling on, okkt_factor(_dev) factors F~ = S F S for a positive diagonal S = diag(s), so that
 * the static-pivot LDL^T sees entries of comparable size.  Off by default; with OKKT_SCALE_NONE every call is bit for bit what it is
 * without this section, with no additional launch and no allocation.
 * The scaling (OKKT_SCALE_RUIZ).  A is the full symmetric matrix okkt_residual defines (lower triangle read, upper entries ignored,
 * duplicates summed), with the diagonal shift the factorisation adds at assembly (okkt_kkt_factor's delta) added to the stored diagonal
 * entries.  s starts at 1.  Each of the `sweeps` sweeps is a Jacobi update: for every row i, r_i = max_j ((|a_ij| * s_i) * s_j), all
 * rows from the old s, the products rounded in exactly this order; entries that are not finite are skipped in the maximum; then
 * s_i <- s_i / sqrt(r_i) (IEEE sqrt and division), except that a row whose r_i is 0 (or not finite) keeps its s_i.  After the last sweep
 * each s_i = m 2^e with m in [1/2, 1) becomes 2^(e-1) when m < fl(sqrt(1/2)) = 0x1.6a09e667f3bcdp-1 and 2^e otherwise, the exponent
 * clamped to [-510, 510] (an s_i that is not positive and finite becomes 1).  Ten sweeps by default: in the infinity norm the smallest
 * row maximum roughly square-roots per sweep, so after ten even a spread of 1e-300 is within a few percent of 1 and the rounding then
 * leaves every non-zero row maximum in (0.45, 2].  Scaling by powers of two is exact: the factor is bitwise the factor of the prescaled
 * matrix and the inertia is that of F (Sylvester); a factorisation that never pivots is moreover invariant under an exact scaling, so the
 * solutions of a RUIZ-scaled handle are bitwise those of an unscaled one while nothing leaves the exponent range: what the scaling changes
 * is which pivots inertia_tol counts as zero (those of F~) and the range.  The sweeps run on the device with no host read between them; a maximum does not
 * depend on the order it is taken in, so two calls give identical bits.
 * OKKT_SCALE_USER takes the caller's vector as it is (not rounded): dim entries in the original order, all finite and > 0, read and
 * copied by okkt_set_scaling, which therefore needs an analysed handle; the factor is then that of S F S up to two roundings per entry.
 * okkt_factor(_dev) with a scaling on: computes s from the values of this factorisation (RUIZ) or takes the caller's (USER), writes
 * v'_e = (s_row * v_e) * s_col for every input entry into a workspace of the handle -- the caller's nzval is never modified -- and
 * factors the workspace by the unchanged numeric path.  Everything is enqueued on the handle's stream inside the timed span of
 * last_factor_ms; the scaling adds no host synchronisation: its row-maximum extrema are read with the pivot counts at the end.  The
 * flag, the inertia counts, inertia_tol, early exit and the 1 / 0 contract apply to the pivots of F~.  The first scaled factorisation
 * after an analysis builds the row map of okkt_residual (if no call has yet) and a workspace of 16 B per input entry.
 * The solve family: okkt_solve(_dev) returns x = S F~^-1 S b, the two multiplications inside the permutation gather and scatter the
 * solve has anyway (no extra pass over the vectors).  okkt_solve_refine, okkt_solve_gmres, okkt_condest, okkt_forward_error and the KKT
 * level's directions and estimates all solve through it: they see F^-1 of the unscaled matrix and keep their residuals and norms against
 * the caller's unscaled nzval.
 * Exports: okkt_get_diag and okkt_get_factor_csc return D~ and L~, the factor of S F S.  okkt_logdet returns log |det F| =
 * log |det F~| - 2 ln 2 * sum_i e_i with s_i = 2^e_i, the e_i summed as integers (USER entries that are no power of two contribute
 * -2 ln s_i); the sign is that of det F~.
 * Refused with OKKT_ERR_INVALID and a message, the handle stays usable: a mode other than NONE on a handle in Schur mode or partitioned
 * with nparts > 1; okkt_set_schur with ns > 0 and okkt_dist_set_partition with nparts > 1 while a scaling is on; okkt_selinv while the
 * current factor is scaled; okkt_get_scaling(_dev) unless the handle holds a complete factorisation that used a scaling; an unknown
 * mode, sweeps > 64, USER with a NULL vector, a non-finite or non-positive entry, or before okkt_analyze; a USER vector given for another
 * dimension than the one analysed since (checked by the next factorisation).  On host_symbolic_only handles the setting is stored (it is
 * configuration) and the getters return OKKT_ERR_NO_DEVICE.
 * A re-analysis keeps the mode, the sweeps and a USER vector, and drops the computed scaling with the factor.  okkt_set_scaling itself
 * does not touch the current factor: the scaling takes effect, or ends, with the next factorisation. */
#define OKKT_SCALE_NONE 0   /* default */
#define OKKT_SCALE_RUIZ 1   /* computed from the values of every factorisation */
#define OKKT_SCALE_USER 2   /* the caller's vector, used as given */
typedef struct {
  int32_t mode, sweeps;           /* of the current factor (sweeps: 0 for USER) */
  double rowmax_min, rowmax_max;  /* over the nonzero rows of |S F S| as factored (0 when every row is zero) */
  int64_t zero_rows;              /* rows whose maximum is 0: they kept their s_i */
} okkt_scaling_info;
int okkt_set_scaling(okkt_handle h, int mode, int32_t sweeps /* RUIZ: 1..64, <= 0: 10 */,
                     const double* s_user /* USER: [dim], original order, all finite and > 0; else NULL */);
/* the scaling of the current factor */
int okkt_get_scaling(okkt_handle h, double* s_out /* [dim], original order */, okkt_scaling_info* info /* or NULL */);
int okkt_get_scaling_dev(okkt_handle h, double* d_s_out);

/* diag(F): the D of LDL^T in pivot (permuted) order, as `diag(solver._factor)` (julia.jl:72); of a scaled factor (section 8.8): D~ */
int okkt_get_diag(okkt_handle h, double* d_out /* [dim] */);
/* L as CSC in permuted numbering (unit diagonal not stored), for parity tests; pass NULLs to size; of a scaled factor: L~ */
int okkt_get_factor_csc(okkt_handle h, int64_t* colptr_out, int64_t* rowval_out, double* val_out, int64_t* nnz_out);

/* device-memory helpers so that callers without a HIP binding (ctypes, Julia) can keep inputs in HBM */
int okkt_dev_alloc(okkt_handle h, int64_t bytes, void** d_ptr_out);
int okkt_dev_free(okkt_handle h, void* d_ptr);
int okkt_dev_upload(okkt_handle h, void* d_dst, const void* src, int64_t bytes);
int okkt_dev_download(okkt_handle h, void* dst, const void* d_src, int64_t bytes);
/* ls_factor! only returns the inertia flag and the reference never solves with a factorisation that failed it
 * inside the delta loop (it updates delta and refactors, delta_strategy.jl:37-114).  With early exit enabled okkt_factor /
 * okkt_factor_dev stop before the top of the elimination tree when the pivots counted so far already decide a wrong
 * inertia; they return 0, `out` holds the counts of the columns eliminated so far, and okkt_solve is refused until the
 * next complete factorisation.  Off by default: outside the delta loop the reference DOES solve with a factorisation whose
 * flag was 0 (the refactorisation after a failed step, one_phase.jl:241), so only a caller that discards failed factors
 * may turn it on (the KKT level does so inside okkt_kkt_ipopt_strategy / okkt_kkt_factor_trial only). */
int okkt_set_early_exit(okkt_handle h, int enable);
/* the handle's HIP stream (hipStream_t as void*), for callers that time with their own events */
void* okkt_get_stream(okkt_handle h);
/* per-launch timing of the dominant kernel (k_front_dataflow, the persistent launch that factors the big fronts of one level;
 * with OKKT_DATAFLOW=0 the FP64-MFMA trailing update k_big_syrk of the per-step schedule): HIP events are recorded around
 * every launch on the handle's stream while enabled; okkt_get_profile returns the number of launches since enabling, their
 * summed duration and their summed algorithmic flops (k f^2 - k^2 f + k^3 / 3 per front of a dataflow launch; rem * (rem + 1) * nb
 * per front and block column of a trailing update, DESIGN.md "Kernels") */
int okkt_profile_dominant(okkt_handle h, int enable);
int okkt_get_profile(okkt_handle h, int64_t* n_launches, double* total_ms, double* total_flops);
/* Test hook, host only (no device, no handle): the task queue of the dataflow launch (csrc/dataflow.hip) for one level of
 * nfronts big fronts of orders f[] with k[] pivot columns each, as it would be uploaded for `workers` workers, `group & 255` panels
 * and `(group >> 8) & 255` row tiles (0 = 1) per bulk update task; bit 16 of `group`: D(q + 1) rides in TU(q) (bit 1 of nq in its task); bit 17: a block row of more than 64 rows is split between TA(q) (type 4, its upper 64 rows) right before TU(q) (bit 2 of nq); bit 18: the panel tiles from panel 1 on carry the last update of their tile (type 5 = TL(i, q): U(i, q, q - 1, 1) then T(i, q); that update is not a task of its own).  tasks receives 4 ints per task: front index, type | nq << 8 | rows << 16 (type 0 = D diagonal tile, 1 = T panel tile,
 * 2 = U update of the tiles (i .. i + rows - 1, j), 3 = TU: panel tile (i, j) and the diagonal tile (i, i), i = j + 1), i | j << 16 (tile row / column; for T: j = the panel), q0 (first panel of an update).  Returns the number of
 * tasks (also when it exceeds cap; only cap tasks are written), or a negative error code.  tests/test_dataflow_queue.py replays
 * the queue on a dense matrix with numpy and checks the dependency order. */
int64_t okkt_debug_dataflow_queue(int32_t nfronts, const int32_t* f, const int32_t* k, int32_t workers, int32_t group,
                                  int32_t* tasks, int64_t cap, double* model_us);
/* Test hook, host only: the register and LDS maps of the update tasks of the dataflow launch (csrc/df_fragments.h), evaluated by the
 * functions the kernel itself uses.  map: 0 = the earlier map (column fragments 4 doubles apart, both operand images with leading
 * dimension 144), 1 = the contiguous map with the ring's own images, < 0 = the one this library's kernel was compiled with.  what:
 * 0 = column (inside the wave's 32) of accumulator group idx of a lane, 1 = column of its column-operand fragment idx, 2 = offset
 * (doubles, from the ring slot's first) of column-operand fragment idx of k-step kk, 3 = the same for row-operand fragment idx (0 .. 3),
 * 4 = rows by which the LDS-DMA rotates the panel column that the lane reads in k-step kk, 5 = geometry: idx 0 / 1 leading dimension of
 * the row / column operand image, 2 doubles per ring slot, 3 panel columns per slot, 4 slots, 5 the compiled-in map, 6 the kernel's LDS
 * bytes, 7 the per-step kernels' leading dimension.  Returns the value, or a negative error code.  tests/test_dataflow_fragments.py. */
int64_t okkt_debug_dataflow_fragment(int32_t map, int32_t what, int32_t wave, int32_t lane, int32_t kk, int32_t idx);

/* ---- Uniform batches: B systems on the analysed pattern of one handle ---------------------------------
 * A batch shares everything the analysis made -- the ordering, the front lists, the schedule, all index arrays on the device -- and
 * gives every item a slot of its own in HBM: a front arena, D, the diagonal shift, a line of pivot counters and the vectors of the
 * solve sweeps.  Every item is a complete factorisation: its own values, its own shift, its own inertia and flag, no early exit; one
 * item's zero or non-finite pivots are counted in that item alone.  Supported for plans whose fronts are ALL small fronts (order <=
 * small_front_max, at most 136): those fronts are factored by one workgroup each with the front in LDS, so a batch is the same
 * per-front device code on a grid with one more coordinate.  Item b's factor is bit for bit what okkt_factor of the same values (and
 * shift) leaves on a fresh handle, and its solution with nrhs columns bit for bit okkt_solve's with the same nrhs.
 * Two launch shapes.  Level mode: one launch per level of the task tree, grid = tasks of the level x B; the launch count does not
 * depend on B.  Item mode: one workgroup per item walks all tasks of the plan in schedule order -- one launch per factorisation and
 * one per group of up to four right-hand sides.  No workgroup of either mode waits for another inside a launch.  OKKT_BATCH_AUTO
 * is level mode (no measured batch size at which item mode pays); okkt_batch_set_mode forces a mode on the
 * handle, and where it has not, the environment variable OKKT_BATCH_MODE (1 = level, 2 = item; read by okkt_batch_reserve) does.
 * okkt_batch_query: host only, also on host_symbolic_only handles.  eligible = 0 comes with the first reason that applies, in the
 * order of the codes below.  bytes_per_item: HBM of one slot with solve work for nrhs_max columns (the sweeps carry up to four at a
 * time); before the device plan exists the arena is counted as dense f x f buffers (okkt_stats.arena_bytes), an upper bound.
 * levels / tasks_per_item: levels and workgroup tasks of the task tree.  launches_*: kernel launches of one okkt_factor_batch, and of
 * one okkt_solve_batch per group of up to four right-hand sides, in each mode.
 * okkt_batch_reserve allocates B slots (index arrays are never duplicated) and replaces a previous reservation; OKKT_ERR_ALLOC with
 * a message when B x bytes_per_item does not fit, OKKT_ERR_INVALID with the reason when the plan is not eligible, for B outside
 * 1..65535 or nrhs_max < 1; OKKT_ERR_NO_DEVICE on host_symbolic_only handles.  A re-analysis releases the slots, and so does
 * okkt_dist_set_partition; a reservation whose device plan has been rebuilt on another footing since (a partition, a Schur set) is
 * released by the next batch call, which returns OKKT_ERR_INVALID.
 * okkt_factor_batch(_dev): item b reads nzval + b * val_stride (val_stride = 0: every item the same array; else >= nnz).  shift: host
 * array of B entries or NULL; shift[b] is added to the first nshift diagonal entries in the original numbering, as okkt_kkt_factor's
 * delta is.  inertia_out[b] / flag_out[b] (host, either may be NULL): what okkt_factor would have reported and returned (1 / 0) for
 * that item.  Returns OKKT_OK or a negative status.  The handle's own factor is not touched.
 * okkt_solve_batch(_dev): rhs and sol are [B][nrhs][dim]; nrhs <= the reserved nrhs_max; rhs may alias sol.  Needs a batch factored
 * with the same B or a larger one.
 * okkt_batch_select(b): slot b -> the handle's own numeric state (L panels, D, the shift, the inertia, the factored flag); afterwards
 * every entry point behaves as after okkt_factor of that item's values and shift. */
#define OKKT_BATCH_OK 0
#define OKKT_BATCH_NOT_ANALYZED 1
#define OKKT_BATCH_PARTITIONED 2
#define OKKT_BATCH_SCHUR 3
#define OKKT_BATCH_SCALING 4
#define OKKT_BATCH_BIG_FRONTS 5
#define OKKT_BATCH_AUTO 0
#define OKKT_BATCH_LEVEL 1
#define OKKT_BATCH_ITEM 2
typedef struct {
  int32_t eligible, reason;
  int64_t bytes_per_item;
  int64_t tasks_per_item;
  int32_t levels, max_front;
  int32_t launches_factor_level, launches_solve_level;
  int32_t launches_factor_item, launches_solve_item;
} okkt_batch_info;
int okkt_batch_query(okkt_handle h, int64_t nrhs_max, okkt_batch_info* out);
int okkt_batch_reserve(okkt_handle h, int64_t B, int64_t nrhs_max);
int okkt_batch_release(okkt_handle h);
int okkt_batch_set_mode(okkt_handle h, int mode /* OKKT_BATCH_AUTO / _LEVEL / _ITEM */);
int okkt_batch_mode_used(okkt_handle h);      /* the mode of the last okkt_factor_batch (0 before the first) */
int okkt_factor_batch(okkt_handle h, int64_t B, const double* nzval, int64_t val_stride, const double* shift /* [B] or NULL */,
                      int64_t nshift, int64_t n, int64_t m, int sym_kind, okkt_inertia* inertia_out /* [B] or NULL */,
                      int32_t* flag_out /* [B] or NULL */);
int okkt_factor_batch_dev(okkt_handle h, int64_t B, const double* d_nzval, int64_t val_stride, const double* shift /* host */,
                          int64_t nshift, int64_t n, int64_t m, int sym_kind, okkt_inertia* inertia_out /* host */,
                          int32_t* flag_out /* host */);
int okkt_solve_batch(okkt_handle h, int64_t B, const double* rhs, double* sol, int64_t nrhs);
int okkt_solve_batch_dev(okkt_handle h, int64_t B, const double* d_rhs, double* d_sol, int64_t nrhs);
int okkt_batch_select(okkt_handle h, int64_t b);

/* ---- Scenario batches: Schur-complement decomposition of B blocks on one pattern -------------------------
 * The handle is in Schur mode (okkt_set_schur before okkt_analyze) and its analysed pattern [[A11 A12]; [A21 A22]] is shared by B items
 * with values of their own.  The target is the arrowhead system
 *     A11_b x_b + A12_b x_L = b_b   (b = 0 .. B-1),      sum_b A21_b x_b + A0 x_L = b_L,
 * the KKT system of a two-stage stochastic programme, a scenario-tree MPC or a multi-start with shared variables: every item factors
 * its A11 and assembles its S_b = A22_b - A21_b A11_b^-1 A12_b, the S_b are summed on the device, and one dense Bunch-Kaufman factor of
 * sum_b S_b (+ S_add) solves the linking system.  (A0 is sum_b A22_b + S_add: give the linking block once as S_add with zero A22
 * values in the items, or spread over the items' A22.)  No host round trip per item.
 * Eligible: analysed, not partitioned, a Schur set, every INTERIOR front a small front (order <= small_front_max, at most 136; the
 * Schur front itself is assembled, never factored, and exempt), ns <= 2048 (the bound of the column-in-LDS assembly).  Item b's
 * factor, D, counts, S_b and condensed right-hand side are bit for bit what okkt_factor_schur / okkt_get_schur / okkt_schur_condense
 * give for its values on a fresh handle.
 * The order of the sums is part of the interface and depends neither on the device nor on ns: with G = ceil(B / OKKT_SBATCH_GROUP),
 * P_g is the sequential sum, starting from 0.0, over the items OKKT_SBATCH_GROUP * g .. min(OKKT_SBATCH_GROUP * (g + 1), B) - 1 in
 * item order, the sum is ((P_0 + P_1) + ... + P_{G-1}), and the caller's addend (S_add, rhs0) is added last.  The sum of the S_b is
 * bitwise symmetric.  No atomics.
 * Scenario batches run in LEVEL MODE ONLY (one launch per level of the interior's task tree, grid = tasks x B): the one-workgroup-
 * per-item solve cannot be interrupted for the dense solve, and no batch size was found at which item mode pays.  okkt_batch_set_mode
 * and OKKT_BATCH_MODE do not apply.  No workgroup waits for another inside a launch; every dependency is a launch boundary.
 * okkt_schur_batch_query: host only, also on host_symbolic_only handles; eligible = 0 comes with the first reason that applies, in the
 * order of the codes below.  bytes_per_item: the slot of okkt_batch_query plus the item's right-hand side of the linking system and
 * its share of the group partials (a started group is allocated whole); bytes_shared: the sum, r2 / x2 for four columns and the
 * batch's own dense factor.  levels / tasks_per_item / max_front: of the interior.  launches_factor: the shifts and counters, one
 * launch per level, the Schur fronts.  launches_solve: the batch's own launches of one fused solve per group of up to four right-hand
 * sides (gather, the levels upwards, the items' r2, the two stages of their sum, the put, the levels downwards, scatter); the launches
 * of the dense solve between them depend on ns and are not counted.
 * okkt_batch_query / okkt_batch_reserve keep answering OKKT_BATCH_SCHUR for such a handle.
 * okkt_schur_batch_reserve(B in 1..65535, nrhs_max >= 1) replaces a previous reservation; a re-analysis, a partition, a changed or
 * cleared set release it, and every call compares the plan it finds with the one reserved for (a stale reservation is released and
 * the call refused).  The handle's own factor and its own dense factor (okkt_schur_factor) are not touched by any call but _select.
 * okkt_factor_schur_batch(_dev): arguments as okkt_factor_batch's, n1 + m1 = dim - ns as okkt_factor_schur's; the counts and flags
 * cover the dim - ns interior pivots of the item alone.
 * okkt_schur_batch_get(_dev)(b): S_b for b in 0 .. B-1, the sum for b = -1; full and symmetric, rows and columns in the order of the
 * set, column-major with leading dimension ld >= ns.
 * okkt_schur_batch_factor(_dev): the dense factor of sum_b S_b (+ S_add: ns x ns, full symmetric, its lower triangle is read, added
 * last; NULL: none).  inertia_total = sum_b inertia(A11_b) + inertia(S).  Returns 1 when no pivot of S is zero or non-finite, else 0
 * (the rule of okkt_schur_factor), or a negative status.
 * okkt_schur_batch_condense(_dev): rhs [B][nrhs][dim] -> r2_sum [nrhs][ns] = sum_b r2_b by the rule above, and r2_items [B][nrhs][ns]
 * (or NULL).  okkt_schur_batch_expand(_dev): the same x2 [nrhs][ns] is put into every item; sol [B][nrhs][dim].
 * okkt_schur_batch_solve(_dev): the fused solve -- one forward sweep over the interiors, r2 = (sum_b r2_b) + rhs0 (rhs0 [nrhs][ns] or
 * NULL, added last; the entries rhs[b][.][idx] are the items' shares of b_L and are summed with them), the dense solve, the put and
 * one backward sweep.  rhs may alias sol.  sol[b][.][idx] is x_L in every item.  Needs okkt_schur_batch_factor and the B of the
 * last okkt_factor_schur_batch.
 * okkt_schur_batch_select(b): slot b -> the handle's own numeric state; afterwards every entry point behaves as after
 * okkt_factor_schur of that item.
 * Refusals (OKKT_ERR_INVALID with the reason, the handle stays usable): no reservation, B outside 1 .. the reserved, a solve before
 * okkt_schur_batch_factor, nrhs above the reserved nrhs_max, null pointers, ld < ns, a scaling.  OKKT_ERR_NO_DEVICE on
 * host_symbolic_only handles.  Out of scope: refinement, GMRES, selected inversion on the batch (select an item, or use the routes
 * of a single handle). */
#define OKKT_SBATCH_OK 0
#define OKKT_SBATCH_NOT_ANALYZED 1
#define OKKT_SBATCH_PARTITIONED 2
#define OKKT_SBATCH_NO_SET 3
#define OKKT_SBATCH_BIG_FRONTS 4
#define OKKT_SBATCH_SET_TOO_LARGE 5
#define OKKT_SBATCH_GROUP 32
typedef struct {
  int32_t eligible, reason;
  int64_t ns;
  int64_t bytes_per_item, bytes_shared;
  int64_t tasks_per_item;
  int32_t levels, max_front;
  int32_t launches_factor, launches_solve;
} okkt_schur_batch_info;
int okkt_schur_batch_query(okkt_handle h, int64_t nrhs_max, okkt_schur_batch_info* out);
int okkt_schur_batch_reserve(okkt_handle h, int64_t B, int64_t nrhs_max);
int okkt_schur_batch_release(okkt_handle h);
int okkt_factor_schur_batch(okkt_handle h, int64_t B, const double* nzval, int64_t val_stride, const double* shift /* [B] or NULL */,
                            int64_t nshift, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* inertia_items /* [B] or NULL */,
                            int32_t* flag_items /* [B] or NULL */);
int okkt_factor_schur_batch_dev(okkt_handle h, int64_t B, const double* d_nzval, int64_t val_stride, const double* shift /* host */,
                                int64_t nshift, int64_t n1, int64_t m1, int sym_kind, okkt_inertia* inertia_items /* host */,
                                int32_t* flag_items /* host */);
int okkt_schur_batch_get(okkt_handle h, int64_t b, double* S, int64_t ld);
int okkt_schur_batch_get_dev(okkt_handle h, int64_t b, double* d_S, int64_t ld);
int okkt_schur_batch_factor(okkt_handle h, const double* S_add, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total);
int okkt_schur_batch_factor_dev(okkt_handle h, const double* d_S_add, int64_t ld, okkt_inertia* inertia_S, okkt_inertia* inertia_total);
int okkt_schur_batch_condense(okkt_handle h, int64_t B, const double* rhs, double* r2_sum, double* r2_items /* or NULL */, int64_t nrhs);
int okkt_schur_batch_condense_dev(okkt_handle h, int64_t B, const double* d_rhs, double* d_r2_sum, double* d_r2_items, int64_t nrhs);
int okkt_schur_batch_expand(okkt_handle h, int64_t B, const double* rhs, const double* x2, double* sol, int64_t nrhs);
int okkt_schur_batch_expand_dev(okkt_handle h, int64_t B, const double* d_rhs, const double* d_x2, double* d_sol, int64_t nrhs);
int okkt_schur_batch_solve(okkt_handle h, int64_t B, const double* rhs, const double* rhs0 /* or NULL */, double* sol, int64_t nrhs);
int okkt_schur_batch_solve_dev(okkt_handle h, int64_t B, const double* d_rhs, const double* d_rhs0, double* d_sol, int64_t nrhs);
int okkt_schur_batch_select(okkt_handle h, int64_t b);


/* ---- multi-GPU: subtree-to-GPU sharding of ONE factorisation (one process per GPU) -------------------
 * No reference counterpart (the reference is single-process).  Every rank analyses the same
 * pattern and calls okkt_dist_set_partition(nparts, its part id): disjoint elimination-tree subtrees are
 * assigned to the parts (flop-balanced, deterministic), the ancestors of the cut ("top") to part 0.  The
 * caller moves three flat device buffers between ranks with its own collective (RCCL reduce / broadcast):
 *   factor: okkt_dist_factor_local -> okkt_dist_cb(buf, 0) [reduce(sum) to part 0] okkt_dist_cb(buf, 1) ->
 *           okkt_dist_factor_top (part 0) -> okkt_dist_counts [all-reduce(sum)] -> okkt_dist_finish -> 1/0
 *   solve : okkt_dist_solve_begin(rhs) -> okkt_dist_cv(buf, 0) [reduce(sum) to part 0] okkt_dist_cv(buf, 1) ->
 *           okkt_dist_solve_top (part 0) -> okkt_dist_x(buf, 0) on part 0 [broadcast] okkt_dist_x(buf, 1) ->
 *           okkt_dist_solve_end -> okkt_dist_x(sol, 2) [reduce(sum)]: the solution in original order.
 * Buffers must be zero before the pack calls (every slot has exactly one writer, the sum is exact).
 * A partitioned plan takes fronts of at most 46 000 rows (its f x f buffers keep 32-bit local offsets): with nparts > 1 and a
 * larger front okkt_dist_set_partition returns OKKT_ERR_INVALID (okkt_last_error says why); the single-GPU plan has no such limit. */
int okkt_dist_set_partition(okkt_handle h, int nparts, int part_id);
int okkt_dist_info(okkt_handle h, int64_t* cb_doubles, int64_t* cv_doubles, int64_t* n_boundary,
                   double* part_flops_out /* [nparts] or NULL */, double* top_flops_out);
int okkt_dist_get_owner(okkt_handle h, int64_t* sn_owner_out, int64_t* col_owner_out, int64_t* sn_parent_out);
int okkt_dist_factor_local(okkt_handle h, const double* d_nzval, int64_t n, int64_t m, int sym_kind);
int okkt_dist_cb(okkt_handle h, double* d_buf, int unpack);
int okkt_dist_factor_top(okkt_handle h);
int okkt_dist_counts(okkt_handle h, int64_t out[4]);
int okkt_dist_finish(okkt_handle h, const int64_t total[4]);
int okkt_dist_solve_begin(okkt_handle h, const double* d_rhs);
int okkt_dist_cv(okkt_handle h, double* d_buf, int unpack);
int okkt_dist_solve_top(okkt_handle h);
int okkt_dist_x(okkt_handle h, double* d_buf, int mode);
int okkt_dist_solve_end(okkt_handle h);

/* The same two sequences with the collectives INSIDE the library, on RCCL directly (ncclReduce / ncclBroadcast / ncclAllReduce
 * enqueued on the handle's stream between the kernels: no host synchronisation between the phases, one at the end) -- what a
 * Julia `linear_solver_HIP` uses when one process per GPU shares a factorisation; torch.distributed is not involved.
 * librccl is opened at run time (dlopen "librccl.so.1" / "librccl.so"; OKKT_RCCL_PATH overrides), so the library loads and the
 * single-GPU path works where RCCL is absent.  Protocol: one rank calls okkt_dist_unique_id and ships the 128 bytes to the
 * others by any means (MPI, a file, torch's store); every rank then calls okkt_dist_set_partition(nranks, rank) and
 * okkt_dist_comm_init(h, nranks, rank, id).  okkt_dist_factor returns the same 1 / 0 flag and the same summed pivot counts
 * on every rank; okkt_dist_solve leaves the whole solution (original order) in d_sol on every rank. */
int okkt_dist_unique_id(void* id_out /* 128 bytes */);
int okkt_dist_comm_init(okkt_handle h, int nranks, int rank, const void* id /* 128 bytes */);
int okkt_dist_comm_destroy(okkt_handle h);
int okkt_dist_factor(okkt_handle h, const double* d_nzval, int64_t n, int64_t m, int sym_kind, okkt_inertia* inertia_out);
int okkt_dist_solve(okkt_handle h, const double* d_rhs, double* d_sol);

/* ---- level 2: device-resident KKT system solver ----------------------------------------- */
typedef struct {
  double delta_start, delta_min, delta_max, delta_inc, delta_dec, delta_zero; /* parameters.jl:147-158 */
  int32_t ItRefine_Num;   /* parameters.jl:20 (3) -- Schur refinement rounds (first one is the plain solve) */
  int32_t max_it;         /* delta_strategy.jl:40 (500) */
} okkt_kkt_pars;

/* device times (HIP events on the handle's stream) of the phases of the last calls, milliseconds; 0 = not run yet.
 * what the reference's class_advanced_timer labels "SCHUR/form_system",
 * "SCHUR/delta_vecs", "<ls>/factorize", "KKT/rhs", "<ls>/ls_solve", "SCHUR/iterative_refinement/residual",
 * "SCHUR/kkt_err" measure on the host */
typedef struct {
  double assemble_ms;      /* okkt_kkt_form_system: kernels only (after the H, J, s, y uploads) */
  double upload_ms;        /* ... the host -> device copies of that call */
  double shift_ms;         /* okkt_kkt_factor: the delta shift (update_delta_vecs!) */
  double factor_ms;        /* ... the numeric factorisation */
  double rhs_ms;           /* okkt_kkt_system_rhs kernels */
  double solve_ms;         /* okkt_kkt_compute_direction: all triangular solves together */
  double refine_ms;        /* ... residual evaluations of the refinement rounds and the rhs / dy / ds vector work */
  double kkt_err_ms;       /* ... update_kkt_error! */
  double direction_ms;     /* ... the whole call on the device */
  int32_t n_solves;        /* triangular solves of the last direction */
  int32_t reserved;
} okkt_kkt_timers;

typedef struct {
  double error_D, error_P, error_mu, overall, rhs_norm, ratio; /* Class_kkt_error, kkt_system_solver.jl:49-65 */
} okkt_kkt_error;

int okkt_kkt_default_pars(okkt_kkt_pars* pars);
int okkt_kkt_create(okkt_kkt_handle* out, const okkt_opts* opts, int kkt_kind);
int okkt_kkt_destroy(okkt_kkt_handle k);
const char* okkt_kkt_last_error(okkt_kkt_handle k);
/* the underlying linear-solver handle (for stats / permutation queries) */
okkt_handle okkt_kkt_linear_solver(okkt_kkt_handle k);
/* structure of the iterate cache (Class_iterate.jl:4-20): H n x n CSC lower triangle only
 * (Class_cutest.jl:548), J m x n CSC.  Builds the pattern of Q or K, analyses it, builds maps.
 * Both must be canonical, as sparse() leaves them: row indices strictly increasing within every column.  A duplicated or
 * unsorted entry is refused, for every kind, with OKKT_ERR_INVALID and a message (okkt_kkt_last_error) naming the entry. */
int okkt_kkt_set_structure(okkt_kkt_handle k, int64_t n, int64_t m,
                           const int64_t* H_colptr, const int64_t* H_rowval,
                           const int64_t* J_colptr, const int64_t* J_rowval, int index_base);
/* form_system!: values of H and J and the point (s, y); computes schur_diag on the device */
int okkt_kkt_form_system(okkt_kkt_handle k, const double* H_nzval, const double* J_nzval,
                         const double* s, const double* y);
/* diag_min(kkt_solver) (kkt_system_solver.jl:291-294) */
int okkt_kkt_diag_min(okkt_kkt_handle k, double* out);
/* factor!(kkt_solver, delta): shift the first n diagonal entries by delta, refactor; 1 / 0 / <0.  Always a complete
 * factorisation (unless the linear-solver handle was created with opts.early_exit = 1 / okkt_set_early_exit): the
 * reference computes a direction from a factor! whose inertia flag was 0 after a failed step (one_phase.jl:231-242,
 * take_step2!), so the factor must exist whatever the flag says. */
int okkt_kkt_factor(okkt_kkt_handle k, double delta, okkt_inertia* inertia_out);
/* factor! as the delta loop uses it (delta_strategy.jl:37-114): a factorisation with the wrong inertia is thrown away by the
 * caller, so it may stop as soon as the pivot counts decide a failure (returns 0; a direction cannot be computed from it --
 * okkt_kkt_compute_direction then fails with OKKT_ERR_INVALID until the next complete factorisation).  A success is always
 * a complete factorisation.  okkt_kkt_ipopt_strategy uses this internally (OKKT_EARLY_EXIT=0 in the environment disables it). */
int okkt_kkt_factor_trial(okkt_kkt_handle k, double delta, okkt_inertia* inertia_out);
int okkt_kkt_get_timers(okkt_kkt_handle k, okkt_kkt_timers* out);
/* ipopt_strategy!: returns 1 on :success, 0 on :failure (delta > delta_max), <0 on error */
int okkt_kkt_ipopt_strategy(okkt_kkt_handle k, double delta_prev, const okkt_kkt_pars* pars,
                            int32_t* num_fac_out, double* delta_out);

/* ---- A Lanczos bound on lambda_min(H + J' Sigma J) for the delta loop ----
 * With Sigma = diag(y ./ s) > 0, K(delta) = [[H + delta I, J'], [J, -inv(Sigma)]] has inertia (n, m, 0) exactly when
 * Q(delta) = H + J' Sigma J + delta I is positive definite, and the Cholesky flag of the Schur kinds is decided by the same Q(delta).
 * For any v with Rayleigh quotient rho = v'Q(0)v / v'v every attempt with delta <= -rho fails.  okkt_kkt_min_eig finds such a v by at
 * most max_steps Lanczos steps (full reorthogonalisation) on Q(0) of the iterate of the last okkt_kkt_form_system, matrix-free from
 * the H, J and Sigma the handle holds (no delta; the same operator whatever the kind and schur_dense_rows).  scaled = 1 runs Lanczos on
 * D Q(0) D, d_i = 1 / sqrt(|schur_diag_i|) (1 where that entry is 0 or not finite); the certificate is taken on the unscaled Q(0)
 * with v = D w either way.  Two calls give the same bits.  The call uses a workspace of its own ((max_steps + 1) n doubles and a few
 * vectors, released with the handle): the resident right-hand side and direction and the handle's work vectors are not touched.
 * Refused with OKKT_ERR_INVALID (okkt_kkt_last_error says why; the handle stays usable): the clever-symmetric kind, a call before
 * okkt_kkt_form_system, max_steps > 64, scaled other than 0 / 1, and n or a row / column of J or a row of H of 2^24 entries or more
 * (rho_margin would not cover the rounding of rho); host_symbolic_only handles get OKKT_ERR_NO_DEVICE. */
typedef struct {
  double theta_min, theta_max; /* extreme Ritz values of the operator Lanczos ran on (the scaled one when scaled = 1) */
  double bound;                /* |beta_k s_k1|: an eigenvalue of that operator lies within this of theta_min */
  double rho;                  /* Rayleigh quotient v'Q(0)v / v'v of the returned v on the UNSCALED Q(0), recomputed explicitly */
  double rho_abs;              /* (|v|'|H||v| + sum_i sigma_i (|J||v|)_i^2) / v'v: the scale of rho's rounding error */
  double rho_margin;           /* 2^-26 * rho_abs: attempts with delta <= -rho - rho_margin are certified to fail */
  double resid;                /* ||Q(0) v - rho v||_2 / ||v||_2, explicit */
  int32_t steps;               /* Lanczos steps taken */
  int32_t status;              /* 0 bound <= tol * |theta_min|, 1 step limit, 2 invariant subspace (beta = 0), 3 non-finite */
  double seconds_device;
} okkt_kkt_eig_info;
/* status 3: rho, rho_abs, rho_margin and resid are NaN and v_out is zero.  beta counts as 0 at 2^-44 of the largest Ritz value in
 * magnitude.  At most min(max_steps, n) steps are taken. */
int okkt_kkt_min_eig(okkt_kkt_handle k, int32_t max_steps /* 1..64, <= 0: 32 */, double tol /* <= 0: 2^-4 */,
                     int32_t scaled /* 0 / 1 */, okkt_kkt_eig_info* info, double* v_out /* [n] host, or NULL */);
/* okkt_kkt_ipopt_strategy with the same tau, first attempt, delta sequence, delta_max exit and completion of an early-exited last
 * trial, except that okkt_kkt_min_eig(max_steps, default tol, scaled) runs once, right after the first failed attempt, and an attempt
 * of the sequence with delta <= -rho - rho_margin and delta <= delta_max is not factored (nor scanned for diagonal dominance): it is
 * counted in skipped_out instead of num_fac_out.  An attempt with delta > delta_max is never skipped.  With status 3 or rho >= 0
 * nothing is skipped.  Status, delta_out and the factor left behind are those of okkt_kkt_ipopt_strategy.  info (or NULL): the
 * estimate; steps = 0 when Lanczos never ran.  Refusals as okkt_kkt_min_eig. */
int okkt_kkt_ipopt_strategy_eig(okkt_kkt_handle k, double delta_prev, const okkt_kkt_pars* pars,
                                int32_t max_steps, int32_t scaled,
                                int32_t* num_fac_out, double* delta_out, int32_t* skipped_out,
                                okkt_kkt_eig_info* info /* or NULL; steps = 0 when Lanczos never ran */);
/* The same loop with its attempts taken `width` (1 .. 64) at a time: the delta sequence is known in advance, so
 * a group of attempts is ONE okkt_factor_batch_dev on the formed values (val_stride = 0) with the candidates as shifts.  The first attempt
 * in sequence order that succeeds, or that exceeds delta_max, ends the loop, and its slot is selected into the handle: the status,
 * delta_out, the factor left behind, okkt_kkt_diag_dom_warnings and a following okkt_kkt_compute_direction are bit for bit those of
 * okkt_kkt_ipopt_strategy.  num_fac_out is the serial count (the index of the chosen attempt + 1), launches_out the number of batched
 * factorisations.  Slots for `width` items are reserved on the linear solver's handle at the first call.  Refused with
 * OKKT_ERR_INVALID (okkt_kkt_last_error says why; the handle stays usable): the clever-symmetric kind, whose shift rewrites the values;
 * a plan that takes no batch (okkt_batch_query); the linear solver's scaling on; width out of range; a call before form_system.
 * host_symbolic_only handles get OKKT_ERR_NO_DEVICE. */
int okkt_kkt_ipopt_strategy_batch(okkt_kkt_handle k, double delta_prev, const okkt_kkt_pars* pars, int32_t width,
                                  int32_t* num_fac_out, double* delta_out, int32_t* launches_out);
/* ---- KKT batches: form, delta-correct and solve B iterates on one structure ----
 * B iterates (H_b, J_b, s_b, y_b, grad_b, cons_b) share the structure of the handle; every one gets a slot of its own in HBM (its
 * values, Sigma, the assembled matrix, the resident rhs and direction, work vectors; index arrays are never duplicated) and a slot of
 * the linear solver's uniform batch.  One rule for every item: its observable results -- diag_min; status, number of factorisations,
 * delta and diagonal-dominance warnings of the delta loop; inertia and flag; the rhs triple; dx, dy, ds and the six numbers of
 * okkt_kkt_error -- are bit for bit those of okkt_kkt_form_system, okkt_kkt_diag_min, okkt_kkt_factor / okkt_kkt_ipopt_strategy,
 * okkt_kkt_system_rhs (J_nzval_cur = NULL) and okkt_kkt_compute_direction (resident rhs) for that iterate on a handle of its own.
 * (okkt_kkt_ipopt_strategy_batch batches the delta CANDIDATES of one iterate; this family batches iterates.)
 * Strides: H_stride / J_stride = 0: every item reads the same array; otherwise >= the number of entries.  s, y, grad, cons, the rhs
 * triple and dx, dy, ds are [B][m] / [B][n], items contiguous.
 * okkt_kkt_items_ipopt_strategy: tau_b, the first attempt and the sequence come from diag_min_b and delta_prev[b] as in
 * okkt_kkt_ipopt_strategy; in every round each item still active makes its next attempt, and a round is ONE batched factorisation over
 * the active items only.  An item leaves at its first success (status 1) or at its first attempt beyond delta_max (status 0) and keeps
 * that complete factor in its slot: an item with status 0 still gives a direction, as in the reference (take_step2!).  launches_out is
 * the number of rounds = max_b num_fac_out[b].  After every failed attempt the scan of okkt_kkt_is_diag_dom runs for the failed items
 * as batched launches (OKKT_DIAG_DOM_SCAN=0 is honoured).  Batched factorisations are always complete.
 * okkt_kkt_items_compute_direction: dx = dy = ds = NULL leaves the directions resident.  One host synchronisation per call.
 * okkt_kkt_items_select(b): slot b -> the handle's own state (the iterate's device arrays, Sigma, schur_diag and the assembled values,
 * delta, the resident rhs and direction where they exist, the linear solver's slot through okkt_batch_select): afterwards every
 * single-iterate entry point behaves as after the serial sequence on that iterate.
 * Scope: the symmetric kind and the Schur kind without dense rows.  okkt_kkt_items_query (host only) gives eligible = 0 with the first
 * reason that applies, in the order of the codes; OKKT_KKT_ITEMS_PLAN + r passes on reason r of okkt_batch_query.  launches_form /
 * launches_direction: kernel launches of one form_system / compute_direction (the Schur kind's for the default ItRefine_Num); they do
 * not depend on B.  bytes_per_item includes the linear solver's slot and counts the values of H and J per item (an upper bound: an
 * array given with stride 0 is held once).  Every entry point refuses a handle that is not eligible with
 * OKKT_ERR_INVALID and a message (okkt_kkt_last_error); the handle stays usable and the single-iterate calls are untouched.  Calls out of
 * order (a direction before a factorisation, a factorisation or a rhs before form_system, B above the reservation) get
 * OKKT_ERR_INVALID; host_symbolic_only handles OKKT_ERR_NO_DEVICE.  okkt_kkt_items_reserve (B in 1 .. 65535) replaces a previous
 * reservation and reserves B slots of the linear solver (okkt_batch_reserve); OKKT_ERR_ALLOC with a message when they do not fit.
 * okkt_kkt_items_release frees the slots of both levels (the linear solver's only while they are still the ones this reservation made:
 * another okkt_batch_reserve on that handle -- okkt_kkt_ipopt_strategy_batch makes one -- replaces them, and the items calls then ask for
 * a new reservation).  The structure of a KKT handle is set once (a second okkt_kkt_set_structure is refused and changes nothing), so a
 * reservation lives until it is released, replaced or the handle is destroyed. */
#define OKKT_KKT_ITEMS_OK 0
#define OKKT_KKT_ITEMS_NO_STRUCTURE 1
#define OKKT_KKT_ITEMS_CLEVER 2
#define OKKT_KKT_ITEMS_SCHUR_DIRECT 3
#define OKKT_KKT_ITEMS_DENSE_ROWS 4
#define OKKT_KKT_ITEMS_SCALING 5
#define OKKT_KKT_ITEMS_LS_REFINE 6
#define OKKT_KKT_ITEMS_PLAN 16      /* + the reason of okkt_batch_query */
typedef struct { int32_t eligible, reason; int64_t bytes_per_item; int32_t launches_form, launches_direction; } okkt_kkt_items_info;
int okkt_kkt_items_query(okkt_kkt_handle k, okkt_kkt_items_info* out);            /* host only */
int okkt_kkt_items_reserve(okkt_kkt_handle k, int64_t B);                         /* 1..65535; replaces a previous reservation */
int okkt_kkt_items_release(okkt_kkt_handle k);
int okkt_kkt_items_form_system(okkt_kkt_handle k, int64_t B, const double* H_nzval, int64_t H_stride,
                               const double* J_nzval, int64_t J_stride, const double* s /* [B][m] */, const double* y /* [B][m] */);
int okkt_kkt_items_diag_min(okkt_kkt_handle k, int64_t B, double* out /* [B] */);
int okkt_kkt_items_factor(okkt_kkt_handle k, int64_t B, const double* delta /* [B] */, okkt_inertia* inertia_out /* [B] or NULL */,
                          int32_t* flag_out /* [B] or NULL */);
int okkt_kkt_items_ipopt_strategy(okkt_kkt_handle k, int64_t B, const double* delta_prev /* [B] */, const okkt_kkt_pars* pars,
                                  int32_t* status_out /* [B]: 1 success, 0 failure */, int32_t* num_fac_out /* [B] */,
                                  double* delta_out /* [B] */, int32_t* diag_dom_warnings_out /* [B] or NULL */, int32_t* launches_out);
int okkt_kkt_items_system_rhs(okkt_kkt_handle k, int64_t B, const double* grad /* [B][n] */, const double* cons /* [B][m] */,
                              const double* s, const double* y, const double* mu /* [B] */, const double* a_norm_penalty /* [B] */,
                              double eta_P, double eta_D, double eta_mu,
                              double* dual_r, double* primal_r, double* comp_r /* [B][..] or NULL */);
int okkt_kkt_items_compute_direction(okkt_kkt_handle k, int64_t B, int32_t ItRefine_Num,
                                     double* dx /* [B][n] */, double* dy, double* ds /* [B][m]; three NULLs: stay resident */,
                                     okkt_kkt_error* err_out /* [B] or NULL */);
int okkt_kkt_items_select(okkt_kkt_handle k, int64_t b);
/* ---- Line-search batches: step sizes and predicted reductions for the items of a KKT batch ----
 * The step-side functions (okkt_kkt_max_step_primal, okkt_kkt_s_bound_ok, okkt_kkt_dual_step_range, okkt_kkt_predicted_reduction,
 * okkt_kkt_dual_step) for B items of a reservation at once, against each item's formed iterate and resident direction in its slot: the
 * direction okkt_kkt_items_compute_direction left, or the triples of okkt_kkt_items_set_direction (which covers B items as
 * okkt_kkt_set_direction covers one; okkt_kkt_items_select(b) afterwards leaves the handle as okkt_kkt_set_direction would).  One rule:
 * every output for item b is bit for bit what the matching single-iterate call returns for that iterate and direction on a KKT handle of
 * its own -- NaN propagation, the reset semantics of dual_bounds and the non-finite fallback (0, -1) included.
 * Per-item scalars are arrays [B], per-item vectors [B][m] or [B][n], items contiguous.  items / nitems is the optional item list:
 * items == NULL means every slot 0 .. B-1; otherwise items[0 .. nitems) are distinct slots below B, inputs and outputs stay indexed by
 * slot, only listed slots are read and only their outputs written (a backtracking loop keeps calling with the items still in it);
 * nitems == 0 is OKKT_OK and writes nothing.  frac_stride = 0: one fraction vector for every item, else m.  okkt_kkt_items_dual_step:
 * J_nzval_cand = NULL reads each item's formed J, J_stride = 0 one candidate array for every item, else >= the number of entries; for
 * dual_ls other than 1 or 3 step_size_D[b] = ub[b] and nothing is launched.  okkt_kkt_items_dual_step_range runs a second pass over
 * the items in which an entry with dy == 0 reset the interval.  One host synchronisation per pass, one more when norm(dx_b, Inf) of the
 * directions is not cached yet (once per direction).  The line-search slots (okkt_kkt_items_ls_info.extra_bytes_per_item) are
 * allocated by the first of these calls after a reservation -- OKKT_ERR_ALLOC with a message when they do not fit -- and freed with it.
 * Refusals: those of the family (an ineligible handle, a missing or replaced reservation: OKKT_ERR_INVALID; host_symbolic_only:
 * OKKT_ERR_NO_DEVICE), and OKKT_ERR_INVALID with a message, the handle staying usable, for B above the items of the last
 * okkt_kkt_items_form_system, a direction call before it, a step call with B above the items that hold a direction ("no direction:
 * ..."), a NULL required array, a slot in items out of range or listed twice, frac_stride other than 0 or m.
 * okkt_kkt_items_ls_query (host only): eligible / reason as okkt_kkt_items_query, the extra HBM of one item, and the kernel launches of
 * the norm pass and of each of the five calls (they do not depend on B; launches_dual_range counts one pass). */
typedef struct {
  int32_t eligible, reason;
  int64_t extra_bytes_per_item;
  int32_t launches_dx_norm, launches_max_step, launches_s_bound, launches_dual_range, launches_predicted_reduction, launches_dual_step;
} okkt_kkt_items_ls_info;
int okkt_kkt_items_set_direction(okkt_kkt_handle k, int64_t B, const double* dx /* [B][n] */, const double* dy, const double* ds /* [B][m] */);
int okkt_kkt_items_max_step_primal(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* frac_bd_predict,
                                   int64_t frac_stride /* 0 or m */, double ex, double* step_size_P /* [B] */, double* dx_norm_inf /* [B] or NULL */);
int okkt_kkt_items_s_bound_ok(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* s_new /* [B][m] */,
                              const double* frac_bd, int64_t frac_stride, double ex, int32_t* ok /* [B] */);
int okkt_kkt_items_dual_step_range(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* s_cand, const double* y_cand /* [B][m] */,
                                   const double* mu_cand /* [B] */, double comp_feas, const double* frac_bd, int64_t frac_stride,
                                   double* lb /* [B] */, double* ub /* [B] */);
int okkt_kkt_items_predicted_reduction(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* grad /* [B][n] */,
                                       const double* mu, const double* dmu, const double* a_norm_penalty, const double* step_size /* [B] each */,
                                       double* out /* [B][4] */);
int okkt_kkt_items_dual_step(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* J_nzval_cand /* or NULL */,
                             int64_t J_stride /* 0: shared */, const double* grad_cand /* [B][n] */, const double* s_cand, const double* y_cand /* [B][m] */,
                             const double* mu_cand, const double* a_norm_penalty, const double* step_size_P, const double* lb, const double* ub,
                             const double* scale_D, const double* scale_mu /* [B] each */, int dual_ls, double* step_size_D /* [B] */);
int okkt_kkt_items_ls_query(okkt_kkt_handle k, okkt_kkt_items_ls_info* out);      /* host only */
/* Test hook: one batched factorisation of the reserved KKT batch over the item list items[0 .. nitems) (distinct slots below B) with the
 * shifts delta[slot], as a round of okkt_kkt_items_ipopt_strategy runs it; flag_out [B] is written for the listed slots only. */
int okkt_debug_kkt_items_factor_list(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* delta /* [B] */,
                                     int32_t* flag_out /* [B] */);
/* Test hook, host only (no device, no handle): the attempt sequence and the round bookkeeping of okkt_kkt_items_ipopt_strategy
 * (csrc/kkt_items_seq.h) for B items whose attempt with delta succeeds exactly when delta >= need[b]; outputs as the loop's. */
int okkt_debug_items_loop_model(int64_t B, const double* diag_min, const double* delta_prev, const double* need, const okkt_kkt_pars* pars,
                                int32_t* status_out, int32_t* num_fac_out, double* delta_out, int32_t* launches_out);
/* Test hook, host only (no device, no handle): the tridiagonal solver of okkt_kkt_min_eig (csrc/lanczos_tridiag.h) on
 * T = tridiag(beta[0 .. k-2]; alpha[0 .. k-1]), 1 <= k <= 64.  beta holds k entries: beta[k-1] is the residual coefficient beta_k of
 * the Lanczos recurrence.  Returns theta_min, theta_max, the unit eigenvector s_out [k] of theta_min (largest entry positive) and
 * bound = |beta[k-1] s_out[k-1]|.  OKKT_ERR_INVALID for k out of range, a NULL pointer or a non-finite entry. */
int okkt_debug_tridiag_eig(int32_t k, const double* alpha, const double* beta, double* theta_min, double* theta_max,
                           double* s_out, double* bound);
/* compute_direction! for nrhs reduction-factor triples in one pass over the factor: the probe of the aggressive step
 * (Reduct_affine, take_step.jl:2-3) and the candidates of take_step2! (take_step.jl:34-66) share the factorised system.
 * System_rhs (system_rhs.jl:57-73) is evaluated on the device for every triple from the iterate of the last okkt_kkt_system_rhs;
 * the triangular solves (and the Schur refinement rounds) carry up to four right-hand sides per sweep over L.
 * etas: nrhs x (eta_P, eta_D, eta_mu); dx: nrhs x n, dy, ds: nrhs x m (NULL: not downloaded); err: nrhs records or NULL.
 * Schur, Schur-direct and symmetric systems; 1 <= nrhs <= 16. */
int okkt_kkt_compute_directions(okkt_kkt_handle k, int32_t nrhs, const double* etas, int32_t ItRefine_Num,
                                double* dx, double* dy, double* ds, okkt_kkt_error* err);
/* is_diag_dom(kkt_solver.Q[1:n,1:n]) (delta_strategy.jl:1-9) at the delta of the last factor call, as a device scan:
 * *out = 1 dominant, 0 not, -1 not evaluated (clever-symmetric system).  ipopt_strategy! runs it after every failed attempt and
 * prints "WARNING: Inertia calculation incorrect" when it holds (delta_strategy.jl:94-98): okkt_kkt_ipopt_strategy does the same
 * scan and okkt_kkt_diag_dom_warnings returns how many of its failed attempts would have printed the warning. */
int okkt_kkt_is_diag_dom(okkt_kkt_handle k, int32_t* out);
int okkt_kkt_diag_dom_warnings(okkt_kkt_handle k, int32_t* count);
/* the tail of estimate_y_tilde (guess-vars.jl:155-160) with the factor and the Jacobian of the handle: y = -J (F \ (-g)) */
int okkt_kkt_estimate_y_tilde(okkt_kkt_handle k, const double* g, double* y_out);
/* System_rhs(it, reduct) (system_rhs.jl:57-73): dual_r = -(grad - J'y + eta_mu*mu*pen*J'1)(1 - eta_D),
 * primal_r = -(cons - s)(1 - eta_P), comp_r = eta_mu*mu - s.*y, at the CURRENT iterate.  J_nzval_cur = NULL
 * uses the J values of the factorised iterate (form_system) */
int okkt_kkt_system_rhs(okkt_kkt_handle k, const double* J_nzval_cur, const double* grad, const double* cons,
                        const double* s, const double* y, double mu, double a_norm_penalty,
                        double eta_P, double eta_D, double eta_mu, double* dual_r, double* primal_r, double* comp_r);
/* compute_direction!: rhs triple (dual_r[n], primal_r[m], comp_r[m]) -> (dx[n], dy[m], ds[m]) + N err.
 * dual_r = primal_r = comp_r = NULL: the rhs that the last okkt_kkt_system_rhs left on the device (no copy);
 * dx = dy = ds = NULL: the direction stays on the device only (step-side functions, okkt_kkt_get_direction).
 * OKKT_KKT_SCHUR_DIRECT reads s, y and J of the iterate of the last okkt_kkt_system_rhs (current_it). */
int okkt_kkt_compute_direction(okkt_kkt_handle k, const double* dual_r, const double* primal_r,
                               const double* comp_r, int32_t ItRefine_Num,
                               double* dx, double* dy, double* ds, okkt_kkt_error* err_out);
int okkt_kkt_get_direction(okkt_kkt_handle k, double* dx, double* dy, double* ds);
/* the assembled matrix values in the order of the analysed pattern (tests), and schur_diag */
int okkt_kkt_get_matrix(okkt_kkt_handle k, int64_t* dim_out, int64_t* nnz_out,
                        int64_t* colptr_out, int64_t* rowval_out, double* nzval_out);
int okkt_kkt_get_schur_diag(okkt_kkt_handle k, double* out /* [n] */);
/* the rows of J that opts.schur_dense_rows took out of the Schur complement (valid after okkt_kkt_set_structure): their count and,
 * unless rows_out is NULL, the rows themselves (0-based, ascending).  The factorised matrix (okkt_kkt_get_matrix) then has order n + count,
 * the inertia okkt_kkt_factor reports is its inertia and the flag is 1 exactly for (n, count, 0, 0), every pivot counted with tolerance 0;
 * okkt_kkt_get_schur_diag and okkt_kkt_diag_min keep describing diag(Q) of the whole Q. */
/* OKKT_KKT_SYMMETRIC only: the triangular solve of okkt_kkt_compute_direction(s) becomes okkt_solve_refine against the assembled,
 * shifted K that was factored (max_steps corrections at most, stop at omega <= tol, tol <= 0: 2^-52).  max_steps = 0 (the default)
 * leaves the plain solve.  The other kinds refine through ItRefine_Num and refuse it with OKKT_ERR_INVALID. */
int okkt_kkt_set_ls_refine(okkt_kkt_handle k, int32_t max_steps, double tol);
/* okkt_condest for the system okkt_kkt_factor last factored: K with delta on its H block (symmetric kind); M as scaled and factored
 * (clever-symmetric kind); Q + delta I (Schur kinds); with schur_dense_rows on, the bordered A (order n + k): then cond1 is kappa_1 of A,
 * not of Q.  Refused (OKKT_ERR_INVALID) before a complete factorisation. */
int okkt_kkt_condest(okkt_kkt_handle k, int32_t t, okkt_condest_info* info);
/* okkt_eigs for the system okkt_kkt_factor last factored: the eigenvalues of smallest modulus of
 * Q(delta) = H + J' Sigma J + delta I at the factored delta and the x-parts of their vectors (vecs_x: n x nev, or NULL).  nlead is set
 * here (opts->nlead is ignored): the pencil with nlead = n where the factored matrix is larger than Q (the symmetric kind with m > 0,
 * the Schur kinds with schur_dense_rows), else the standard problem.  resid holds the true residuals against the assembled values
 * with delta on the H block.  Refused (OKKT_ERR_INVALID): before a complete factorisation, and the clever-symmetric kind, whose
 * factored matrix is rescaled and reduced. */
int okkt_kkt_eigs(okkt_kkt_handle k, const okkt_eigs_opts* opts, double* lambda /* [nev] */, double* vecs_x /* [n x nev] or NULL */,
                  double* resid /* [nev] */, okkt_eigs_info* info /* or NULL */);
/* OKKT_KKT_SYMMETRIC only: the forward error bound (okkt_forward_error) of the last okkt_kkt_compute_direction's solve, against the
 * factored K + delta.  Refused until such a direction exists for the current factorisation and rhs; the other kinds refuse it as they
 * refuse okkt_kkt_set_ls_refine. */
int okkt_kkt_direction_error_bound(okkt_kkt_handle k, double* ferr);
int okkt_kkt_get_dense_rows(okkt_kkt_handle k, int64_t* count_out, int64_t* rows_out /* [count] or NULL */);
/* Schur, Schur-direct (with and without schur_dense_rows) and symmetric kinds: okkt_set_scaling on the level-1 handle, mode
 * OKKT_SCALE_RUIZ or OKKT_SCALE_NONE.  Every okkt_kkt_factor, okkt_kkt_factor_trial and attempt of
 * okkt_kkt_ipopt_strategy then computes the scaling from the shifted values it factors; directions, okkt_kkt_estimate_y_tilde,
 * okkt_kkt_condest and okkt_kkt_direction_error_bound keep describing the unscaled system.  Refused with OKKT_ERR_INVALID: the
 * clever-symmetric kind (it has okkt_kkt_set_rescale) and OKKT_SCALE_USER. */
int okkt_kkt_set_ls_scaling(okkt_kkt_handle k, int mode, int32_t sweeps);

/* ---- Clever_Symmetric only -------------------------------------------------------
 * initialize!(::Clever_Symmetric_KKT_solver, it) = compute_indicies(get_jac(it)) (clever_symmetric.jl:53-61,
 * 200-246): rows of J that are exact multiples of each other (same pattern, ||a_i - a_j * ratio||_2 < 1e-16)
 * are grouped on the host with the reference's ordering rule (compare_columns, :107-155); the reduced matrix
 * is analysed here.  Call once after okkt_kkt_set_structure and before the first okkt_kkt_form_system; the
 * grouping is kept for the life of the handle, as in the reference. */
int okkt_kkt_compute_indicies(okkt_kkt_handle k, const double* J_nzval, int64_t* m_new_out);
/* the grouping, 0-based: first_para_indicies [m_new] (sorted first rows = para_row_info[g].first),
 * group_ptr [m_new + 1], and per member in ls order: ind, ratio; after a form_system also u, g and the
 * group's combined u (update_indicies!, clever_symmetric.jl:262-287).  Any pointer may be NULL. */
int okkt_kkt_get_indicies(okkt_kkt_handle k, int64_t* first_para_indicies, int64_t* group_ptr, int64_t* member_ind,
                          double* member_ratio, double* member_u, double* member_g, double* group_u);
/* read-only, for tests: diag_rescale [n + m_new] of the last okkt_kkt_form_system and, of the last okkt_kkt_compute_direction,
 * symmetric_primal_rhs [m], the combined rhs of the groups [m_new], the refined solution of the scaled system [n + m_new] and
 * v [m_new], the group part of the unscaled solution (clever_symmetric.jl:417-474).  Any pointer may be NULL.  The last four are
 * refused (OKKT_ERR_INVALID) unless that direction is the last thing computed on the handle; the other kinds refuse the call. */
int okkt_kkt_get_clever_vectors(okkt_kkt_handle k, double* diag_rescale, double* symrhs, double* crhs, double* sol, double* v);
/* diag_rescale used by the next okkt_kkt_form_system: mode OKKT_RESCALE_*, mu = iter.point.mu,
 * x_norm_inf = norm(iter.point.x, Inf) (create_diag_rescale_*, clever_symmetric.jl:307-319); default NONE */
int okkt_kkt_set_rescale(okkt_kkt_handle k, int mode, double mu, double x_norm_inf);

/* ---- step-side vector kernels ---------------------------------------------------
 * The reductions and SpMVs simple_ls runs either side of a step (line_search.jl:36-199), on the state the
 * handle already holds: "iter" = the point (s, y) and J, H of the last okkt_kkt_form_system, "dir" = the
 * direction left on the device by the last okkt_kkt_compute_direction (an error if there is none).  Vector
 * arguments are host pointers of the stated length; min / max reductions propagate NaN as Julia's do and are
 * bit-exact, sums are taken in a fixed order (reproducible, not Julia's order). */
/* replace the resident direction (scale_direction of line_search.jl:10-19, corrections, tests): dx [n], dy, ds [m] */
int okkt_kkt_set_direction(okkt_kkt_handle k, const double* dx, const double* dy, const double* ds);
/* simple_max_step(iter.point.s, dir.s, lb_s_predict(iter, dir, pars)) (frac_boundary.jl:3-15,31-35;
 * line_search.jl:40-41); ex = pars.ls.fraction_to_boundary_predict_exp; also returns norm(dir.x, Inf) */
int okkt_kkt_max_step_primal(okkt_kkt_handle k, const double* frac_bd_predict /* [m] */, double ex,
                             double* step_size_P, double* dx_norm_inf);
/* all(s_new .>= lb_s(iter, dir, pars)) of move_primal (move.jl:15-17; frac_boundary.jl:22-28): 1 / 0 */
int okkt_kkt_s_bound_ok(okkt_kkt_handle k, const double* s_new /* [m] */, const double* frac_bd /* [m] */, double ex,
                        int32_t* ok);
/* lb, ub = dual_bounds(candidate, candidate.point.y, dir.y, comp_feas); ub = min(ub, simple_max_step(
 * candidate.point.y, dir.y, lb_y(iter, dir, pars))) (move.jl:28-80; frac_boundary.jl:17-20;
 * line_search.jl:84-86), with the sequential semantics of the reference's loop */
int okkt_kkt_dual_step_range(okkt_kkt_handle k, const double* s_cand /* [m] */, const double* y_cand /* [m] */,
                             double mu_cand, double comp_feas, const double* frac_bd /* [m] */, double* lb, double* ub);
/* out = { phi_predicted_reduction_primal_dual, norm(comp(iter), Inf), norm(comp_predicted(iter, dir, step), Inf),
 * merit_function_predicted_reduction } (eval.jl:11-13,117-120,236-273); grad = get_grad(iter) [n], mu =
 * iter.point.mu, dmu = dir.mu, a_norm_penalty = iter.a_norm_penalty_par */
int okkt_kkt_predicted_reduction(okkt_kkt_handle k, const double* grad, double mu, double dmu, double a_norm_penalty,
                                 double step_size, double out[4]);
/* step_size_D of move_dual (move.jl:82-118) for move_primal_seperate_to_dual: dual_ls 1 / 3 = the least-squares
 * step on [scale_D * dual residual; -scale_mu * comp] clamped to [max(lb, min(ub, step_size_P)), ub], any other
 * dual_ls = ub.  The candidate: J_nzval_cand (pattern of okkt_kkt_set_structure; NULL = the J of form_system),
 * grad_cand [n], s_cand, y_cand [m] (y not yet moved), mu_cand */
int okkt_kkt_dual_step(okkt_kkt_handle k, const double* J_nzval_cand, const double* grad_cand, const double* s_cand,
                       const double* y_cand, double mu_cand, double a_norm_penalty, double step_size_P, double lb,
                       double ub, int dual_ls, double scale_D, double scale_mu, double* step_size_D);

#ifdef __cplusplus
}
#endif
#endif /* OKKT_H */
