# linear_solver_hip.jl -- Julia glue for libonephase_kkt.so (C ABI: include/okkt.h).
#
# UNTESTED IN THIS REPOSITORY: neither Julia nor the reference's dependencies are available in the
# build environment.  The file mirrors the reference's own plug-in pattern
# (src/linear_system_solvers/hsl.jl: a `mutable struct X <: abstract_linear_system_solver` in a file
# that `loadHSL`-style code `include`s at run time) and is what a maintainer of OnePhase.jl would
# drop into src/linear_system_solvers/ -- see INTEGRATION.md for the three edits around it.
#
# Every ccall below binds exactly one entry point of include/okkt.h; pointers are to Julia-owned
# arrays that are GC.@preserve'd for the duration of the (blocking) call.

const OKKT_LIB = get(ENV, "ONEPHASE_KKT_LIB", "libonephase_kkt")

struct OkktInertia
    pos::Int64
    neg::Int64
    zero::Int64
    nonfinite::Int64
end

# okkt_opts of include/okkt.h, field for field (an isbits struct has C layout: six Int32, four Float64, four Int32 = 72 bytes)
struct OkktOpts
    device::Int32
    host_symbolic_only::Int32
    ordering::Int32
    relax_always::Int32
    relax_small::Int32
    relax_mid::Int32
    relax_small_frac::Float64
    relax_mid_frac::Float64
    relax_any_frac::Float64
    inertia_tol::Float64
    small_front_max::Int32
    panel_nb::Int32
    early_exit::Int32
    schur_dense_rows::Int32    # Schur kinds: 0 off, > 0 rows longer than this border the system, -1 automatic
end

function okkt_default_opts()
    o = Ref(OkktOpts(0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0))
    ccall((:okkt_default_opts, OKKT_LIB), Cint, (Ref{OkktOpts},), o)
    return o[]
end

# The back-end's own knobs ride in pars.kkt like the reference's `ma97_u` (parameters.jl:13,25 -> linear_solver_HSL(..., pars.kkt.ma97_u),
# kkt_system_solver.jl:247): the fields hip_device, hip_ordering, hip_relax_always / _small / _mid, hip_relax_small_frac / _mid_frac /
# _any_frac, hip_inertia_tol, hip_schur_dense_rows of Class_kkt_solver_options (INTEGRATION.md, edit 4), set through the existing plumbing, e.g.
# "kkt!hip_ordering" => 3 (create_pars_JuMP, JuMPinterface.jl:570-586).  -1 / 0.0 keep the library's default.
function okkt_opts_from_pars(kkt)
    d = okkt_default_opts()
    pick(v, dflt) = v > 0 ? v : dflt
    return OkktOpts(kkt.hip_device >= 0 ? Int32(kkt.hip_device) : d.device, d.host_symbolic_only,
                    kkt.hip_ordering != 0 ? Int32(kkt.hip_ordering) : d.ordering,
                    Int32(pick(kkt.hip_relax_always, d.relax_always)), Int32(pick(kkt.hip_relax_small, d.relax_small)), Int32(pick(kkt.hip_relax_mid, d.relax_mid)),
                    pick(kkt.hip_relax_small_frac, d.relax_small_frac), pick(kkt.hip_relax_mid_frac, d.relax_mid_frac), pick(kkt.hip_relax_any_frac, d.relax_any_frac),
                    kkt.hip_inertia_tol > 0 ? kkt.hip_inertia_tol : d.inertia_tol,
                    d.small_front_max, d.panel_nb, d.early_exit,
                    kkt.hip_schur_dense_rows != 0 ? Int32(kkt.hip_schur_dense_rows) : d.schur_dense_rows)
end

mutable struct linear_solver_HIP <: abstract_linear_system_solver
    handle::Ptr{Cvoid}
    sym::Symbol            # :definite (Cholesky semantics) or :symmetric (LDL', inertia from sign(D))
    safe_mode::Bool
    recycle::Bool
    inertia::OkktInertia
    opts::Union{Nothing,OkktOpts}      # nothing: okkt_create(NULL) = the library's defaults

    function linear_solver_HIP(sym::Symbol, safe_mode::Bool, recycle::Bool, opts::Union{Nothing,OkktOpts}=nothing)
        this = new()
        this.handle = C_NULL
        this.sym = sym
        this.safe_mode = safe_mode
        this.recycle = recycle
        this.inertia = OkktInertia(0, 0, 0, 0)
        this.opts = opts
        return this
    end
end

function okkt_error(solver::linear_solver_HIP, what::String, rc)
    msg = solver.handle == C_NULL ? "" : unsafe_string(ccall((:okkt_last_error, OKKT_LIB), Cstring, (Ptr{Cvoid},), solver.handle))
    error("$what failed with code $rc: $msg")
end

function initialize!(solver::linear_solver_HIP)
    if solver.handle == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = solver.opts === nothing ?
             ccall((:okkt_create, OKKT_LIB), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}), h, C_NULL) :             # NULL = default options
             ccall((:okkt_create, OKKT_LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{OkktOpts}), h, Ref(solver.opts))  # pars.kkt.hip_* (okkt_opts_from_pars)
        rc == 0 || error("okkt_create failed with code $rc (no HIP device? the KKT path has no CPU fallback)")
        solver.handle = h[]
        # Early exit stays OFF at this level: ls_factor! cannot know whether its caller will solve with a factorisation
        # whose flag is 0 -- the refactorisation after a failed step does (one_phase.jl:231-242 -> take_step2!).  A caller
        # that discards failed factors (a delta loop of its own) may switch it on around those calls:
        #   ccall((:okkt_set_early_exit, OKKT_LIB), Cint, (Ptr{Cvoid}, Cint), solver.handle, 1)
        finalizer(finalize!, solver)
    end
end

function finalize!(solver::linear_solver_HIP)
    if solver.handle != C_NULL
        ccall((:okkt_destroy, OKKT_LIB), Cint, (Ptr{Cvoid},), solver.handle)
        solver.handle = C_NULL
    end
end

function ls_factor!(solver::linear_solver_HIP, SparseMatrix::SparseMatrixCSC{Float64,Int64}, n::Int64, m::Int64, timer::class_advanced_timer)
    start_advanced_timer(timer, "HIP/factorize")
    A = SparseMatrix
    dim = size(A, 1)
    rc = 0
    inert = Ref(OkktInertia(0, 0, 0, 0))
    GC.@preserve A begin
        # pattern analysis is cached by pattern hash inside the library: free when only values changed
        rc = ccall((:okkt_analyze, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Cint),
                   solver.handle, dim, A.colptr, A.rowval, 1)
        rc == 0 || okkt_error(solver, "okkt_analyze", rc)
        kind = solver.sym == :definite ? 0 : (solver.sym == :symmetric ? 1 : error("this.options.sym = " * string(solver.sym) * " not supported"))
        rc = ccall((:okkt_factor, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Cint, Ref{OkktInertia}),
                   solver.handle, A.nzval, n, m, kind, inert)
    end
    pause_advanced_timer(timer, "HIP/factorize")
    rc < 0 && okkt_error(solver, "okkt_factor", rc)
    solver.inertia = inert[]
    return Int(rc)       # 1: inertia correct, 0: not (same contract as linear_solver_JULIA / linear_solver_HSL)
end

function ls_solve!(solver::linear_solver_HIP, my_rhs::Array{Float64,1}, my_sol::Array{Float64,1}, timer::class_advanced_timer)
    start_advanced_timer(timer, "HIP/ls_solve")
    GC.@preserve my_rhs my_sol begin
        rc = ccall((:okkt_solve, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64),
                   solver.handle, my_rhs, my_sol, 1)
        rc == 0 || okkt_error(solver, "okkt_solve", rc)
    end
    pause_advanced_timer(timer, "HIP/ls_solve")
end

struct OkktRefineInfo     # okkt_refine_info of include/okkt.h
    steps::Int32
    status::Int32        # 0 omega <= tol, 1 step limit, 2 stagnated, 3 non-finite
    omega0::Float64
    omega::Float64
    resid_inf::Float64
end

# sol = F \ rhs refined against A (its nzval in the analysed order; the factor may be of a nearby matrix): at most max_steps
# corrections from double-double residuals, stopping at a componentwise backward error <= tol (<= 0: 2^-52).  Not part of the
# reference interface (DESIGN.md section 8.2).
function ls_solve_refine!(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}, my_rhs::Array{Float64,1}, my_sol::Array{Float64,1};
                          max_steps::Integer=3, tol::Float64=0.0)
    info = Ref(OkktRefineInfo(0, 0, 0.0, 0.0, 0.0))
    rc = ccall((:okkt_solve_refine, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Float64,
                                                     Ref{OkktRefineInfo}, Ptr{Float64}),
               solver.handle, A.nzval, my_rhs, my_sol, 1, Int32(max_steps), tol, info, C_NULL)
    rc < 0 && okkt_error(solver, "okkt_solve_refine", rc)
    return info[]
end

struct OkktGmresInfo      # okkt_gmres_info of include/okkt.h
    iterations::Int32    # preconditioned operator applications inside GMRES cycles
    cycles::Int32        # outer steps (one double-double residual + one GMRES cycle each)
    status::Int32        # 0 omega <= tol, 1 iteration limit, 2 stagnated, 3 non-finite
    solves::Int32        # solve passes with the factor
    omega0::Float64
    omega::Float64
    resid_inf::Float64
    work_bytes::Int64
end

# sol for A sol = rhs with the held factor F ~ A as the preconditioner of GMRES(restart) cycles on the correction equation, the
# residual in double-double (GMRES-IR): converges where ls_solve_refine! stalls because F is too far from A.  Not part of the
# reference interface (DESIGN.md section 8.6).
function ls_solve_gmres(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}, my_rhs::Array{Float64,1}, my_sol::Array{Float64,1};
                        restart::Integer=30, max_iters::Integer=200, tol::Float64=0.0)
    info = Ref(OkktGmresInfo(0, 0, 0, 0, 0.0, 0.0, 0.0, 0))
    rc = ccall((:okkt_solve_gmres, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Float64,
                                                    Ref{OkktGmresInfo}, Ptr{Float64}),
               solver.handle, A.nzval, my_rhs, my_sol, 1, Int32(restart), Int32(max_iters), tol, info, C_NULL)
    rc < 0 && okkt_error(solver, "okkt_solve_gmres", rc)
    return info[]
end

struct OkktCondestInfo    # okkt_condest_info of include/okkt.h
    norm1::Float64       # ||F||_1, exact
    inv_norm1::Float64   # estimate of ||F^-1||_1 (a lower bound)
    cond1::Float64
    iterations::Int32
    solves::Int32
    status::Int32        # 0 converged, 1 iteration limit, 3 non-finite
end

# kappa_1 of the factored F (A.nzval plus the factorisation's diagonal shift), Higham-Tisseur block estimate with t columns (1..4).
# Not part of the reference interface (DESIGN.md section 8.3).
function ls_condest(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}; t::Integer=2)
    info = Ref(OkktCondestInfo(0.0, 0.0, 0.0, 0, 0, 0))
    rc = ccall((:okkt_condest, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{OkktCondestInfo}), solver.handle, A.nzval, Int32(t), info)
    rc < 0 && okkt_error(solver, "okkt_condest", rc)
    return info[]
end

# LAPACK's forward error bound (FERR) and the componentwise backward error (BERR) of a solution x of A x = rhs; a bound only when A
# is the factored matrix
function ls_forward_error(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}, my_rhs::Array{Float64,1}, x::Array{Float64,1})
    ferr = zeros(1)
    berr = zeros(1)
    rc = ccall((:okkt_forward_error, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
               solver.handle, A.nzval, my_rhs, x, 1, ferr, berr)
    rc < 0 && okkt_error(solver, "okkt_forward_error", rc)
    return ferr[1], berr[1]
end

struct OkktEigsOpts       # okkt_eigs_opts of include/okkt.h
    nev::Int32
    block::Int32
    max_basis::Int32     # 0: the default
    max_restarts::Int32
    tol::Float64         # 0: 2^-26
    nlead::Int64         # 0 or dim: the standard problem; else the leading block of the pencil (a count, not an index)
    seed::UInt64
end

struct OkktEigsInfo       # okkt_eigs_info of include/okkt.h
    status::Int32        # 0 converged, 1 restart limit, 2 the whole space was spanned, 3 non-finite
    nconv::Int32
    sweeps::Int32
    solves::Int32
    restarts::Int32
    basis::Int32
    fresh_blocks::Int32
    dropped_columns::Int32
    true_residuals::Int32
    bytes::Int64
end

# The nev eigenvalues of smallest modulus of the factored F (or of the pencil F v = lambda B v, B = diag(I_nlead, 0)) by block shift-invert
# Krylov-Schur through the factor: (lambda, V, resid, info), the vectors in the columns of V.  With A the residuals are the true
# ||lambda B v - F v||_2 against A.nzval.  Not part of the reference interface (DESIGN.md section 8.14).
function ls_eigs(solver::linear_solver_HIP, nev::Integer, A::Union{SparseMatrixCSC{Float64,Int64},Nothing}=nothing; block::Integer=4,
                 max_basis::Integer=0, max_restarts::Integer=20, tol::Float64=0.0, nlead::Integer=0, seed::Integer=1, dim::Integer=(A === nothing ? 0 : size(A, 1)))
    opts = Ref(OkktEigsOpts(Int32(nev), Int32(block), Int32(max_basis), Int32(max_restarts), tol, Int64(nlead), UInt64(seed)))
    info = Ref(OkktEigsInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    lambda = zeros(max(nev, 1))
    resid = zeros(max(nev, 1))
    V = zeros(max(dim, 1), max(nev, 1))
    rc = ccall((:okkt_eigs, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{OkktEigsOpts}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{OkktEigsInfo}),
               solver.handle, opts, A === nothing ? C_NULL : A.nzval, lambda, dim > 0 ? V : C_NULL, resid, info)
    rc < 0 && okkt_error(solver, "okkt_eigs", rc)
    return lambda[1:nev], V[1:dim, 1:nev], resid[1:nev], info[]
end

struct OkktScalingInfo    # okkt_scaling_info of include/okkt.h
    mode::Int32          # 0 none, 1 Ruiz sweeps rounded to powers of two, 2 the caller's vector
    sweeps::Int32
    rowmax_min::Float64  # over the non-zero rows of |S F S| as factored
    rowmax_max::Float64
    zero_rows::Int64
end

# Symmetric equilibration before the factorisation (DESIGN.md section 8.8): mode 0 off, 1 every ls_factor! computes s by `sweeps`
# Jacobi sweeps (0 = 10) rounded to powers of two and factors S F S, 2 the vector s (the analysed dimension, finite and > 0) as given.
# Solves, refinement and the estimates keep describing the unscaled matrix.  Not part of the reference interface.
function set_scaling!(solver::linear_solver_HIP, mode::Integer, sweeps::Integer=0, s::Union{Nothing,Array{Float64,1}}=nothing)
    rc = s === nothing ?
         ccall((:okkt_set_scaling, OKKT_LIB), Cint, (Ptr{Cvoid}, Cint, Int32, Ptr{Float64}), solver.handle, mode, Int32(sweeps), C_NULL) :
         ccall((:okkt_set_scaling, OKKT_LIB), Cint, (Ptr{Cvoid}, Cint, Int32, Ptr{Float64}), solver.handle, mode, Int32(sweeps), s)
    rc < 0 && okkt_error(solver, "okkt_set_scaling", rc)
end

# (s, info) of the current factor: s in the original order (dim = the analysed dimension)
function scaling(solver::linear_solver_HIP, dim::Integer)
    s = zeros(dim)
    info = Ref(OkktScalingInfo(0, 0, 0.0, 0.0, 0))
    rc = ccall((:okkt_get_scaling, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{OkktScalingInfo}), solver.handle, s, info)
    rc < 0 && okkt_error(solver, "okkt_get_scaling", rc)
    return s, info[]
end
scaling_info(solver::linear_solver_HIP, dim::Integer) = scaling(solver, dim)[2]

struct OkktPivotInfo      # okkt_pivot_info of include/okkt.h
    u::Float64
    rejected::Int64          # columns with g_j > 1/u: the pivots MA97 with ma97_u = u would not have taken where they stand
    nonfinite_cols::Int64
    max_multiplier::Float64
    max_col::Int64           # 0-based original index, -1 when dim = 0
    seconds_device::Float64
end

# Threshold pivot report of the current factor (DESIGN.md section 8.9): g_j = max_i |L_ij| per pivot column, counted against 1/u
# (u <= 0: 1e-8, pars.kkt.ma97_u).  Not part of the reference interface.
function pivot_report(solver::linear_solver_HIP, u::Float64=1e-8)
    info = Ref(OkktPivotInfo(0.0, 0, 0, 0.0, -1, 0.0))
    rc = ccall((:okkt_pivot_report, OKKT_LIB), Cint, (Ptr{Cvoid}, Float64, Ref{OkktPivotInfo}), solver.handle, u, info)
    rc < 0 && okkt_error(solver, "okkt_pivot_report", rc)
    return info[]
end

# (g, partner) of the last report in the original order; partner is 0-based, -1 for a column without a row below the diagonal
function multipliers(solver::linear_solver_HIP, dim::Integer)
    g = zeros(dim)
    partner = zeros(Int64, dim)
    rc = ccall((:okkt_get_multipliers, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), solver.handle, g, partner)
    rc < 0 && okkt_error(solver, "okkt_get_multipliers", rc)
    return g, partner
end

# the rejected columns of the last report (0-based original indices) by descending g, and their partners
function rejected_pivots(solver::linear_solver_HIP)
    cnt = ccall((:okkt_get_rejected_pivots, OKKT_LIB), Int64, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64), solver.handle, C_NULL, C_NULL, 0)
    cnt < 0 && okkt_error(solver, "okkt_get_rejected_pivots", cnt)
    idx = zeros(Int64, cnt)
    partner = zeros(Int64, cnt)
    ccall((:okkt_get_rejected_pivots, OKKT_LIB), Int64, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Int64), solver.handle, idx, partner, cnt)
    return idx, partner
end

# The factor as an operator (DESIGN.md section 8.12).  Factor coordinates: the library holds S P F P' S = L D L'; entry j of a vector
# in factor order is original index perm[j] (okkt_get_perm).  Not part of the reference interface.
# z = D^-1 L^-1 P S b (factor order): ls_solve! stopped behind its forward sweep; my_rhs is a vector or a dim x nrhs matrix
function ls_solve_forward(solver::linear_solver_HIP, my_rhs::Array{Float64})
    z = similar(my_rhs)
    rc = ccall((:okkt_solve_forward, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), solver.handle, my_rhs, z, size(my_rhs, 2))
    rc < 0 && okkt_error(solver, "okkt_solve_forward", rc)
    return z
end

# x = S P' L^-T z (original order); ls_solve_backward(ls_solve_forward(b)) is ls_solve!'s x bit for bit
function ls_solve_backward(solver::linear_solver_HIP, z::Array{Float64})
    x = similar(z)
    rc = ccall((:okkt_solve_backward, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), solver.handle, z, x, size(z, 2))
    rc < 0 && okkt_error(solver, "okkt_solve_backward", rc)
    return x
end

# (q_pos, q_neg) per right-hand side from one forward sweep: the sums of d_j z_j^2 over the positive and the negative pivots;
# b' F^-1 b = q_pos + q_neg
function quadform(solver::linear_solver_HIP, my_rhs::Array{Float64})
    nrhs = size(my_rhs, 2)
    q_pos = zeros(nrhs)
    q_neg = zeros(nrhs)
    rc = ccall((:okkt_quadform, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}), solver.handle, my_rhs, nrhs, q_pos, q_neg)
    rc < 0 && okkt_error(solver, "okkt_quadform", rc)
    return q_pos, q_neg
end

const OKKT_OP_L = 1          # y = L x, factor coordinates, unit diagonal included, no scaling
const OKKT_OP_LT = 2         # y = L' x, the same
const OKKT_OP_LDLT = 3       # y = S^-1 P' L D L' P S^-1 x, original coordinates: F x up to the factorisation's error
const OKKT_OP_ABS_LDLT = 4   # y = S^-1 P' |L| |D| |L'| P S^-1 |x|

function factor_multiply(solver::linear_solver_HIP, op::Integer, x::Array{Float64})
    y = similar(x)
    rc = ccall((:okkt_factor_multiply, OKKT_LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Int64), solver.handle, op, x, y, size(x, 2))
    rc < 0 && okkt_error(solver, "okkt_factor_multiply", rc)
    return y
end

struct OkktFactorErrorInfo    # okkt_factor_error_info of include/okkt.h
    rho::Float64             # norm_abs_ldlt / norm_f: the growth factor of the static-pivot factorisation
    norm_abs_ldlt::Float64   # || |L||D||L'| e ||_inf (original coordinates)
    norm_f::Float64          # ||F||_inf
    eta::Float64             # max over the probes and rows of |(F v - L D L' v)_i| / ((|F| + |L||D||L'|) e)_i
    eta_row::Int64           # 0-based original index of the row that attains it, -1 when dim = 0
    probes::Int32
end

# the growth factor and the sampled backward error of the current factor against A.nzval (probes 1..8, <= 0: 2)
function factor_error(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}; probes::Integer=2)
    info = Ref(OkktFactorErrorInfo(0.0, 0.0, 0.0, 0.0, -1, 0))
    rc = ccall((:okkt_factor_error, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{OkktFactorErrorInfo}), solver.handle, A.nzval, Int32(probes), info)
    rc < 0 && okkt_error(solver, "okkt_factor_error", rc)
    return info[]
end

# Sparse right-hand sides (DESIGN.md section 8.13): solves that visit only the supernodes between the non-zeros of b, the wanted rows
# and the roots of the elimination forest.  Indices are 1-based here and converted.  Not part of the reference interface.
struct OkktSparseInfo     # okkt_sparse_info of include/okkt.h
    nsuper::Int64
    fwd_reach::Int64             # supernodes in the closures (union over the call's columns)
    bwd_reach::Int64
    fwd_run::Int64               # supernodes the launches visit (>= reach: small fronts run as whole tasks)
    bwd_run::Int64
    fringe::Int64                # fronts whose contribution vectors are zeroed, and their entries
    fringe_entries::Int64
    fwd_panel_bytes::Int64
    bwd_panel_bytes::Int64
    factor_panel_bytes::Int64
    batches::Int32
    pruned::Int32                # 0: the ordinary sweeps ran
    seconds_device::Float64
end
okkt_sparse_info_zero() = Ref(OkktSparseInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0))

# X (length(rows) x nrhs; rows = nothing: dim x nrhs) with X[t, q] = x_q[rows[t]] for the columns of B, and the info: equal to
# ls_solve! of the densified columns at those entries
function ls_solve_sparse(solver::linear_solver_HIP, B::SparseMatrixCSC{Float64,Int64}; rows::Union{Nothing,Vector{Int64}}=nothing)
    nrhs = size(B, 2)
    colptr = B.colptr .- 1
    rowidx = B.rowval .- 1
    nx = rows === nothing ? size(B, 1) : length(rows)
    xidx = rows === nothing ? Int64[] : rows .- 1
    X = zeros(nx, nrhs)
    info = okkt_sparse_info_zero()
    rc = ccall((:okkt_solve_sparse, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64},
                                                     Ref{OkktSparseInfo}),
               solver.handle, nrhs, colptr, rowidx, B.nzval, nx, rows === nothing ? C_NULL : xidx, X, info)
    rc < 0 && okkt_error(solver, "okkt_solve_sparse", rc)
    return X, info[]
end

# (F^-1)[rows, cols] (rows = nothing: all), entries off the pattern of L included
function inverse_columns(solver::linear_solver_HIP, cols::Vector{Int64}; rows::Union{Nothing,Vector{Int64}}=nothing, dim::Integer=0)
    nr = rows === nothing ? Int64(dim) : length(rows)
    rows === nothing && dim <= 0 && error("inverse_columns: give dim when rows = nothing")
    c0 = cols .- 1
    r0 = rows === nothing ? Int64[] : rows .- 1
    Z = zeros(nr, length(cols))
    info = okkt_sparse_info_zero()
    rc = ccall((:okkt_get_inverse_columns, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Ref{OkktSparseInfo}),
               solver.handle, length(cols), c0, nr, rows === nothing ? C_NULL : r0, Z, info)
    rc < 0 && okkt_error(solver, "okkt_get_inverse_columns", rc)
    return Z
end

inverse_block(solver::linear_solver_HIP, idx::Vector{Int64}) = inverse_columns(solver, idx; rows=idx)

# host only (also on host_symbolic_only handles after the analysis): the sets ls_solve_sparse would use.  Returns the info and dim bytes
# in factor order: bit 0 = the column's supernode runs in the forward sweep, bit 1 = in the backward sweep, bit 2 = it is fringe
function sparse_reach(solver::linear_solver_HIP, b_rows::Vector{Int64}, dim::Integer; x_rows::Union{Nothing,Vector{Int64}}=nothing)
    b0 = b_rows .- 1
    x0 = x_rows === nothing ? Int64[] : x_rows .- 1
    active = zeros(UInt8, dim)
    info = okkt_sparse_info_zero()
    rc = ccall((:okkt_sparse_reach, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ref{OkktSparseInfo}, Ptr{UInt8}),
               solver.handle, length(b0), b0, length(x0), x_rows === nothing ? C_NULL : x0, info, active)
    rc < 0 && okkt_error(solver, "okkt_sparse_reach", rc)
    return info[], active
end

# Uniform batches (DESIGN.md section 8.15): B systems on the analysed pattern, plans of small fronts only.  Not part of the reference
# interface.  okkt_batch_info of include/okkt.h
struct OkktBatchInfo
    eligible::Int32; reason::Int32
    bytes_per_item::Int64; tasks_per_item::Int64
    levels::Int32; max_front::Int32
    launches_factor_level::Int32; launches_solve_level::Int32
    launches_factor_item::Int32; launches_solve_item::Int32
end

function batch_query(solver::linear_solver_HIP; nrhs_max::Integer=1)
    info = Ref(OkktBatchInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:okkt_batch_query, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ref{OkktBatchInfo}), solver.handle, nrhs_max, info)
    rc < 0 && okkt_error(solver, "okkt_batch_query", rc)
    return info[]
end

# mode: 0 by the measured rule, 1 level mode, 2 item mode
function batch_reserve(solver::linear_solver_HIP, B::Integer; nrhs_max::Integer=1, mode::Union{Nothing,Integer}=nothing)
    if mode !== nothing
        rc = ccall((:okkt_batch_set_mode, OKKT_LIB), Cint, (Ptr{Cvoid}, Cint), solver.handle, mode)
        rc < 0 && okkt_error(solver, "okkt_batch_set_mode", rc)
    end
    rc = ccall((:okkt_batch_reserve, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Int64), solver.handle, B, nrhs_max)
    rc < 0 && okkt_error(solver, "okkt_batch_reserve", rc)
end

function batch_release(solver::linear_solver_HIP)
    rc = ccall((:okkt_batch_release, OKKT_LIB), Cint, (Ptr{Cvoid},), solver.handle)
    rc < 0 && okkt_error(solver, "okkt_batch_release", rc)
end

# vals: nnz x B (one column per item), or a vector shared by all items together with shifts (length B); shifts[b] is added to the first
# nshift (default n) diagonal entries.  Returns the items' flags and inertia counts (4 x B: pos, neg, zero, nonfinite)
function ls_factor_batch(solver::linear_solver_HIP, vals::Union{Matrix{Float64},Vector{Float64}}, n::Int64, m::Int64;
                         shifts::Union{Nothing,Vector{Float64}}=nothing, nshift::Int64=n)
    B = vals isa Matrix ? size(vals, 2) : length(shifts)
    stride = vals isa Matrix ? size(vals, 1) : 0
    inertia = zeros(Int64, 4, B); flags = zeros(Int32, B)
    kind = solver.sym == :definite ? 0 : 1
    rc = ccall((:okkt_factor_batch, OKKT_LIB), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Ptr{Int64}, Ptr{Int32}),
               solver.handle, B, vals, stride, shifts === nothing ? C_NULL : shifts, nshift, n, m, kind, inertia, flags)
    rc < 0 && okkt_error(solver, "okkt_factor_batch", rc)
    return flags, inertia
end

# rhs: dim x nrhs x B (or dim x B): the items' solutions in the same shape
function ls_solve_batch(solver::linear_solver_HIP, rhs::Array{Float64})
    B = size(rhs, ndims(rhs)); nrhs = ndims(rhs) == 3 ? size(rhs, 2) : 1
    sol = similar(rhs)
    rc = ccall((:okkt_solve_batch, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Int64), solver.handle, B, rhs, sol, nrhs)
    rc < 0 && okkt_error(solver, "okkt_solve_batch", rc)
    return sol
end

# slot b (1-based) becomes the handle's own factor
function batch_select(solver::linear_solver_HIP, b::Integer)
    rc = ccall((:okkt_batch_select, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64), solver.handle, b - 1)
    rc < 0 && okkt_error(solver, "okkt_batch_select", rc)
end

# Scenario batches (DESIGN.md section 8.16): B items in Schur mode on the analysed pattern [[A11 A12]; [A21 A22]], their S_b summed on the
# device in the order okkt.h states, one dense factor of the sum: the arrowhead system of B blocks.  The handle is in Schur mode
# (okkt_set_schur before the analysis).  Not part of the reference interface.  okkt_schur_batch_info of include/okkt.h
struct OkktSchurBatchInfo
    eligible::Int32; reason::Int32
    ns::Int64
    bytes_per_item::Int64; bytes_shared::Int64
    tasks_per_item::Int64
    levels::Int32; max_front::Int32
    launches_factor::Int32; launches_solve::Int32
end

function schur_batch_query(solver::linear_solver_HIP; nrhs_max::Integer=1)
    info = Ref(OkktSchurBatchInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:okkt_schur_batch_query, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ref{OkktSchurBatchInfo}), solver.handle, nrhs_max, info)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_query", rc)
    return info[]
end

function schur_batch_reserve(solver::linear_solver_HIP, B::Integer; nrhs_max::Integer=1)
    rc = ccall((:okkt_schur_batch_reserve, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Int64), solver.handle, B, nrhs_max)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_reserve", rc)
end

function schur_batch_release(solver::linear_solver_HIP)
    rc = ccall((:okkt_schur_batch_release, OKKT_LIB), Cint, (Ptr{Cvoid},), solver.handle)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_release", rc)
end

# vals: nnz x B (one column per item); n1 + m1 = dim - ns; shifts[b] is added to the first nshift (default n1) diagonal entries.
# Returns the items' flags and the inertia counts of their A11 (4 x B: pos, neg, zero, nonfinite)
function ls_factor_schur_batch(solver::linear_solver_HIP, vals::Matrix{Float64}, n1::Int64, m1::Int64;
                               shifts::Union{Nothing,Vector{Float64}}=nothing, nshift::Int64=n1)
    B = size(vals, 2)
    inertia = zeros(Int64, 4, B); flags = zeros(Int32, B)
    kind = solver.sym == :definite ? 0 : 1
    rc = ccall((:okkt_factor_schur_batch, OKKT_LIB), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Ptr{Int64}, Ptr{Int32}),
               solver.handle, B, vals, size(vals, 1), shifts === nothing ? C_NULL : shifts, nshift, n1, m1, kind, inertia, flags)
    rc < 0 && okkt_error(solver, "okkt_factor_schur_batch", rc)
    return flags, inertia
end

# S_b of item b (1-based), or the sum of the items' S_b for b = 0: ns x ns, symmetric, in the order of the set
function schur_batch(solver::linear_solver_HIP, b::Integer=0)
    ns = schur_batch_query(solver).ns
    S = zeros(Float64, ns, ns)
    rc = ccall((:okkt_schur_batch_get, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), solver.handle, b - 1, S, ns)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_get", rc)
    return S
end

# dense factor of sum_b S_b (+ S_add, added last): (flag, inertia of the sum, inertia of the arrowhead matrix), counts as (pos, neg, zero, nonfinite)
function schur_batch_factor(solver::linear_solver_HIP; S_add::Union{Nothing,Matrix{Float64}}=nothing)
    si = zeros(Int64, 4); ti = zeros(Int64, 4)
    rc = ccall((:okkt_schur_batch_factor, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}),
               solver.handle, S_add === nothing ? C_NULL : S_add, S_add === nothing ? 0 : size(S_add, 1), si, ti)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_factor", rc)
    return rc, si, ti
end

# rhs: dim x nrhs x B -> (the summed r2: ns x nrhs, the items' r2_b: ns x nrhs x B)
function schur_batch_condense(solver::linear_solver_HIP, rhs::Array{Float64,3})
    ns = schur_batch_query(solver).ns
    nrhs = size(rhs, 2); B = size(rhs, 3)
    r2 = zeros(Float64, ns, nrhs); items = zeros(Float64, ns, nrhs, B)
    rc = ccall((:okkt_schur_batch_condense, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
               solver.handle, B, rhs, r2, items, nrhs)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_condense", rc)
    return r2, items
end

# the one x2 (ns x nrhs) put into every item: the items' solutions, dim x nrhs x B
function schur_batch_expand(solver::linear_solver_HIP, rhs::Array{Float64,3}, x2::Matrix{Float64})
    sol = similar(rhs)
    rc = ccall((:okkt_schur_batch_expand, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
               solver.handle, size(rhs, 3), rhs, x2, sol, size(rhs, 2))
    rc < 0 && okkt_error(solver, "okkt_schur_batch_expand", rc)
    return sol
end

# the arrowhead system: rhs dim x nrhs x B (the entries at the set are the items' shares of the linking right-hand side), rhs0 (ns x nrhs)
# added to their sum last; the solutions in the shape of rhs, x_L at the set in every item
function schur_batch_solve(solver::linear_solver_HIP, rhs::Array{Float64,3}; rhs0::Union{Nothing,Matrix{Float64}}=nothing)
    sol = similar(rhs)
    rc = ccall((:okkt_schur_batch_solve, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
               solver.handle, size(rhs, 3), rhs, rhs0 === nothing ? C_NULL : rhs0, sol, size(rhs, 2))
    rc < 0 && okkt_error(solver, "okkt_schur_batch_solve", rc)
    return sol
end

# slot b (1-based) becomes the handle's own state, as after okkt_factor_schur of that item
function schur_batch_select(solver::linear_solver_HIP, b::Integer)
    rc = ccall((:okkt_schur_batch_select, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64), solver.handle, b - 1)
    rc < 0 && okkt_error(solver, "okkt_schur_batch_select", rc)
end

# ls_solve_refine! through the Schur route: every solve is okkt_schur_solve's, the residuals are against the whole A.  Needs
# okkt_factor_schur and okkt_schur_factor of the handle's own S.
function schur_solve_refine!(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}, my_rhs::Array{Float64,1}, my_sol::Array{Float64,1};
                             max_steps::Integer=3, tol::Float64=0.0)
    info = Ref(OkktRefineInfo(0, 0, 0.0, 0.0, 0.0))
    rc = ccall((:okkt_schur_solve_refine, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Float64,
                                                           Ref{OkktRefineInfo}, Ptr{Float64}),
               solver.handle, A.nzval, my_rhs, my_sol, 1, Int32(max_steps), tol, info, C_NULL)
    rc < 0 && okkt_error(solver, "okkt_schur_solve_refine", rc)
    return info[]
end

# The Schur route made whole (DESIGN.md section 8.10): what judges a doubtful factor, for a handle in Schur mode.  Except schur_inverse
# every call needs okkt_factor_schur and okkt_schur_factor of the handle's own S.  Not part of the reference interface.
struct OkktSelinvInfo     # okkt_selinv_info of include/okkt.h
    seconds_device::Float64
    arena_bytes::Int64
    nonfinite::Int64
    status::Int32            # 1 when Z has non-finite entries
    flops::Float64
end

# (S^-1, the number of its non-finite entries): ns x ns in the order of the set, both triangles the same bits; of the current dense
# factor, the handle's own S or a caller's
function schur_inverse(solver::linear_solver_HIP, ns::Integer)
    Z = zeros(ns, ns)
    rc = ccall((:okkt_schur_get_inverse, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), solver.handle, Z, ns)
    rc < 0 && okkt_error(solver, "okkt_schur_get_inverse", rc)
    return Z, ccall((:okkt_schur_inverse_nonfinite, OKKT_LIB), Int64, (Ptr{Cvoid},), solver.handle)
end

# Z = A^-1 on the pattern of the whole factor, kept on the device for okkt_get_inverse_diag / _on_pattern / _csc
function schur_selinv(solver::linear_solver_HIP)
    info = Ref(OkktSelinvInfo(0.0, 0, 0, 0, 0.0))
    rc = ccall((:okkt_schur_selinv, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{OkktSelinvInfo}), solver.handle, info)
    rc < 0 && okkt_error(solver, "okkt_schur_selinv", rc)
    return info[]
end

# (log |det A|, sign)
function schur_logdet(solver::linear_solver_HIP)
    v = Ref(0.0)
    s = Ref(Int32(0))
    rc = ccall((:okkt_schur_logdet, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Int32}), solver.handle, v, s)
    rc < 0 && okkt_error(solver, "okkt_schur_logdet", rc)
    return v[], s[]
end

function schur_condest(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}; t::Integer=2)
    info = Ref(OkktCondestInfo(0.0, 0.0, 0.0, 0, 0, 0))
    rc = ccall((:okkt_schur_condest, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{OkktCondestInfo}), solver.handle, A.nzval, Int32(t), info)
    rc < 0 && okkt_error(solver, "okkt_schur_condest", rc)
    return info[]
end

function schur_forward_error(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}, my_rhs::Array{Float64,1}, x::Array{Float64,1})
    ferr = zeros(1)
    berr = zeros(1)
    rc = ccall((:okkt_schur_forward_error, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
               solver.handle, A.nzval, my_rhs, x, 1, ferr, berr)
    rc < 0 && okkt_error(solver, "okkt_schur_forward_error", rc)
    return ferr[1], berr[1]
end

function schur_solve_gmres(solver::linear_solver_HIP, A::SparseMatrixCSC{Float64,Int64}, my_rhs::Array{Float64,1}, my_sol::Array{Float64,1};
                           restart::Integer=30, max_iters::Integer=200, tol::Float64=0.0)
    info = Ref(OkktGmresInfo(0, 0, 0, 0, 0.0, 0.0, 0.0, 0))
    rc = ccall((:okkt_schur_solve_gmres, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Float64,
                                                          Ref{OkktGmresInfo}, Ptr{Float64}),
               solver.handle, A.nzval, my_rhs, my_sol, 1, Int32(restart), Int32(max_iters), tol, info, C_NULL)
    rc < 0 && okkt_error(solver, "okkt_schur_solve_gmres", rc)
    return info[]
end

function ls_solve(solver::linear_solver_HIP, my_rhs::AbstractArray, timer::class_advanced_timer)
    rhs = Vector{Float64}(my_rhs)      # SparseVector rhs is densified, as in julia.jl:105-113
    sol = zeros(length(rhs))
    ls_solve!(solver, rhs, sol, timer)
    return sol
end
