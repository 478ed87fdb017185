# kkt_solver_hip.jl -- Julia glue for the device-resident KKT-system level of libonephase_kkt.so.
# UNTESTED IN THIS REPOSITORY (no Julia in the build environment); mirrors symmetric.jl / schur.jl of the
# reference and implements the four methods every abstract_KKT_system_solver must define
# (src/kkt_system_solver/kkt_system_solver.jl:13-17).  See INTEGRATION.md.

mutable struct HIP_KKT_solver <: abstract_KKT_system_solver
    ls_solver::abstract_linear_system_solver    # unused (the library owns the factorisation); kept for field parity
    factor_it::Class_iterate
    delta_x_vec::Array{Float64,1}
    delta_s_vec::Array{Float64,1}
    rhs::System_rhs
    dir::Class_point
    kkt_err_norm::Class_kkt_error
    rhs_norm::Float64
    pars::Class_parameters
    schur_diag::Array{Float64,1}
    ready::Symbol
    Q::SparseMatrixCSC{Float64,Int64}           # left empty: the assembled matrix lives in HBM
    handle::Ptr{Cvoid}
    kind::Cint                                   # 0 = :schur, 1 = :symmetric, 2 = :clever_symmetric, 3 = :schur_direct
    pattern_set::Bool
    current_it::Class_iterate                    # iterate of the last kkt_associate_rhs! (schur.jl:34-45)
    reduct_factors::Class_reduction_factors
    resident_rhs::Any                            # the System_rhs object whose triple okkt_kkt_system_rhs left in HBM (nothing: none)

    function HIP_KKT_solver(kind::Symbol, opts::Union{Nothing,OkktOpts}=nothing)      # opts: okkt_opts_from_pars(pars.kkt), linear_solver_hip.jl
        this = new()
        this.ready = :not_ready
        this.kind = Dict(:schur => 0, :symmetric => 1, :clever_symmetric => 2, :schur_direct => 3)[kind]
        this.pattern_set = false
        this.resident_rhs = nothing
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = opts === nothing ?
             ccall((:okkt_kkt_create, OKKT_LIB), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Cint), h, C_NULL, this.kind) :
             ccall((:okkt_kkt_create, OKKT_LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{OkktOpts}, Cint), h, Ref(opts), this.kind)
        rc == 0 || error("okkt_kkt_create failed with code $rc")
        this.handle = h[]
        finalizer(s -> ccall((:okkt_kkt_destroy, OKKT_LIB), Cint, (Ptr{Cvoid},), s.handle), this)
        return this
    end
end

struct OkktKktEigInfo   # okkt_kkt_eig_info of include/okkt.h
    theta_min::Float64
    theta_max::Float64
    bound::Float64
    rho::Float64
    rho_abs::Float64
    rho_margin::Float64
    resid::Float64
    steps::Int32
    status::Int32
    seconds_device::Float64
end

struct OkktKktPars      # okkt_kkt_pars of include/okkt.h
    delta_start::Float64
    delta_min::Float64
    delta_max::Float64
    delta_inc::Float64
    delta_dec::Float64
    delta_zero::Float64
    ItRefine_Num::Int32
    max_it::Int32
end

function kkt_hip_check(k::HIP_KKT_solver, what::String, rc)
    rc < 0 && error("$what failed ($rc): " * unsafe_string(ccall((:okkt_kkt_last_error, OKKT_LIB), Cstring, (Ptr{Cvoid},), k.handle)))
    return rc
end

# okkt_kkt_set_ls_refine (symmetric kind only): pars.kkt.hip_ls_refine_steps / hip_ls_refine_tol ("kkt!hip_ls_refine_steps",
# "kkt!hip_ls_refine_tol"; not okkt_opts fields).  Call once after construction; 0 steps (the default) leaves the plain solve.
function set_ls_refine!(k::HIP_KKT_solver, max_steps::Integer, tol::Float64=0.0)
    kkt_hip_check(k, "okkt_kkt_set_ls_refine", ccall((:okkt_kkt_set_ls_refine, OKKT_LIB), Cint, (Ptr{Cvoid}, Int32, Float64),
                                                     k.handle, Int32(max_steps), tol))
end
function set_ls_refine!(k::HIP_KKT_solver, pars::Class_parameters)
    steps = hasproperty(pars.kkt, :hip_ls_refine_steps) ? pars.kkt.hip_ls_refine_steps : 0
    tol = hasproperty(pars.kkt, :hip_ls_refine_tol) ? pars.kkt.hip_ls_refine_tol : 0.0
    (steps != 0 || tol != 0.0) && set_ls_refine!(k, steps, tol)
end

# okkt_kkt_set_ls_scaling (Schur, Schur-direct and symmetric kinds): pars.kkt.hip_ls_scaling (0 / 1) and hip_ls_scaling_sweeps (0 = 10)
# ("kkt!hip_ls_scaling", "kkt!hip_ls_scaling_sweeps"; not okkt_opts fields).  Call once after construction: every factor! then
# equilibrates the shifted system it factors (DESIGN.md section 8.8); directions and estimates keep describing the unscaled system.
function set_ls_scaling!(k::HIP_KKT_solver, on::Integer, sweeps::Integer=0)
    kkt_hip_check(k, "okkt_kkt_set_ls_scaling", ccall((:okkt_kkt_set_ls_scaling, OKKT_LIB), Cint, (Ptr{Cvoid}, Cint, Int32),
                                                      k.handle, on != 0 ? 1 : 0, Int32(sweeps)))
end
function set_ls_scaling!(k::HIP_KKT_solver, pars::Class_parameters)
    on = hasproperty(pars.kkt, :hip_ls_scaling) ? pars.kkt.hip_ls_scaling : 0
    sweeps = hasproperty(pars.kkt, :hip_ls_scaling_sweeps) ? pars.kkt.hip_ls_scaling_sweeps : 0
    on != 0 && set_ls_scaling!(k, on, sweeps)
end

# okkt_kkt_condest: kappa_1 of the system the last factor! factored (K + delta, M, Q + delta I or the bordered A with dense rows)
function kkt_condest(k::HIP_KKT_solver; t::Integer=2)
    info = Ref(OkktCondestInfo(0.0, 0.0, 0.0, 0, 0, 0))
    kkt_hip_check(k, "okkt_kkt_condest", ccall((:okkt_kkt_condest, OKKT_LIB), Cint, (Ptr{Cvoid}, Int32, Ref{OkktCondestInfo}),
                                               k.handle, Int32(t), info))
    return info[]
end
# okkt_kkt_eigs: (lambda, X, resid, info) -- the nev eigenvalues of smallest modulus of H + J' Sigma J + delta I at the delta of the last
# factor!, the x-parts of their vectors in the columns of X (n x nev) and the true residuals (DESIGN.md section 8.14)
function kkt_eigs(k::HIP_KKT_solver, nev::Integer, n::Integer; block::Integer=4, max_basis::Integer=0, max_restarts::Integer=20,
                  tol::Float64=0.0, seed::Integer=1)
    opts = Ref(OkktEigsOpts(Int32(nev), Int32(block), Int32(max_basis), Int32(max_restarts), tol, Int64(0), UInt64(seed)))
    info = Ref(OkktEigsInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    lambda = zeros(max(nev, 1))
    resid = zeros(max(nev, 1))
    X = zeros(max(n, 1), max(nev, 1))
    kkt_hip_check(k, "okkt_kkt_eigs", ccall((:okkt_kkt_eigs, OKKT_LIB), Cint,
                                            (Ptr{Cvoid}, Ref{OkktEigsOpts}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{OkktEigsInfo}),
                                            k.handle, opts, lambda, X, resid, info))
    return lambda[1:nev], X[1:n, 1:nev], resid[1:nev], info[]
end
# okkt_kkt_direction_error_bound (symmetric kind): the forward error bound of the last direction's solve against K + delta
function direction_error_bound(k::HIP_KKT_solver)
    ferr = Ref(0.0)
    kkt_hip_check(k, "okkt_kkt_direction_error_bound", ccall((:okkt_kkt_direction_error_bound, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{Float64}),
                                                             k.handle, ferr))
    return ferr[]
end

# the rows of J (1-based, ascending) that okkt_opts.schur_dense_rows ("kkt!hip_schur_dense_rows", carried by okkt_opts_from_pars) moved out
# of Q into the border of the factorised Schur system; empty with the option off and for the other kinds
function dense_rows(k::HIP_KKT_solver)
    cnt = Ref{Int64}(0)
    kkt_hip_check(k, "okkt_kkt_get_dense_rows", ccall((:okkt_kkt_get_dense_rows, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}),
                                                      k.handle, cnt, C_NULL))
    rows = zeros(Int64, cnt[])
    kkt_hip_check(k, "okkt_kkt_get_dense_rows", ccall((:okkt_kkt_get_dense_rows, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}),
                                                      k.handle, cnt, rows))
    return rows .+ 1
end

# initialize!(::Clever_Symmetric_KKT_solver, it) (clever_symmetric.jl:53-61): the parallel-row grouping is computed
# once, from the Jacobian of the initial iterate
function initialize!(k::HIP_KKT_solver, intial_it::Class_iterate)
    k.dir = zero_point(dim(intial_it), ncon(intial_it))
    if k.kind == 2
        H = get_lag_hess(intial_it); J = get_jac(intial_it)
        kkt_hip_check(k, "okkt_kkt_set_structure", ccall((:okkt_kkt_set_structure, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint),
            k.handle, dim(intial_it), ncon(intial_it), H.colptr, H.rowval, J.colptr, J.rowval, 1))
        k.pattern_set = true
        m_new = Ref{Int64}(0)
        kkt_hip_check(k, "okkt_kkt_compute_indicies", ccall((:okkt_kkt_compute_indicies, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}), k.handle, J.nzval, m_new))
    end
end

function form_system!(k::HIP_KKT_solver, iter::Class_iterate, timer::class_advanced_timer)
    start_advanced_timer(timer, "HIP/form_system")
    H = get_lag_hess(iter); J = get_jac(iter)
    n = dim(iter); m = ncon(iter)
    if k.kind == 2     # kkt_system_rescale, clever_symmetric.jl:377-385
        mode = Dict(:none => 0, :u_only => 1, :u_and_x => 2)[k.pars.kkt.kkt_system_rescale]
        kkt_hip_check(k, "okkt_kkt_set_rescale", ccall((:okkt_kkt_set_rescale, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Cint, Float64, Float64), k.handle, mode, iter.point.mu, LinearAlgebra.norm(iter.point.x, Inf)))
    end
    if !k.pattern_set
        kkt_hip_check(k, "okkt_kkt_set_structure", ccall((:okkt_kkt_set_structure, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint),
            k.handle, n, m, H.colptr, H.rowval, J.colptr, J.rowval, 1))
        k.pattern_set = true
    end
    kkt_hip_check(k, "okkt_kkt_form_system", ccall((:okkt_kkt_form_system, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        k.handle, H.nzval, J.nzval, get_s(iter), get_y(iter)))
    k.schur_diag = zeros(n)
    ccall((:okkt_kkt_get_schur_diag, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), k.handle, k.schur_diag)
    k.factor_it = iter
    k.ready = :system_formed
    pause_advanced_timer(timer, "HIP/form_system")
end

function update_delta_vecs!(k::HIP_KKT_solver, delta_x_vec::Array{Float64,1}, delta_s_vec::Array{Float64,1}, timer::class_advanced_timer)
    k.delta_x_vec = delta_x_vec
    k.delta_s_vec = delta_s_vec
    sum(abs.(delta_s_vec)) > 0.0 && error("Not implemented")
    k.ready = :delta_updated
end

# factor!(kkt_solver, timer) -> factor_implementation!: a COMPLETE factorisation whatever the inertia flag, because the
# failed-step branch of one_phase.jl:231-242 computes a direction from it even when the flag is 0.  The delta loop, which
# throws failed attempts away, goes through ipopt_strategy! below (trial factorisations that may stop early).
function factor_implementation!(k::HIP_KKT_solver, timer::class_advanced_timer)
    inert = Ref(OkktInertia(0, 0, 0, 0))
    delta = length(k.delta_x_vec) > 0 ? k.delta_x_vec[1] : 0.0
    return Int(kkt_hip_check(k, "okkt_kkt_factor", ccall((:okkt_kkt_factor, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Float64, Ref{OkktInertia}), k.handle, delta, inert)))
end

# okkt_kkt_min_eig: (info, v) -- the Lanczos estimate of lambda_min(Q(0)), Q(0) = H + J' Sigma J of the last form_system!, and the vector
# whose Rayleigh quotient on Q(0) is info.rho; every factor! with delta <= -info.rho - info.rho_margin has the wrong inertia
function min_eig(k::HIP_KKT_solver, max_steps::Integer=0, tol::Float64=0.0, scaled::Integer=0)
    info = Ref(OkktKktEigInfo(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0))
    v = zeros(dim(k.factor_it))
    kkt_hip_check(k, "okkt_kkt_min_eig", ccall((:okkt_kkt_min_eig, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int32, Float64, Int32, Ref{OkktKktEigInfo}, Ptr{Float64}), k.handle, max_steps, tol, scaled, info, v))
    return info[], v
end

# ipopt_strategy! (delta_strategy.jl:37-114) for this solver type: the whole loop behind one ccall; (status, num_fac, delta)
# are those of the reference's loop
function ipopt_strategy!(iter::Class_iterate, k::HIP_KKT_solver, pars::Class_parameters, timer::class_advanced_timer)
    num_fac = Ref{Int32}(0); delta = Ref{Float64}(0.0)
    p = OkktKktPars(pars.delta.start, pars.delta.min, pars.delta.max, pars.delta.inc, pars.delta.dec, pars.delta.zero, Int32(pars.kkt.ItRefine_Num), Int32(500))
    # pars.kkt.hip_delta_eig_steps > 0 ("kkt!hip_delta_eig_steps", "kkt!hip_delta_eig_scaled"): the same loop without the attempts that a
    # Lanczos bound on lambda_min(H + J' Sigma J) certifies to fail (okkt_kkt_ipopt_strategy_eig); status and delta do not change
    eig_steps = hasproperty(pars.kkt, :hip_delta_eig_steps) ? pars.kkt.hip_delta_eig_steps : 0
    eig_scaled = hasproperty(pars.kkt, :hip_delta_eig_scaled) ? pars.kkt.hip_delta_eig_scaled : 0
    # pars.kkt.hip_delta_batch > 1 ("kkt!hip_delta_batch"): the attempts that many at a time as one uniform batch on the formed values
    # (okkt_kkt_ipopt_strategy_batch, DESIGN.md section 8.15); a refusal (big fronts, the clever-symmetric kind, scaling) takes the serial loop
    width = hasproperty(pars.kkt, :hip_delta_batch) ? pars.kkt.hip_delta_batch : 0
    rc = Cint(-1)
    if width > 1
        launches = Ref{Int32}(0)
        rc = ccall((:okkt_kkt_ipopt_strategy_batch, OKKT_LIB), Cint, (Ptr{Cvoid}, Float64, Ref{OkktKktPars}, Int32, Ref{Int32}, Ref{Float64}, Ref{Int32}),
                   k.handle, get_delta(iter), p, min(width, 64), num_fac, delta, launches)
        rc < -1 && kkt_hip_check(k, "okkt_kkt_ipopt_strategy_batch", rc)      # -1 = refused: the serial loop below
    end
    if rc >= 0
    elseif eig_steps > 0
        skipped = Ref{Int32}(0); info = Ref(OkktKktEigInfo(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0))
        rc = kkt_hip_check(k, "okkt_kkt_ipopt_strategy_eig", ccall((:okkt_kkt_ipopt_strategy_eig, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Float64, Ref{OkktKktPars}, Int32, Int32, Ref{Int32}, Ref{Float64}, Ref{Int32}, Ref{OkktKktEigInfo}),
            k.handle, get_delta(iter), p, eig_steps, eig_scaled, num_fac, delta, skipped, info))
    else
        rc = kkt_hip_check(k, "okkt_kkt_ipopt_strategy", ccall((:okkt_kkt_ipopt_strategy, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Float64, Ref{OkktKktPars}, Ref{Int32}, Ref{Float64}), k.handle, get_delta(iter), p, num_fac, delta))
    end
    k.delta_x_vec = delta[] * ones(dim(iter)); k.delta_s_vec = zeros(ncon(iter))
    k.ready = :factored
    # delta_strategy.jl:94-98: a failed attempt on a diagonally dominant x-block prints a warning; the library ran the scan on the
    # device after every failed attempt and counted
    nwarn = Ref{Int32}(0)
    if ccall((:okkt_kkt_diag_dom_warnings, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), k.handle, nwarn) == 0
        for _ in 1:nwarn[]
            println("WARNING: Inertia calculation incorrect")
            @warn("Inertia calculation incorrect")
        end
    end
    # the caller reads old_delta = get_delta(iter) and then calls set_delta(iter, new_delta) itself (one_phase.jl:203-206)
    return rc == 1 ? :success : :failure, Int(num_fac[]), delta[]
end

# kkt_associate_rhs! (schur.jl:34-45, symmetric.jl: same body): System_rhs(iter, reduct_factors) evaluated on the device from
# the iterate's cached gradient / constraint values; the triple stays in HBM for compute_direction! and is also copied
# back, because the IPM reads kkt_solver.rhs (e.g. the merit function).  It also tells the library which iterate is
# current_it, which Schur_KKT_solver_direct reads (schur_direct.jl:35-37).
function kkt_associate_rhs!(k::HIP_KKT_solver, iter::Class_iterate, reduct_factors::Class_reduction_factors, timer::class_advanced_timer)
    start_advanced_timer(timer, "KKT/rhs")
    n = dim(iter); m = ncon(iter)
    rD = zeros(n); rP = zeros(m); rC = zeros(m)
    J = get_jac(iter)
    Jcur = iter === k.factor_it ? C_NULL : pointer(J.nzval)     # NULL: the Jacobian values of form_system! are current
    GC.@preserve J begin
        kkt_hip_check(k, "okkt_kkt_system_rhs", ccall((:okkt_kkt_system_rhs, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64, Float64, Float64,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            k.handle, Jcur, get_grad(iter), get_cons(iter), get_s(iter), get_y(iter), get_mu(iter), iter.a_norm_penalty_par,
            reduct_factors.P, reduct_factors.D, reduct_factors.mu, rD, rP, rC))
    end
    k.rhs = System_rhs(rD, rP, rC)
    k.resident_rhs = k.rhs     # identity, not a flag: reference code that assigns k.rhs afterwards (compute_eigenvector!,
                               # kkt_system_solver.jl:205-228) must get ITS rhs solved, not the stale device copy
    k.dir.mu = -(1.0 - reduct_factors.mu) * get_mu(iter)
    k.dir.primal_scale = -(1.0 - reduct_factors.P) * iter.point.primal_scale
    k.reduct_factors = reduct_factors
    k.current_it = iter
    pause_advanced_timer(timer, "KKT/rhs")
end

function compute_direction_implementation!(k::HIP_KKT_solver, timer::class_advanced_timer)
    n = dim(k.factor_it); m = ncon(k.factor_it)
    dx = zeros(n); dy = zeros(m); ds = zeros(m)
    err = zeros(6)
    # resident rhs (k.rhs is still the object kkt_associate_rhs! created): three NULLs, nothing crosses PCIe on the way in;
    # a rhs the caller replaced on the host is uploaded
    rhs = k.rhs
    resident = rhs === k.resident_rhs
    GC.@preserve rhs begin
        r = resident ? (C_NULL, C_NULL, C_NULL) : (pointer(rhs.dual_r), pointer(rhs.primal_r), pointer(rhs.comp_r))
        kkt_hip_check(k, "okkt_kkt_compute_direction", ccall((:okkt_kkt_compute_direction, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            k.handle, r[1], r[2], r[3], Int32(k.pars.kkt.ItRefine_Num), dx, dy, ds, err))
    end
    k.dir.x = dx; k.dir.y = dy; k.dir.s = ds
    check_for_nan(k.dir)
    k.kkt_err_norm = Class_kkt_error(err[1], err[2], err[3], err[4], err[5], err[6])
end


# Several directions of the same factor in one pass over L: the probe of the aggressive step (Reduct_affine, take_step.jl:2-3) and the
# candidates of take_step2! (take_step.jl:34-66) are right-hand sides of one factorised system.  Returns [(dir, kkt_err_norm)];
# kkt_associate_rhs!(k, iter, ...) must have told the library the current iterate.
function compute_directions!(k::HIP_KKT_solver, etas::Vector{Class_reduction_factors})
    # the same guards as compute_direction_implementation!: the BigFloat refinement of the Schur solvers ends in a MethodError in
    # the reference (schur.jl:167, eval.jl:232), and every returned direction goes through check_for_nan (IPM_tools.jl:32-49).
    # k.dir and k.kkt_err_norm are NOT updated: the caller picks one of the candidates.
    if k.pars.kkt.ItRefine_BigFloat && (k.kind == 0 || k.kind == 3)       # :schur, :schur_direct
        error("MethodError: no method matching hess_product(::Class_iterate, ::Array{BigFloat,1}) (schur.jl:167 with pars.kkt.ItRefine_BigFloat = true)")
    end
    n = dim(k.factor_it); m = ncon(k.factor_it); q = length(etas)
    e = zeros(3 * q)
    for i in 1:q
        e[3i - 2] = etas[i].P; e[3i - 1] = etas[i].D; e[3i] = etas[i].mu
    end
    dx = zeros(n * q); dy = zeros(m * q); ds = zeros(m * q); err = zeros(6 * q)
    kkt_hip_check(k, "okkt_kkt_compute_directions", ccall((:okkt_kkt_compute_directions, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        k.handle, Int32(q), e, Int32(k.pars.kkt.ItRefine_Num), dx, dy, ds, err))
    out = Vector{Tuple{Class_point, Class_kkt_error}}()
    for i in 1:q
        d = Class_point(); d.x = dx[(i - 1) * n + 1:i * n]; d.y = dy[(i - 1) * m + 1:i * m]; d.s = ds[(i - 1) * m + 1:i * m]
        d.mu = -(1.0 - etas[i].mu) * get_mu(k.current_it)
        d.primal_scale = -(1.0 - etas[i].P) * k.current_it.point.primal_scale
        check_for_nan(d)
        r = err[6 * (i - 1) + 1:6 * i]
        push!(out, (d, Class_kkt_error(r[1], r[2], r[3], r[4], r[5], r[6])))
    end
    return out
end

# ---- KKT batches (okkt_kkt_items_*, DESIGN.md section 8.17): B iterates on the structure of one HIP_KKT_solver (:schur without dense
# rows, or :symmetric).  Plain ccalls, UNTESTED like the rest of this file.  A multi-start or sweep driver calls these instead of looping
# over solvers: item b's results are bit for bit those of form_system!, ipopt_strategy!, kkt_associate_rhs! and compute_direction! for
# that iterate on a solver of its own.  Matrices are column-major in Julia: values go in as nnz x B (one column per item), vectors as
# n x B / m x B, which is the [B][..] layout of the C ABI.
struct OkktKktItemsInfo     # okkt_kkt_items_info of include/okkt.h
    eligible::Int32
    reason::Int32
    bytes_per_item::Int64
    launches_form::Int32
    launches_direction::Int32
end

function items_query(k::HIP_KKT_solver)
    info = Ref(OkktKktItemsInfo(0, 0, 0, 0, 0))
    kkt_hip_check(k, "okkt_kkt_items_query", ccall((:okkt_kkt_items_query, OKKT_LIB), Cint, (Ptr{Cvoid}, Ref{OkktKktItemsInfo}), k.handle, info))
    return info[]
end
items_reserve!(k::HIP_KKT_solver, B::Integer) =
    kkt_hip_check(k, "okkt_kkt_items_reserve", ccall((:okkt_kkt_items_reserve, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64), k.handle, B))
items_release!(k::HIP_KKT_solver) =
    kkt_hip_check(k, "okkt_kkt_items_release", ccall((:okkt_kkt_items_release, OKKT_LIB), Cint, (Ptr{Cvoid},), k.handle))

# its: iterates on the structure the solver was given (form_system! of the first one sets it).  A value array that is the same object
# for every item goes in once, with stride 0
function form_system_items!(k::HIP_KKT_solver, its::Vector{Class_iterate})
    B = length(its)
    Hs = [get_lag_hess(it) for it in its]; Js = [get_jac(it) for it in its]
    sameH = all(H -> H.nzval === Hs[1].nzval, Hs); sameJ = all(J -> J.nzval === Js[1].nzval, Js)
    Hx = sameH ? Hs[1].nzval : hcat([H.nzval for H in Hs]...); Jx = sameJ ? Js[1].nzval : hcat([J.nzval for J in Js]...)
    s = hcat([get_s(it) for it in its]...); y = hcat([get_y(it) for it in its]...)
    kkt_hip_check(k, "okkt_kkt_items_form_system", ccall((:okkt_kkt_items_form_system, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
        k.handle, B, Hx, sameH ? 0 : length(Hs[1].nzval), Jx, sameJ ? 0 : length(Js[1].nzval), s, y))
    k.ready = :system_formed
end

function diag_min_items(k::HIP_KKT_solver, B::Integer)
    out = zeros(B)
    kkt_hip_check(k, "okkt_kkt_items_diag_min", ccall((:okkt_kkt_items_diag_min, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), k.handle, B, out))
    return out
end

# factor!(kkt_solver, deltas[b]) for every item: (flags, inertias)
function factor_items!(k::HIP_KKT_solver, deltas::Vector{Float64})
    B = length(deltas)
    inertia = Vector{OkktInertiaCounts}(undef, B); flags = zeros(Int32, B)
    kkt_hip_check(k, "okkt_kkt_items_factor", ccall((:okkt_kkt_items_factor, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{OkktInertiaCounts}, Ptr{Int32}), k.handle, B, deltas, inertia, flags))
    k.ready = :factored
    return flags, inertia
end

# ipopt_strategy! for every item, a round of attempts being ONE batched factorisation over the items still active:
# ([(status, num_fac, delta)], launches)
function ipopt_strategy_items!(its::Vector{Class_iterate}, k::HIP_KKT_solver, pars::Class_parameters)
    B = length(its)
    p = OkktKktPars(pars.delta.start, pars.delta.min, pars.delta.max, pars.delta.inc, pars.delta.dec, pars.delta.zero,
                    Int32(pars.kkt.ItRefine_Num), Int32(500))
    prev = [get_delta(it) for it in its]
    status = zeros(Int32, B); nfac = zeros(Int32, B); warn = zeros(Int32, B); delta = zeros(B); launches = Ref{Int32}(0)
    kkt_hip_check(k, "okkt_kkt_items_ipopt_strategy", ccall((:okkt_kkt_items_ipopt_strategy, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{OkktKktPars}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ref{Int32}),
        k.handle, B, prev, Ref(p), status, nfac, delta, warn, launches))
    for b in 1:B, _ in 1:warn[b]          # delta_strategy.jl:94-98, counted per item by the library
        println("WARNING: Inertia calculation incorrect")
        @warn("Inertia calculation incorrect")
    end
    k.ready = :factored
    # the caller calls set_delta(its[b], delta_b) itself, as after ipopt_strategy! (one_phase.jl:203-206)
    return [(status[b] == 1 ? :success : :failure, Int(nfac[b]), delta[b]) for b in 1:B], Int(launches[])
end

# kkt_associate_rhs! for every item at the iterate it was formed at: [System_rhs]
function kkt_associate_rhs_items!(k::HIP_KKT_solver, its::Vector{Class_iterate}, reduct_factors::Class_reduction_factors)
    B = length(its); n = dim(its[1]); m = ncon(its[1])
    grad = hcat([get_grad(it) for it in its]...); cons = hcat([get_cons(it) for it in its]...)
    s = hcat([get_s(it) for it in its]...); y = hcat([get_y(it) for it in its]...)
    mu = [get_mu(it) for it in its]; pen = [it.a_norm_penalty_par for it in its]
    rD = zeros(n, B); rP = zeros(m, B); rC = zeros(m, B)
    kkt_hip_check(k, "okkt_kkt_items_system_rhs", ccall((:okkt_kkt_items_system_rhs, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        k.handle, B, grad, cons, s, y, mu, pen, reduct_factors.P, reduct_factors.D, reduct_factors.mu, rD, rP, rC))
    return [System_rhs(rD[:, b], rP[:, b], rC[:, b]) for b in 1:B]
end

# compute_direction! for every item: ([Class_point], [Class_kkt_error])
function compute_direction_items!(k::HIP_KKT_solver, its::Vector{Class_iterate}, reduct_factors::Class_reduction_factors)
    B = length(its); n = dim(its[1]); m = ncon(its[1])
    dx = zeros(n, B); dy = zeros(m, B); ds = zeros(m, B); err = zeros(6, B)
    kkt_hip_check(k, "okkt_kkt_items_compute_direction", ccall((:okkt_kkt_items_compute_direction, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        k.handle, B, Int32(k.pars.kkt.ItRefine_Num), dx, dy, ds, err))
    dirs = Vector{Class_point}(); errs = Vector{Class_kkt_error}()
    for b in 1:B
        d = Class_point(); d.x = dx[:, b]; d.y = dy[:, b]; d.s = ds[:, b]
        d.mu = -(1.0 - reduct_factors.mu) * get_mu(its[b])
        d.primal_scale = -(1.0 - reduct_factors.P) * its[b].point.primal_scale
        push!(dirs, d)
        push!(errs, Class_kkt_error(err[1, b], err[2, b], err[3, b], err[4, b], err[5, b], err[6, b]))
    end
    return dirs, errs
end

# slot b (0-based, as in the C ABI) -> the solver's own state: afterwards every single-iterate method behaves as after the serial
# sequence on that iterate
function items_select!(k::HIP_KKT_solver, b::Integer, it::Class_iterate)
    kkt_hip_check(k, "okkt_kkt_items_select", ccall((:okkt_kkt_items_select, OKKT_LIB), Cint, (Ptr{Cvoid}, Int64), k.handle, b))
    k.factor_it = it
    k.resident_rhs = nothing
end

# ---- line-search batches (okkt_kkt_items_max_step_primal ..., DESIGN.md section 8.18): the step-side functions of line_search_hip.jl
# for the items of a KKT batch, against the iterates of form_system_items! and the directions compute_direction_items! left resident
# (or set_direction_items!).  Plain ccalls, UNTESTED like the rest of this file.  Per-item vectors are matrices with one COLUMN per
# item (the [B][m] / [B][n] of the C ABI), per-item scalars vectors of length B; items: nothing for every item, else 0-based slots --
# inputs and outputs stay indexed by slot, and only the listed slots' outputs are written (a backtracking loop passes the items still
# in it).  Item b's numbers are bit for bit those of the single-iterate functions on a solver of its own.
items_arg(items) = items === nothing ? (Ptr{Int32}(C_NULL), Int64(0)) : (pointer(items), Int64(length(items)))
frac_arg(frac, m) = ndims(frac) == 1 ? Int64(0) : Int64(m)          # one fraction vector for every item, or one column per item

function set_direction_items!(k::HIP_KKT_solver, dx::Matrix{Float64}, dy::Matrix{Float64}, ds::Matrix{Float64})
    kkt_hip_check(k, "okkt_kkt_items_set_direction", ccall((:okkt_kkt_items_set_direction, OKKT_LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), k.handle, size(dx, 2), dx, dy, ds))
end

# (step_size_P, norm(dir_b.x, Inf)), vectors of length B
function max_step_primal_items(k::HIP_KKT_solver, B::Integer, frac_bd_predict::Array{Float64}, ex::Float64; items::Union{Nothing,Vector{Int32}}=nothing)
    step = fill(NaN, B); nx = fill(NaN, B)
    GC.@preserve items begin
        ip, ni = items_arg(items)
        kkt_hip_check(k, "okkt_kkt_items_max_step_primal", ccall((:okkt_kkt_items_max_step_primal, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int32}, Int64, Ptr{Float64}, Int64, Float64, Ptr{Float64}, Ptr{Float64}),
            k.handle, B, ip, ni, frac_bd_predict, frac_arg(frac_bd_predict, size(frac_bd_predict, 1)), ex, step, nx))
    end
    return step, nx
end

function s_bound_ok_items(k::HIP_KKT_solver, s_new::Matrix{Float64}, frac_bd::Array{Float64}, ex::Float64; items::Union{Nothing,Vector{Int32}}=nothing)
    m, B = size(s_new)
    ok = fill(Int32(-1), B)
    GC.@preserve items begin
        ip, ni = items_arg(items)
        kkt_hip_check(k, "okkt_kkt_items_s_bound_ok", ccall((:okkt_kkt_items_s_bound_ok, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int32}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Ptr{Int32}),
            k.handle, B, ip, ni, s_new, frac_bd, frac_arg(frac_bd, m), ex, ok))
    end
    return ok
end

# (lb, ub), vectors of length B
function dual_step_range_items(k::HIP_KKT_solver, s_cand::Matrix{Float64}, y_cand::Matrix{Float64}, mu_cand::Vector{Float64}, comp_feas::Float64,
                               frac_bd::Array{Float64}; items::Union{Nothing,Vector{Int32}}=nothing)
    m, B = size(s_cand)
    lb = fill(NaN, B); ub = fill(NaN, B)
    GC.@preserve items begin
        ip, ni = items_arg(items)
        kkt_hip_check(k, "okkt_kkt_items_dual_step_range", ccall((:okkt_kkt_items_dual_step_range, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int32}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
            k.handle, B, ip, ni, s_cand, y_cand, mu_cand, comp_feas, frac_bd, frac_arg(frac_bd, m), lb, ub))
    end
    return lb, ub
end

# 4 x B: (phi_predicted_reduction_primal_dual, |comp|_inf, |comp_predicted|_inf, merit_function_predicted_reduction) per column
function predicted_reduction_items(k::HIP_KKT_solver, grad::Matrix{Float64}, mu::Vector{Float64}, dmu::Vector{Float64}, a_norm_penalty::Vector{Float64},
                                   step_size::Vector{Float64}; items::Union{Nothing,Vector{Int32}}=nothing)
    B = size(grad, 2)
    out = fill(NaN, 4, B)
    GC.@preserve items begin
        ip, ni = items_arg(items)
        kkt_hip_check(k, "okkt_kkt_items_predicted_reduction", ccall((:okkt_kkt_items_predicted_reduction, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int32}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            k.handle, B, ip, ni, grad, mu, dmu, a_norm_penalty, step_size, out))
    end
    return out
end

# step_size_D of move_dual per item; J_nzval_cand: nothing (each item's formed J), a vector (one array for every item) or nnz x B
function dual_step_items(k::HIP_KKT_solver, J_nzval_cand::Union{Nothing,Array{Float64}}, grad_cand::Matrix{Float64}, s_cand::Matrix{Float64},
                         y_cand::Matrix{Float64}, mu_cand::Vector{Float64}, a_norm_penalty::Vector{Float64}, step_size_P::Vector{Float64},
                         lb::Vector{Float64}, ub::Vector{Float64}, scale_D::Vector{Float64}, scale_mu::Vector{Float64}, dual_ls::Integer;
                         items::Union{Nothing,Vector{Int32}}=nothing)
    B = size(s_cand, 2)
    out = fill(NaN, B)
    Jp = J_nzval_cand === nothing ? Ptr{Float64}(C_NULL) : pointer(J_nzval_cand)
    Js = (J_nzval_cand === nothing || ndims(J_nzval_cand) == 1) ? Int64(0) : Int64(size(J_nzval_cand, 1))
    GC.@preserve items J_nzval_cand begin
        ip, ni = items_arg(items)
        kkt_hip_check(k, "okkt_kkt_items_dual_step", ccall((:okkt_kkt_items_dual_step, OKKT_LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int32}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}),
            k.handle, B, ip, ni, Jp, Js, grad_cand, s_cand, y_cand, mu_cand, a_norm_penalty, step_size_P, lb, ub, scale_D, scale_mu, dual_ls, out))
    end
    return out
end

# ---- the dense factor of the Schur complement (DESIGN.md section 8.7) on a linear_solver_HIP in Schur mode (okkt_set_schur before the
# analysis, okkt_factor_schur before these).  UNTESTED like the rest of this file.  Inertias come back as (pos, neg, zero, nonfinite).
struct OkktInertiaCounts    # okkt_inertia of include/okkt.h
    pos::Int64
    neg::Int64
    zero::Int64
    nonfinite::Int64
end

# P S P' = L D L' with Bunch-Kaufman pivoting; S === nothing: the S the handle assembled, else a symmetric ns x ns matrix (lower triangle
# read).  Returns (flag, inertia of S, inertia of the whole matrix); flag 1: no zero and no non-finite pivot
function schur_factor(solver::linear_solver_HIP, S::Union{Nothing,Array{Float64,2}}=nothing)
    si = Ref(OkktInertiaCounts(0, 0, 0, 0)); ti = Ref(OkktInertiaCounts(0, 0, 0, 0))
    rc = ccall((:okkt_schur_factor, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{OkktInertiaCounts}, Ref{OkktInertiaCounts}),
               solver.handle, S === nothing ? C_NULL : pointer(S), S === nothing ? 0 : size(S, 1), si, ti)
    rc < 0 && okkt_error(solver, "okkt_schur_factor", rc)
    return rc, si[], ti[]
end

# x2 = S^-1 r2 (set order); r2 may be x2
function schur_dense_solve(solver::linear_solver_HIP, r2::Array{Float64,1}, x2::Array{Float64,1})
    rc = ccall((:okkt_schur_dense_solve, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), solver.handle, r2, x2, 1)
    rc < 0 && okkt_error(solver, "okkt_schur_dense_solve", rc)
    return x2
end

# A sol = rhs for the whole matrix: one forward sweep over the interior, the dense solve, the backward sweep; rhs may be sol
function schur_solve(solver::linear_solver_HIP, my_rhs::Array{Float64,1}, my_sol::Array{Float64,1})
    rc = ccall((:okkt_schur_solve, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), solver.handle, my_rhs, my_sol, 1)
    rc < 0 && okkt_error(solver, "okkt_schur_solve", rc)
    return my_sol
end

# (LD, ipiv) in the layout and convention of LAPACK.sytrf!('L', S)
function schur_get_factor(solver::linear_solver_HIP, ns::Integer)
    LD = zeros(ns, ns); ipiv = zeros(Int32, ns)
    rc = ccall((:okkt_schur_get_factor, OKKT_LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int32}), solver.handle, LD, ns, ipiv)
    rc < 0 && okkt_error(solver, "okkt_schur_get_factor", rc)
    return LD, ipiv
end
