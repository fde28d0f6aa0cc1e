# MI355Schur.jl — the reference-side binding of libmi355schur (include/mi355schur.h).
#
# Drop this module next to Fem/ and RecyclingKrylovSolvers/ of venkovic/julia-phd-krylov-spdes and
# `push!(LOAD_PATH, "./MI355Schur/")`. It is purely mechanical: every function is one `ccall`.
#
# It EXTENDS the reference's own generic functions with methods on `MiOperator` and never defines a second
# function of the same name: `cg`, `pcg`, `defcg`, `defpcg`, `eigcg`, … are imported from RecyclingKrylovSolvers
# (exports at RecyclingKrylovSolvers.jl:10-13) and `apply_local_schurs`, `apply_global_schur`,
# `apply_neumann_neumann_schur`, `get_schur_rhs`, `get_subdomain_solutions`, `NeumannNeumannSchurPreconditioner`
# from Fem (exports at Fem/Fem.jl:54-75). A script that does `using Fem; using RecyclingKrylovSolvers; using MI355Schur`
# (Example03:6-7 plus one line) therefore keeps every unqualified call site — `pcg(S, b, x, Πnn)` (Example03:193),
# `defpcg(S, b, x, ϕ, Πnn)` (:214, :224) — and Julia's dispatch picks the device method when `S` is a `MiOperator`.
# Only names the reference does not have are exported from here.
#
# NOTE: there is no `julia` in the build container, so this file has been reviewed, not executed;
# tests/test_julia_shim_cpu.py checks it mechanically (no shadowed export, every `ccall` signature against
# include/mi355schur.h, `index_base = 1` at every create).
module MI355Schur

using LinearAlgebra
using SparseArrays: SparseMatrixCSC
import Base: *, \, size
import LinearAlgebra: mul!, ldiv!
import RecyclingKrylovSolvers
import RecyclingKrylovSolvers: cg, pcg, defcg, defpcg, eigcg, eigpcg, eigdefcg, eigdefpcg, initcg, initpcg
import MyPreconditioners
import Fem
import Fem: apply_local_schur, apply_local_schurs, apply_global_schur, apply_neumann_neumann_schur,
            get_schur_rhs, get_subdomain_solutions, NeumannNeumannSchurPreconditioner,
            assemble_local_schurs, prepare_neumann_neumann_schur_precond,
            LorascPreconditioner, prepare_lorasc_precond, apply_lorasc

# new names only (none of them is exported by Fem or RecyclingKrylovSolvers)
export MiContext, MiOperator, MiPrecond,
       LocalSchurs, LocalSchur, MatrixFreeLocalSchurs, GlobalSchur,
       AssemblyPlan, assemble!, set_values!, SchurSetup, set_blocks!, interior_precond!, interior_iterations,
       keep_levels!, interior_solve, use_level_solver!, peer_handle!, peer_connect!, set_exchange!,
       SparseDirectPreconditioner, spd_direct_stats, bj_set_values!, MiLorasc, set_correction!, MiNNInduced, set_coupling!,
       mi_eigsolve, mi_geneigsolve, MiAMGPreconditioner, amg_stats,
       MiKlField, MiMcmcSampler, coefficient!, klfield_stats, MiFullAssembly, jacobi_refresh!,
       MiAMGBank, MiAMGBankView, select!, combine!, amg_bank_stats,
       MiCsrBatch, pcg_batch, csr_batch_stats

const lib = get(ENV, "MI355SCHUR_LIB", "libmi355schur")
const MI_ERR_SINGULAR = Cint(-3)
const MI_ERR_RES_CAPACITY = Cint(-4)
const MI_ERR_BOUNDS = Cint(-8)

function check(rc::Cint)
  rc == 0 && return
  msg = unsafe_string(ccall((:mi_last_error, lib), Cstring, ()))
  rc == MI_ERR_SINGULAR && throw(LinearAlgebra.SingularException(0))   # `WtAW \ mu`, defcg.jl:53,273
  rc == MI_ERR_RES_CAPACITY && throw(BoundsError())                    # res_norm[it], cg.jl:47
  rc == MI_ERR_BOUNDS && throw(BoundsError())                          # V[:, nev+1] / eigvecs(...)[:, 1:nvec], eigcg.jl:101,275
  error("libmi355schur error $rc: $msg")
end

mutable struct MiContext
  h::Ptr{Cvoid}
  function MiContext(device::Integer=0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mi_ctx_create, lib), Cint, (Cint, Ref{Ptr{Cvoid}}), device, r))
    ctx = new(r[])
    finalizer(c -> ccall((:mi_ctx_destroy, lib), Cint, (Ptr{Cvoid},), c.h), ctx)
  end
end

# Anything usable as `A` (A*x, mul!) or as `M` (M \ r, ldiv!). `keep` roots Julia callbacks.
mutable struct MiOperator
  h::Ptr{Cvoid}
  n::Int
  N::Int            # LinearMaps.FunctionMap field read by Example07:273 (`S.N`)
  ctx::MiContext
  keep::Any
end
const MiPrecond = MiOperator

function wrap(ctx::MiContext, r::Ref{Ptr{Cvoid}}, keep=nothing)
  n = Ref{Int64}(0)
  check(ccall((:mi_op_size, lib), Cint, (Ptr{Cvoid}, Ref{Int64}), r[], n))
  op = MiOperator(r[], n[], n[], ctx, keep)
  finalizer(o -> ccall((:mi_op_destroy, lib), Cint, (Ptr{Cvoid},), o.h), op)
end

size(A::MiOperator) = (A.n, A.n)

function mul!(y::Vector{Float64}, A::MiOperator, x::Vector{Float64})     # cg.jl:36,93
  check(ccall((:mi_op_apply, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), A.h, x, y))
  y
end
*(A::MiOperator, x::Vector{Float64}) = mul!(Vector{Float64}(undef, A.n), A, x)   # cg.jl:28,83
\(M::MiOperator, r::Vector{Float64}) = M * r                                     # EPDD.jl:1389-1392
ldiv!(z::Vector{Float64}, M::MiOperator, r::Vector{Float64}) = mul!(z, M, r)     # EPDD.jl:1394-1398
ldiv!(M::MiOperator, r::Vector{Float64}) = (r .= M * copy(r))                    # EPDD.jl:1400-1403

# ---------------------------------------------------------------- flattening of the reference's containers
# ind_Γd_Γ2l[d]::Dict{Int,Int} (lΓ => lΓd, EPDD.jl:186-191)  ->  gather_idx[d][lΓd] = lΓ (1-based kept;
# the library is told index_base = 1).
function flatten_maps(ind_Γd_Γ2l::Vector{Dict{Int,Int}})
  g = [Vector{Int64}(undef, length(m)) for m in ind_Γd_Γ2l]
  for (d, m) in enumerate(ind_Γd_Γ2l), (lΓ, lΓd) in m
    g[d][lΓd] = lΓ
  end
  g
end
ptrs(v::Vector{<:Vector{T}}) where {T} = Ptr{T}[pointer(a) for a in v]

"""`LocalSchurs(ctx, Sd, ind_Γd_Γ2l, node_Γ_cnt)`: the operator `x -> apply_local_schurs(Sd, ind_Γd_Γ2l,
node_Γ_cnt, x)` (EPDD.jl:761-785) that Example03:131-135 wraps in a LinearMap."""
function LocalSchurs(ctx::MiContext, Sd::Vector, ind_Γd_Γ2l::Vector{Dict{Int,Int}}, node_Γ_cnt::Vector{Int};
                     dom_range=(0, length(Sd)))
  ndom = length(Sd); g = flatten_maps(ind_Γd_Γ2l); nd = Int64[length(x) for x in g]
  blocks = [Matrix{Float64}(S) for S in Sd]              # `Array(Sd[idom])`, column-major
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve g blocks begin
    check(ccall((:mi_schur_assembled_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Cint, Int64, Int64, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, length(node_Γ_cnt), nd, ptrs(g), Ptr{Float64}[pointer(b) for b in blocks], 1,
                dom_range[1], dom_range[2], r))
  end
  wrap(ctx, r)
end

"""`NeumannNeumannSchurPreconditioner(ctx, ΠSd, ind_Γd_Γ2l, node_Γ_cnt)`: a method added to the constructor of Fem's
own struct (EPDD.jl:1111-1137; its fields are `ΠSd`, `ind_Γd_Γ2l`, `node_Γ_cnt`): with a `MiContext` in front the blocks
go to the device and a `MiOperator` comes back, usable wherever the reference uses `Πnn \\ r` / `ldiv!` (:1389-1403).
`storage=Float32` holds the blocks as fp32 on the device (rounded once; the apply and the solvers stay fp64, half the
bytes are streamed) — storage only, unlike `Cholesky32` of MyPreconditioners/CholPreconditioners.jl:32-56, which also
solves in fp32."""
function NeumannNeumannSchurPreconditioner(ctx::MiContext, ΠSd::Vector{Matrix{Float64}},
                                           ind_Γd_Γ2l::Vector{Dict{Int,Int}}, node_Γ_cnt::Vector{Int};
                                           dom_range=(0, length(ΠSd)), storage::Type=Float64)
  storage === Float64 || storage === Float32 || error("storage must be Float64 or Float32")
  st = storage === Float32 ? 1 : 0   # MI_STORE_F32 / MI_STORE_F64
  ndom = length(ΠSd); g = flatten_maps(ind_Γd_Γ2l); nd = Int64[length(x) for x in g]
  cnt = Vector{Int64}(node_Γ_cnt)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve g ΠSd cnt begin
    if st == 0
      check(ccall((:mi_nn_create, lib), Cint,
                  (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Cint, Int64, Int64, Ref{Ptr{Cvoid}}),
                  ctx.h, ndom, length(cnt), nd, ptrs(g), Ptr{Float64}[pointer(b) for b in ΠSd], cnt, 1,
                  dom_range[1], dom_range[2], r))
    else
      check(ccall((:mi_nn_create_stored, lib), Cint,
                  (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Cint, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
                  ctx.h, ndom, length(cnt), nd, ptrs(g), Ptr{Float64}[pointer(b) for b in ΠSd], cnt, 1,
                  dom_range[1], dom_range[2], st, r))
    end
  end
  wrap(ctx, r)
end

# Interior solve callback: `interior(idom, rhs) -> A_II[idom] \ rhs`, e.g. a CHOLMOD factor or
# `rhs -> IterativeSolvers.cg(A_IIdd[idom], rhs, Pl=Π_IId[idom], reltol=1e-9)` (EPDD.jl:648-650).
function interior_trampoline(user::Ptr{Cvoid}, idom::Int64, n::Int64, rhs::Ptr{Float64}, sol::Ptr{Float64})::Cint
  f = unsafe_pointer_to_objref(user)[]
  try
    unsafe_wrap(Array, sol, n) .= f(Int(idom) + 1, copy(unsafe_wrap(Array, rhs, n)))
    return Cint(0)
  catch
    return Cint(1)
  end
end

csc_parts(As::Vector{SparseMatrixCSC{Float64,Int}}) =
  ([Vector{Int64}(A.colptr) for A in As], [Vector{Int64}(A.rowval) for A in As], [A.nzval for A in As])

"""`MatrixFreeLocalSchurs(ctx, A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt, interior)`: the operator of
Example03:143-150, `apply_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, ...)` (EPDD.jl:711-747); sparse products on the
GPU, `A_IIdd^{-1}` through `interior(idom, rhs)` on the host."""
function MatrixFreeLocalSchurs(ctx::MiContext, A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt, interior)
  ndom = length(A_IΓdd); g = flatten_maps(ind_Γd_Γ2l)
  nd = Int64[length(x) for x in g]; ni = Int64[A.n for A in A_IIdd]
  igp, igi, igv = csc_parts(A_IΓdd); ggp, ggi, ggv = csc_parts(A_ΓΓdd)
  fref = Ref{Any}(interior)
  cb = @cfunction(interior_trampoline, Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}))
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve g igp igi igv ggp ggi ggv fref begin
    check(ccall((:mi_schur_matfree_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}},
                 Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}},
                 Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Int64, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, length(node_Γ_cnt), nd, ni, ptrs(g), ptrs(igp), ptrs(igi), ptrs(igv),
                ptrs(ggp), ptrs(ggi), ptrs(ggv), cb, pointer_from_objref(fref), 1, 0, ndom, r))
  end
  wrap(ctx, r, (fref, cb))
end

"""`MatrixFreeLocalSchurs(ctx, A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt; reltol=1e-9)`: the same operator with the
interior solve on the device — the library's restatement of `IterativeSolvers.cg(A_IIdd[idom], rhs, reltol=reltol)`
(EPDD.jl:648-650), all local subdomains iterated together."""
function MatrixFreeLocalSchurs(ctx::MiContext, A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt; reltol=1e-9)
  ndom = length(A_IΓdd); g = flatten_maps(ind_Γd_Γ2l)
  nd = Int64[length(x) for x in g]; ni = Int64[A.n for A in A_IIdd]
  iip, iii, iiv = csc_parts(A_IIdd); igp, igi, igv = csc_parts(A_IΓdd); ggp, ggi, ggv = csc_parts(A_ΓΓdd)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve g iip iii iiv igp igi igv ggp ggi ggv begin
    check(ccall((:mi_schur_matfree_device_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}},
                 Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}},
                 Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Float64, Cint, Int64, Int64, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, length(node_Γ_cnt), nd, ni, ptrs(g), ptrs(iip), ptrs(iii), ptrs(iiv),
                ptrs(igp), ptrs(igi), ptrs(igv), ptrs(ggp), ptrs(ggi), ptrs(ggv), reltol, 1, 0, ndom, r))
  end
  wrap(ctx, r)
end

"""`GlobalSchur(ctx, A_IId, A_IΓd, A_ΓΓ, interior)`: `x -> apply_global_schur(A_IId, A_IΓd, A_ΓΓ, x)`
(EPDD.jl:596-625), the operator of Example03:101."""
function GlobalSchur(ctx::MiContext, A_IId, A_IΓd, A_ΓΓ::SparseMatrixCSC{Float64,Int}, interior)
  ndom = length(A_IΓd); ni = Int64[A.n for A in A_IId]
  igp, igi, igv = csc_parts(A_IΓd)
  ggp, ggi = Vector{Int64}(A_ΓΓ.colptr), Vector{Int64}(A_ΓΓ.rowval)
  fref = Ref{Any}(interior)
  cb = @cfunction(interior_trampoline, Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}))
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve igp igi igv ggp ggi fref begin
    check(ccall((:mi_schur_global_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}},
                 Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, A_ΓΓ.n, ni, ptrs(igp), ptrs(igi), ptrs(igv), ggp, ggi, A_ΓΓ.nzval,
                cb, pointer_from_objref(fref), 1, r))
  end
  wrap(ctx, r, (fref, cb))
end

"""`GlobalSchur(ctx, A_IId, A_IΓd, A_ΓΓ; reltol=sqrt(eps()))`: the same operator with the interior solves on the device
(`IterativeSolvers.cg(A_IId[idom], A_IΓd[idom]*x)` restated, EPDD.jl:609-619; sqrt(eps) is that package's default)."""
function GlobalSchur(ctx::MiContext, A_IId, A_IΓd, A_ΓΓ::SparseMatrixCSC{Float64,Int}; reltol=sqrt(eps(Float64)))
  ndom = length(A_IΓd); ni = Int64[A.n for A in A_IId]
  iip, iii, iiv = csc_parts(A_IId); igp, igi, igv = csc_parts(A_IΓd)
  ggp, ggi = Vector{Int64}(A_ΓΓ.colptr), Vector{Int64}(A_ΓΓ.rowval)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve iip iii iiv igp igi igv ggp ggi begin
    check(ccall((:mi_schur_global_device_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}},
                 Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Float64, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, A_ΓΓ.n, ni, ptrs(iip), ptrs(iii), ptrs(iiv), ptrs(igp), ptrs(igi), ptrs(igv),
                ggp, ggi, A_ΓΓ.nzval, reltol, 1, r))
  end
  wrap(ctx, r)
end

"""A symmetric `SparseMatrixCSC` as a device operator (config 2: `pcg(A, b, x, M)` on the full system)."""
function MiOperator(ctx::MiContext, A::SparseMatrixCSC{Float64,Int})
  r = Ref{Ptr{Cvoid}}(C_NULL)
  cp, rv = Vector{Int64}(A.colptr), Vector{Int64}(A.rowval)
  check(ccall((:mi_csr_create, lib), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
              ctx.h, A.m, A.n, cp, rv, A.nzval, 1, r))
  wrap(ctx, r)
end

"""`MiOperator(ctx, Πnn::NeumannNeumannSchurPreconditioner)`: the reference's own preconditioner object — what
`prepare_neumann_neumann_schur_precond(Sd_local_mat, ind_Γd_Γ2l, node_Γ_cnt)` returns (EPDD.jl:1201-1220; Example03:139,
Example07:152-154) — copied to the device as it is."""
MiOperator(ctx::MiContext, Πnn::NeumannNeumannSchurPreconditioner) =
  NeumannNeumannSchurPreconditioner(ctx, Πnn.ΠSd, Πnn.ind_Γd_Γ2l, Πnn.node_Γ_cnt)

"""`LocalSchur(ctx, A_IIdd, A_IΓdd, A_ΓΓdd; reltol=1e-9)`: ONE subdomain, `xd -> apply_local_schur(A_IIdd, A_IΓdd,
A_ΓΓdd, xd; reltol)` (EPDD.jl:639-654) in its own Γ_d numbering, interior solve on the device."""
function LocalSchur(ctx::MiContext, A_IIdd::SparseMatrixCSC{Float64,Int}, A_IΓdd::SparseMatrixCSC{Float64,Int},
                    A_ΓΓdd::SparseMatrixCSC{Float64,Int}; reltol=1e-9)
  n = A_ΓΓdd.n
  MatrixFreeLocalSchurs(ctx, [A_IIdd], [A_IΓdd], [A_ΓΓdd], [Dict{Int,Int}(i => i for i in 1:n)], ones(Int, n); reltol=reltol)
end

# Methods added to the reference's own functions (EPDD.jl:639, 711, 761, 596, 1361): the operator handle takes the
# place of the block arrays, the vector argument stays last.
apply_local_schur(S::MiOperator, xd::Vector{Float64}) = S * xd
apply_local_schurs(S::MiOperator, x::Vector{Float64}) = S * x
apply_global_schur(S::MiOperator, x::Vector{Float64}) = S * x
apply_neumann_neumann_schur(Πnn::MiOperator, r::Vector{Float64}) = Πnn * r

# ---------------------------------------------------------------- set-up of the assembled mode on the device
# Methods added to Fem's `assemble_local_schurs` (EPDD.jl:667-695) and `prepare_neumann_neumann_schur_precond` (:1201-1220):
# with a MiContext in front the dense S_d come from the device's exact level elimination (mi_schur_setup_*) and the
# pseudo-inverses from mi_nn_pinv; return types are what LocalSchurs / the device preconditioner take.
mutable struct SchurSetup
  h::Ptr{Cvoid}; n_Γd::Vector{Int64}; ctx::MiContext
end
function SchurSetup(ctx::MiContext, A_IIdd::Vector{SparseMatrixCSC{Float64,Int}}, A_IΓdd::Vector{SparseMatrixCSC{Float64,Int}},
                    A_ΓΓdd::Vector{SparseMatrixCSC{Float64,Int}})
  ndom = length(A_IΓdd)
  nd = Int64[A.n for A in A_ΓΓdd]; ni = Int64[A.n for A in A_IIdd]
  iip, iii, _ = csc_parts(A_IIdd); igp, igi, _ = csc_parts(A_IΓdd); ggp, ggi, _ = csc_parts(A_ΓΓdd)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve iip iii igp igi ggp ggi begin
    check(ccall((:mi_schur_setup_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}},
                 Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, nd, ni, ptrs(iip), ptrs(iii), ptrs(igp), ptrs(igi), ptrs(ggp), ptrs(ggi), 1, r))
  end
  p = SchurSetup(r[], nd, ctx)
  finalizer(q -> ccall((:mi_schur_setup_destroy, lib), Cint, (Ptr{Cvoid},), q.h), p)
end
"""`assemble_local_schurs(plan, A_IIdd, A_IΓdd, A_ΓΓdd[, b_Id])`: one realization on a plan built once for the sparsity; returns
the dense S_d (and, with b_Id, the condensed right-hand sides A_IΓdd' (A_IIdd \\ b_Id) of `get_schur_rhs`, EPDD.jl:853-861)."""
function assemble_local_schurs(p::SchurSetup, A_IIdd, A_IΓdd, A_ΓΓdd, b_Id=nothing)
  ii = reduce(vcat, [A.nzval for A in A_IIdd]); ig = reduce(vcat, [A.nzval for A in A_IΓdd]); gg = reduce(vcat, [A.nzval for A in A_ΓΓdd])
  Sd = Vector{Float64}(undef, sum(p.n_Γd .^ 2)); w = Vector{Float64}(undef, sum(p.n_Γd))
  bI = b_Id === nothing ? C_NULL : reduce(vcat, b_Id)
  check(ccall((:mi_schur_setup_run, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              p.h, ii, ig, gg, bI, Sd, b_Id === nothing ? C_NULL : w))
  ends = cumsum(p.n_Γd .^ 2)
  S = [reshape(Sd[(e - n * n + 1):e], n, n) for (e, n) in zip(ends, p.n_Γd)]
  b_Id === nothing && return S
  we = cumsum(p.n_Γd)
  return S, [w[(e - n + 1):e] for (e, n) in zip(we, p.n_Γd)]
end
assemble_local_schurs(ctx::MiContext, A_IIdd, A_IΓdd, A_ΓΓdd) = assemble_local_schurs(SchurSetup(ctx, A_IIdd, A_IΓdd, A_ΓΓdd), A_IIdd, A_IΓdd, A_ΓΓdd)
"""`prepare_neumann_neumann_schur_precond(ctx, Sd, ind_Γd_Γ2l, node_Γ_cnt)`: ΠS_d = pinv(S_d, rtol = sqrt(eps)) on the device
(EPDD.jl:1211) and the device preconditioner built from them."""
function prepare_neumann_neumann_schur_precond(ctx::MiContext, Sd::Vector{Matrix{Float64}}, ind_Γd_Γ2l::Vector{Dict{Int,Int}},
                                               node_Γ_cnt::Vector{Int})
  nd = Int64[size(S, 1) for S in Sd]
  cat = reduce(vcat, [vec(S) for S in Sd]); out = similar(cat)
  check(ccall((:mi_nn_pinv, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Float64, Ptr{Float64}), ctx.h, length(Sd), nd, cat, 0.0, out))
  ends = cumsum(nd .^ 2)
  ΠSd = [reshape(out[(e - n * n + 1):e], n, n) for (e, n) in zip(ends, nd)]
  NeumannNeumannSchurPreconditioner(ctx, ΠSd, ind_Γd_Γ2l, node_Γ_cnt)
end
"""New S_d / ΠS_d on an existing device operator (same maps): Example07's per-realization update without re-creating it."""
set_blocks!(op::MiOperator, blocks::Vector{Matrix{Float64}}) =
  check(ccall((:mi_dense_set_blocks, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), op.h, reduce(vcat, [vec(B) for B in blocks])))

"""`keep_levels!(plan)`: the next `assemble_local_schurs(plan, …)` keeps the elimination's factors on the device, after which
`interior_solve(plan, f)` is the exact `A_IIdd \\ f_d` of every subdomain (the reference's Cholesky solve, EPDD.jl:649, as
level sweeps) and `use_level_solver!(S, plan)` makes a matrix-free operator use it instead of its inner CG."""
keep_levels!(p::SchurSetup, on::Bool=true) = check(ccall((:mi_schur_setup_keep_levels, lib), Cint, (Ptr{Cvoid}, Cint), p.h, on ? 1 : 0))
function interior_solve(p::SchurSetup, f::Vector{Float64})
  u = similar(f)
  check(ccall((:mi_schur_setup_interior_solve, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), p.h, f, u))
  u
end
function use_level_solver!(S::MiOperator, p::SchurSetup)
  check(ccall((:mi_schur_matfree_interior_levels, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), S.h, p.h))
  S.keep = (S.keep, p)   # the plan outlives S: while S is bound the library refuses the mi_schur_setup_destroy of p's finalizer
  nothing
end

# ---------------------------------------------------------------- one Julia worker per GPU
# The reference's sketch of the distributed apply is `@sync @distributed (+) for idom` (EllipticPdePllDomainDecomposition.jl:
# 10-14). Here every worker owns a context on its own GPU and a slice of the subdomains (`dom_range` of LocalSchurs /
# NeumannNeumannSchurPreconditioner); the Γ-sum of every iteration is the library's peer exchange (include/mi355schur.h):
#   handles = [remotecall_fetch(() -> peer_handle!(ctx, r, np), workers()[r + 1]) for r in 0:np-1]     # 64 bytes each
#   @everywhere peer_connect!(ctx, myrank, handles)
# after which `pcg(S, b, x, Πnn)` on every worker runs the sharded loop and returns the same bits everywhere.
const MI_PEER_HANDLE_BYTES = 64
function peer_handle!(ctx::MiContext, rank::Integer, n_ranks::Integer)
  check(ccall((:mi_ctx_peer_init, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Int64), ctx.h, rank, n_ranks, 0))
  h = Vector{UInt8}(undef, MI_PEER_HANDLE_BYTES); base = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:mi_ctx_peer_export, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), ctx.h, h, base))
  h
end
function peer_connect!(ctx::MiContext, rank::Integer, handles::Vector{Vector{UInt8}})
  for q in 0:length(handles)-1
    q == rank && continue
    check(ccall((:mi_ctx_peer_import, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}), ctx.h, q, handles[q + 1], C_NULL))
  end
  check(ccall((:mi_ctx_peer_ready, lib), Cint, (Ptr{Cvoid},), ctx.h))
end
"""0: off; 1: peer exchange with wait kernels between the launches; 2: the launches wait themselves (one GPU per worker)."""
set_exchange!(ctx::MiContext, mode::Integer) = check(ccall((:mi_ctx_set_exchange, lib), Cint, (Ptr{Cvoid}, Cint), ctx.h, mode))

# ---------------------------------------------------------------- solver drop-ins (whole loop on the GPU)
# Same positional order, keyword and 3-tuple return as RecyclingKrylovSolvers (cg.jl:14,67; defcg.jl:24,242).
function solve(sym::Symbol, A::MiOperator, M, b::Vector{Float64}, x::Vector{Float64}, W, maxit::Int)
  n = A.n
  res = Vector{Float64}(undef, n)                      # cg.jl:23 `res_norm = Array{T,1}(undef, n)`
  it = Ref{Int64}(0)
  rc = if sym == :cg
    ccall((:mi_cg, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}),
          A.h, b, x, maxit, 1e-7, res, n, it)
  elseif sym == :pcg
    ccall((:mi_pcg, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}),
          A.h, M.h, b, x, maxit, 1e-7, res, n, it)
  elseif sym == :defcg
    ccall((:mi_defcg, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}),
          A.h, b, x, W, size(W, 2), maxit, 1e-7, res, n, it)
  else
    ccall((:mi_defpcg, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}),
          A.h, M.h, b, x, W, size(W, 2), maxit, 1e-7, res, n, it)
  end
  check(rc)
  return x, Int(it[]), res[1:it[]]
end

cg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}; maxit=0) = solve(:cg, A, nothing, b, x, nothing, maxit)
pcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiOperator; maxit=0) = solve(:pcg, A, M, b, x, nothing, maxit)
defcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}; maxit=0) = solve(:defcg, A, nothing, b, x, W, maxit)
defpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, M::MiOperator; maxit=0) = solve(:defpcg, A, M, b, x, W, maxit)

# On-device numeric assembly (the element loop of prepare_local_schurs, EPDD.jl:389-546, for a new coefficient vector).
# `cptr`/`ccode` (0-based, Int64) are recorded ONCE by running that loop symbolically: wherever the reference pushes
# (I, J, ΔKij) or does `b[k] += Δ` for element iel and local pair (i, j), record the code 12*(iel-1) + 3*(i-1) + (j-1)
# (or 12*(iel-1) + 9 + (i-1) for a load term) under the stored entry it lands in, in loop order.
mutable struct AssemblyPlan
  h::Ptr{Cvoid}; n_node::Int; n_entries::Int; ctx
end
function AssemblyPlan(ctx::MiContext, cells::Matrix{Int}, n_node::Int, G::Matrix{Float64}, area::Vector{Float64},
                      ue::Matrix{Float64}, be::Matrix{Float64}, n_matrix_entries::Int, cptr::Vector{Int64}, ccode::Vector{Int64})
  nel = size(cells, 2)
  ct = permutedims(cells)                  # library layout: vertex i of every element contiguous (3 x nel row-major)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:mi_assembly_plan_create, lib), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
        ctx.h, nel, n_node, ct, 1, permutedims(G), area, permutedims(ue), permutedims(be), length(cptr) - 1, n_matrix_entries, cptr, ccode, h))
  p = AssemblyPlan(h[], n_node, length(cptr) - 1, ctx)
  finalizer(q -> ccall((:mi_assembly_plan_destroy, lib), Cint, (Ptr{Cvoid},), q.h), p)
  return p
end
function assemble!(values::Vector{Float64}, p::AssemblyPlan, a::Vector{Float64})
  check(ccall((:mi_assembly_run, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), p.h, a, values)); values
end
# On-device FULL-system assembly (DESIGN §6k): the element loop of `update_isotropic_elliptic_assembly!`
# (Fem/EllipticPde.jl:291-377) for a new coefficient vector, into the device operator of A_mat. `MiFullAssembly(ctx, A_mat,
# cells, points, point_marker, f, u_exact)` prepares the row-owned index plan ONCE (A_mat: the matrix of
# `do_isotropic_elliptic_assembly`, for its pattern; it is symmetric, so its CSC arrays are the CSR arrays the library takes);
# per realization `update_isotropic_elliptic_assembly!(A_op, plan, b_vec, coeff)` then replaces the reference's call. The
# handle is the library's `mi_plan_t`, freed by `mi_assembly_plan_destroy` like an `AssemblyPlan`'s.
mutable struct MiFullAssembly
  h::Ptr{Cvoid}; n_node::Int; n::Int; nnz::Int; ctx
end
function MiFullAssembly(ctx::MiContext, A_mat::SparseMatrixCSC{Float64,Int}, cells::Array{Int,2}, points::Array{Float64,2},
                        point_marker::Array{Int,2}, f::Function, u_exact::Function)
  nel, n_node = size(cells, 2), size(points, 2)
  ue, be = Matrix{Float64}(undef, nel, 3), Matrix{Float64}(undef, nel, 3)   # nel x 3 column-major: the library's 3 x nel rows
  for iel in 1:nel
    c = cells[:, iel]
    x, y = points[1, c], points[2, c]
    Area = ((x[2] - x[1]) * (y[3] - y[1]) - (x[1] - x[3]) * (y[1] - y[2])) / 2.      # :331, Δx[3] Δy[2] - Δx[2] Δy[3]
    for i in 1:3
      j, k = mod1(i + 1, 3), mod1(i + 2, 3)
      ue[iel, i] = u_exact(x[i], y[i])                                                # :357
      be[iel, i] = (2 * f(x[i], y[i]) + f(x[j], y[j]) + f(x[k], y[k])) * Area / 12   # :371-373
    end
  end
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:mi_full_assembly_plan_create, lib), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Cint, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
        ctx.h, nel, n_node, permutedims(cells), 1, permutedims(points), Vector{Int64}(vec(point_marker)), A_mat.n,
        Vector{Int64}(A_mat.colptr), Vector{Int64}(A_mat.rowval), ue, be, h))
  p = MiFullAssembly(h[], n_node, A_mat.n, length(A_mat.nzval), ctx)
  finalizer(q -> ccall((:mi_assembly_plan_destroy, lib), Cint, (Ptr{Cvoid},), q.h), p)
  return p
end
"""`assemble!(values, b_vec, p::MiFullAssembly, coeff)`: `A_mat.nzval` and `b_vec` of the new realization, on the host."""
function assemble!(values::Vector{Float64}, b_vec::Vector{Float64}, p::MiFullAssembly, coeff::Vector{Float64})
  check(ccall((:mi_full_assembly_run, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), p.h, coeff, values, b_vec))
  values, b_vec
end
"""`update_isotropic_elliptic_assembly!(A_op, p, b_vec, coeff)`: the reference's in-place update (EllipticPde.jl:291-377) with
the device operator of A_mat and the plan in place of the mesh arguments: the new values go straight into `A_op` (its solve
graphs stay valid), `b_vec` is overwritten."""
function Fem.update_isotropic_elliptic_assembly!(A_op::MiOperator, p::MiFullAssembly, b_vec::Vector{Float64}, coeff::Vector{Float64})
  check(ccall((:mi_full_assembly_update, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}), p.h, coeff, A_op.h, b_vec))
  b_vec
end
"""`set_values!(A_op, nzval)`: new values on the pattern of `MiOperator(ctx, A)` (`mi_csr_set_values`)."""
set_values!(A_op::MiOperator, nzval::Vector{Float64}) = check(ccall((:mi_csr_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), A_op.h, nzval))
"""`jacobi_refresh!(M, A_op)`: `dinv = 1 ./ diag(A)` of the values `A_op` holds now, on the device (`mi_diag_set_from_csr`)."""
jacobi_refresh!(M::MiOperator, A_op::MiOperator) = check(ccall((:mi_diag_set_from_csr, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), M.h, A_op.h))
set_values!(S::MiOperator, ii, ig, gg) =
  check(ccall((:mi_schur_matfree_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              S.h, ii === nothing ? C_NULL : ii, ig === nothing ? C_NULL : ig, gg === nothing ? C_NULL : gg))
"""`interior_precond!(S, :diagonal)`: the `precond(s)` keyword of apply_local_schur(s) / apply_global_schur (EPDD.jl:648-650)
for the device interior CG — `:none` (default, plain CG) or `:diagonal` (`Pl = Diagonal(A_IIdd)`)."""
interior_precond!(S::MiOperator, kind::Symbol) =
  check(ccall((:mi_schur_interior_precond, lib), Cint, (Ptr{Cvoid}, Cint), S.h, kind === :diagonal ? 1 : 0))
"""`interior_amg!(S, n_l, agg)`: `Pl` = smoothed-aggregation AMG for the device interior CG (`mi_schur_interior_amg`), the
reference's `cg(A_IId, rhs; Pl = Π_IId, reltol)`. One hierarchy of blockdiag(A_IIdd): `n_l` the level sizes, `agg[l]` the
1-based aggregate of every stacked node of level `l`; the numbers are made on the device from the operator's values and
redone by `set_values!(S, ii, ...)`. `interior_precond!(S, :none | :diagonal)` switches back."""
function interior_amg!(S::MiOperator, n_l::Vector{Int64}, agg::Vector{Vector{Int64}})
  length(agg) == length(n_l) - 1 || error("interior_amg!: one aggregate array per smoothed level")
  GC.@preserve agg begin
    ptrs = Ptr{Int64}[pointer(a) for a in agg]
    check(ccall((:mi_schur_interior_amg, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Cint),
                S.h, length(n_l), n_l, isempty(ptrs) ? C_NULL : ptrs, 1))
  end
  S
end
function interior_amg_stats(S::MiOperator)
  l, c, b = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
  check(ccall((:mi_schur_interior_amg_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), S.h, l, c, b))
  (levels = l[], coarse_n = c[], bytes_kept = b[])
end
function interior_iterations(S::MiOperator)
  it = Ref{Int64}(0)
  check(ccall((:mi_schur_interior_iterations, lib), Cint, (Ptr{Cvoid}, Ref{Int64}), S.h, it)); it[]
end
function get_schur_rhs(S::MiOperator, b_I::Vector{Float64}, b_Γ::Vector{Float64})      # EPDD.jl:835-864
  out = similar(b_Γ)
  check(ccall((:mi_schur_matfree_rhs, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), S.h, b_I, b_Γ, out)); out
end
# the reference's own container: b_Id::Vector{Vector{Float64}} (one vector per subdomain), concatenated for the library
get_schur_rhs(S::MiOperator, b_Id::Vector{Vector{Float64}}, b_Γ::Vector{Float64}) = get_schur_rhs(S, reduce(vcat, b_Id), b_Γ)
"""`get_subdomain_solutions(S, u_Γ, b_Id)` (EPDD.jl:1014-1025): `u_Id = A_IId \\ (b_Id - A_IΓd u_Γ)` with the operator's
own interior solve; returns one vector per subdomain like the reference."""
function get_subdomain_solutions(S::MiOperator, u_Γ::Vector{Float64}, b_Id::Vector{Vector{Float64}})
  b_I = reduce(vcat, b_Id); u_I = similar(b_I)
  check(ccall((:mi_schur_matfree_interior_solutions, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              S.h, u_Γ, b_I, u_I))
  ends = cumsum(length.(b_Id))
  [u_I[(e - length(b) + 1):e] for (e, b) in zip(ends, b_Id)]
end

# eigCG family and Init-CG (eigcg.jl:27-33, 143-150; defcg.jl:111-116, 337-343; initcg.jl:28-33, 106-111).
# Same positional orders and 4-tuple / 3-tuple returns as the reference (Example09_..._Functions.jl:314, 364).
function eigsolve(kind::Symbol, A::MiOperator, M, b::Vector{Float64}, x::Vector{Float64}, W, nvec::Int, spdim::Int, maxit::Int)
  n = A.n
  res = Vector{Float64}(undef, n); it = Ref{Int64}(0)
  V = Matrix{Float64}(undef, n, nvec)
  tail = (Int64(spdim), Int64(maxit), 1e-7, res, Int64(n), it, V)
  rc = if kind == :eigcg
    ccall((:mi_eigcg, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}),
          A.h, b, x, Int64(nvec), tail...)
  elseif kind == :eigpcg
    ccall((:mi_eigpcg, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}),
          A.h, M.h, b, x, Int64(nvec), tail...)
  elseif kind == :eigdefcg
    ccall((:mi_eigdefcg, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}),
          A.h, b, x, W, Int64(nvec), tail...)
  else
    ccall((:mi_eigdefpcg, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}),
          A.h, M.h, b, x, W, Int64(nvec), tail...)
  end
  check(rc)
  return x, Int(it[]), res[1:it[]], V
end

eigcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, nvec::Int, spdim::Int; maxit=0) =
  eigsolve(:eigcg, A, nothing, b, x, nothing, nvec, spdim, maxit)
eigpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiOperator, nvec::Int, spdim::Int; maxit=0) =
  eigsolve(:eigpcg, A, M, b, x, nothing, nvec, spdim, maxit)
eigdefcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, spdim::Int; maxit=0) =
  eigsolve(:eigdefcg, A, nothing, b, x, W, size(W, 2), spdim, maxit)
eigdefpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiOperator, W::Matrix{Float64}, spdim::Int; maxit=0) =
  eigsolve(:eigdefpcg, A, M, b, x, W, size(W, 2), spdim, maxit)

function initsolve(A::MiOperator, M, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, maxit::Int)
  n = A.n
  res = Vector{Float64}(undef, n); it = Ref{Int64}(0)
  rc = if M === nothing
    ccall((:mi_initcg, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}),
          A.h, b, x, W, size(W, 2), maxit, 1e-7, res, n, it)
  else
    ccall((:mi_initpcg, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Float64}, Int64, Ref{Int64}),
          A.h, M.h, b, x, W, size(W, 2), maxit, 1e-7, res, n, it)
  end
  check(rc)
  return x, Int(it[]), res[1:it[]]
end
initcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}; maxit=0) = initsolve(A, nothing, b, x, W, maxit)
initpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiOperator, W::Matrix{Float64}; maxit=0) = initsolve(A, M, b, x, W, maxit)

# ---------------------------------------------------------------- eigensolver (thick-restart Lanczos on the device)
# KrylovKit.eigsolve(x -> S_local_mat*x, n_Γ, nev, :SR | :LR, krylovdim=2*nev) (Example03:209/219) and
# KrylovKit.geneigsolve(x -> (S*x, A_ΓΓ*x), n_Γ, nvec, :SR, krylovdim=2*nvec, isposdef=true) (EPDD.jl:1546-1549) in KrylovKit's
# return shape (vals, [vec₁, …], info); info has KrylovKit.ConvergenceInfo's field names. `tol` is absolute, as KrylovKit's.
# Arpack.eigs(A, nev, :SM) (Example03:311): mi_eigsolve(BJPreconditioner(ctx, 1, A), nev, :LR), λ = 1 ./ vals.
function lanczos_call(A::MiOperator, B, Binv, nev::Int, which::Symbol, krylovdim::Int, tol::Float64, maxiter::Int, v0)
  which in (:SR, :LR) || error("which = $which: :SR or :LR expected")
  n = A.n
  vals = Vector{Float64}(undef, nev); resid = Vector{Float64}(undef, nev)
  X = Matrix{Float64}(undef, n, nev)
  nconv = Ref{Int64}(0); nrestart = Ref{Int64}(0); napply = Ref{Int64}(0)
  hB = B === nothing ? C_NULL : B.h
  hBinv = Binv === nothing ? C_NULL : Binv.h
  start = v0 === nothing ? Ptr{Float64}(C_NULL) : pointer(v0)
  GC.@preserve v0 check(ccall((:mi_eigsolve, lib), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Int64, Float64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
              A.h, hB, hBinv, Int64(nev), Cint(which == :SR ? 0 : 1), Int64(krylovdim), tol, Int64(maxiter), start, vals, X,
              resid, nconv, nrestart, napply))
  info = (converged = Int(nconv[]), normres = resid, numiter = Int(nrestart[]), numops = Int(napply[]))
  return vals, [X[:, k] for k in 1:nev], info
end
mi_eigsolve(A::MiOperator, nev::Int, which::Symbol=:SR; krylovdim::Int=0, tol::Float64=1e-12, maxiter::Int=100, v0=nothing) =
  lanczos_call(A, nothing, nothing, nev, which, krylovdim, tol, maxiter, v0)
mi_geneigsolve(A::MiOperator, B::MiOperator, Binv::MiOperator, nev::Int, which::Symbol=:SR; krylovdim::Int=0, tol::Float64=1e-12,
               maxiter::Int=100, v0=nothing) =
  lanczos_call(A, B, Binv, nev, which, krylovdim, tol, maxiter, v0)

# ---------------------------------------------------------------- sparse direct `M \ r` (Example07:412/416)
"""`SparseDirectPreconditioner(ctx, A)`: `M \\ r` for a sparse SPD `A::SparseMatrixCSC` — RecyclingKrylovSolvers' pcg applies
its `M` as `z .= M \\ r` (cg.jl:85, 100), and Example07:412/416 pass the interface block `A_ΓΓ` itself — by the device
sparse direct solve (`mi_spd_direct_create`: one level of nested dissection, dense inverses of small pieces)."""
function SparseDirectPreconditioner(ctx::MiContext, A::SparseMatrixCSC{Float64,Int})
  r = Ref{Ptr{Cvoid}}(C_NULL)
  cp, rv = Vector{Int64}(A.colptr), Vector{Int64}(A.rowval)
  check(ccall((:mi_spd_direct_create, lib), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
              ctx.h, A.n, cp, rv, A.nzval, 1, r))
  wrap(ctx, r)
end
"""`set_values!(M, A)`: the values of `A` (same pattern as at creation) — a new realization's A_ΓΓ (Example07:416)."""
set_values!(M::MiOperator, A::SparseMatrixCSC{Float64,Int}) =
  check(ccall((:mi_spd_direct_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.h, A.nzval))
function spd_direct_stats(M::MiOperator)
  p, s = Ref{Int64}(0), Ref{Int64}(0)
  check(ccall((:mi_spd_direct_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), M.h, p, s))
  (p[], s[])
end

# ---------------------------------------------------------------- block-Jacobi on the full matrix (Example09 `bj$(nbj)_0`)
"""`MyPreconditioners.BJPreconditioner(ctx, nb, A)`: a device method ADDED to the reference's constructor
(MyPreconditioners/BJPreconditioner.jl:16-21; `mi_block_jacobi_create`): `nb` contiguous slices of `A`, `bsize = n ÷ nb`, the
last one to the end, each solved exactly. A script that writes `using MyPreconditioners: BJPreconditioner` calls
`BJPreconditioner(ctx, nbj, A)` where it called `BJPreconditioner(nbj, A)`; the two-argument method keeps resolving, and the
shim exports no name of its own for it. `M \\ r` and `ldiv!` work as for every operator; `bj_set_values!(M, A)` takes a new
realization on the same pattern (Example06:600)."""
function MyPreconditioners.BJPreconditioner(ctx::MiContext, nb::Int, A::SparseMatrixCSC{Float64,Int})
  r = Ref{Ptr{Cvoid}}(C_NULL)
  cp, rv = Vector{Int64}(A.colptr), Vector{Int64}(A.rowval)
  check(ccall((:mi_block_jacobi_create, lib), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Cint, Ref{Ptr{Cvoid}}),
              ctx.h, A.n, cp, rv, A.nzval, nb, C_NULL, C_NULL, 1, r))
  wrap(ctx, r)
end
bj_set_values!(M::MiOperator, A::SparseMatrixCSC{Float64,Int}) =
  check(ccall((:mi_block_jacobi_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.h, A.nzval))

# `pcg(S, b_schur, zeros(S.N), A_ΓΓ)` as Example07:412/416 write it: the device factor is cached per matrix object, refilled
# (set_values!) when its values changed since the last call and rebuilt when its pattern or the context did.
const spd_factors = WeakKeyDict{SparseMatrixCSC{Float64,Int},Any}()
function spd_factor(ctx::MiContext, M::SparseMatrixCSC{Float64,Int})
  c = get(spd_factors, M, nothing)
  if c === nothing || c.op.ctx !== ctx || c.colptr != M.colptr || c.rowval != M.rowval
    c = (op=SparseDirectPreconditioner(ctx, M), colptr=copy(M.colptr), rowval=copy(M.rowval), nzval=copy(M.nzval))
    spd_factors[M] = c
  elseif c.nzval != M.nzval
    set_values!(c.op, M)
    copyto!(c.nzval, M.nzval)
  end
  c.op
end
pcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::SparseMatrixCSC{Float64,Int}; maxit=0) =
  solve(:pcg, A, spd_factor(A.ctx, M), b, x, nothing, maxit)

# ---------------------------------------------------------------- LORASC (Example03:245-268)
"""`MiLorasc`: the device form of Fem's `LorascPreconditioner` (EPDD.jl:1406-1428). `op` applies `apply_lorasc`
(EPDD.jl:1908-1976) on the device; `plan` (the exact `A_IId \\ f` by level solves, in place of `chol_A_IId`) and `A_ΓΓ`
(the sparse direct factor, in place of `chol_A_ΓΓ`) are borrowed by `op` and therefore kept in fields: the library
refuses to destroy them while `op` lives."""
mutable struct MiLorasc
  op::MiOperator
  plan::SchurSetup
  A_ΓΓ::MiOperator
  n_Γ::Int
end

function lorasc_maps(ind_Id_g2l::Vector{Dict{Int,Int}}, ind_Γ_g2l::Dict{Int,Int}, not_dirichlet_inds_g2l::Dict{Int,Int})
  pI = [Vector{Int64}(undef, length(m)) for m in ind_Id_g2l]
  for (d, m) in enumerate(ind_Id_g2l), (node, i) in m
    pI[d][i] = not_dirichlet_inds_g2l[node]                  # EPDD.jl:1924
  end
  pΓ = Vector{Int64}(undef, length(ind_Γ_g2l))
  for (node, g) in ind_Γ_g2l
    pΓ[g] = not_dirichlet_inds_g2l[node]                     # EPDD.jl:1930
  end
  pI, pΓ
end

"""`LorascPreconditioner(ctx, A_IΓd, ind_Id_g2l, ind_Γ_g2l, not_dirichlet_inds_g2l, plan, A_ΓΓ_solver[, E, coef])`: a method
added to the constructor of Fem's struct. `plan` is a `SchurSetup` of the same subdomains after `keep_levels!` and an
`assemble_local_schurs(plan, …)`; `A_ΓΓ_solver = SparseDirectPreconditioner(ctx, A_ΓΓ)`; `E` the vectors of the low-rank
correction as columns. `coef === nothing` applies them as the reference does — its loop never uses the Σ it stores
(EPDD.jl:1954-1957, 1596); `coef = Σ` is the correction of the paper."""
function LorascPreconditioner(ctx::MiContext, A_IΓd::Vector{SparseMatrixCSC{Float64,Int}}, ind_Id_g2l::Vector{Dict{Int,Int}},
                              ind_Γ_g2l::Dict{Int,Int}, not_dirichlet_inds_g2l::Dict{Int,Int}, plan::SchurSetup,
                              A_ΓΓ_solver::MiOperator, E::Matrix{Float64}=Matrix{Float64}(undef, length(ind_Γ_g2l), 0), coef=nothing)
  ndom = length(A_IΓd); n_Γ = length(ind_Γ_g2l)
  pI, pΓ = lorasc_maps(ind_Id_g2l, ind_Γ_g2l, not_dirichlet_inds_g2l)
  ni = Int64[length(p) for p in pI]
  igp, igi, igv = csc_parts(A_IΓd)
  cf = coef === nothing ? C_NULL : Vector{Float64}(coef)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve pI igp igi igv begin
    check(ccall((:mi_lorasc_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}},
                 Ptr{Ptr{Float64}}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, sum(ni) + n_Γ, n_Γ, ni, ptrs(pI), pΓ, ptrs(igp), ptrs(igi), ptrs(igv), plan.h, A_ΓΓ_solver.h,
                size(E, 2), E, cf, 1, r))
  end
  MiLorasc(wrap(ctx, r), plan, A_ΓΓ_solver, n_Γ)
end

"""`prepare_lorasc_precond(ctx, S, A_IId, A_IΓd, A_ΓΓ, ind_Id_g2l, ind_Γ_g2l, not_dirichlet_inds_g2l, A_IIdd, A_IΓdd, A_ΓΓdd;
nvec, ε)`: Example03:246-252 with the factorizations on the device. The eigenpairs come from the reference's own host
method with `compute_A_ΓΓ_chol`'s work skipped where it can be (its `E`, `Σ` fields are taken over as they are); the local
blocks of `prepare_local_schurs` are needed for the level elimination that stands in for `cholesky(A_IId[idom])`."""
function prepare_lorasc_precond(ctx::MiContext, S, A_IId, A_IΓd, A_ΓΓ::SparseMatrixCSC{Float64,Int}, ind_Id_g2l, ind_Γ_g2l,
                                not_dirichlet_inds_g2l, A_IIdd, A_IΓdd, A_ΓΓdd; nvec=25, ε=.01, verbose=true)
  Π = prepare_lorasc_precond(S, A_IId, A_IΓd, A_ΓΓ, ind_Id_g2l, ind_Γ_g2l, not_dirichlet_inds_g2l; nvec=nvec, ε=ε, verbose=verbose)
  plan = SchurSetup(ctx, A_IIdd, A_IΓdd, A_ΓΓdd)
  keep_levels!(plan)
  assemble_local_schurs(plan, A_IIdd, A_IΓdd, A_ΓΓdd)
  E = isempty(Π.Σ) ? Matrix{Float64}(undef, A_ΓΓ.n, 0) : reduce(hcat, Π.E[1:length(Π.Σ)])
  LorascPreconditioner(ctx, A_IΓd, ind_Id_g2l, ind_Γ_g2l, not_dirichlet_inds_g2l, plan, SparseDirectPreconditioner(ctx, A_ΓΓ), E)
end

apply_lorasc(Π::MiLorasc, x::Vector{Float64}) = Π.op * x                                 # EPDD.jl:1908-1976
\(Π::MiLorasc, x::Vector{Float64}) = apply_lorasc(Π, x)                                  # EPDD.jl:1980-1982
ldiv!(z::Vector{Float64}, Π::MiLorasc, r::Vector{Float64}) = mul!(z, Π.op, r)            # EPDD.jl:1984-1988
ldiv!(Π::MiLorasc, r::Vector{Float64}) = (r .= apply_lorasc(Π, copy(r)))                 # EPDD.jl:1990-1993
"""New values of all A_IΓd (same patterns) for a new realization; the interior and A_ΓΓ factors move with
`assemble_local_schurs(Π.plan, …)` and `set_values!(Π.A_ΓΓ, A_ΓΓ)`."""
set_values!(Π::MiLorasc, A_IΓd::Vector{SparseMatrixCSC{Float64,Int}}) =
  check(ccall((:mi_lorasc_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), Π.op.h, reduce(vcat, [A.nzval for A in A_IΓd])))
"""A new low-rank correction: the columns of `E`, applied with `coef` (`nothing`: ones, the reference as written)."""
set_correction!(Π::MiLorasc, E::Matrix{Float64}, coef=nothing) =
  check(ccall((:mi_lorasc_set_correction, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}),
              Π.op.h, size(E, 2), E, coef === nothing ? C_NULL : Vector{Float64}(coef)))
pcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiLorasc; maxit=0) = solve(:pcg, A, M.op, b, x, nothing, maxit)   # Example03:255
defpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, M::MiLorasc; maxit=0) =
  solve(:defpcg, A, M.op, b, x, W, maxit)                                                                                        # Example03:262, 268


# ---------------------------------------------------------------- Neumann-Neumann induced (Example03:300-319)
# Fem exports `NeumannNeumannInducedPreconditioner`, `prepare_neumann_neumann_induced_precond` and
# `apply_neumann_neumann_induced` (Fem.jl:84-86): the methods below are added to Fem's own functions by their qualified
# names, so nothing of the reference is shadowed.
const MI_NNI_AS_WRITTEN = Cint(0)
const MI_NNI_ASSEMBLED = Cint(1)
nni_coupling(c::Symbol) = c == :reference ? MI_NNI_AS_WRITTEN : c == :assembled ? MI_NNI_ASSEMBLED :
  throw(ArgumentError("coupling must be :reference or :assembled, not $c"))

"""`MiNNInduced`: the device form of Fem's `NeumannNeumannInducedPreconditioner` (EPDD.jl:2274-2285). `op` applies
`apply_neumann_neumann_induced` (EPDD.jl:2363-2423) on the device; `plan` (the exact `A_IIdd \\ f` by level solves, in
place of `chol_A_IId`) is borrowed by `op` and therefore kept in a field: the library refuses to destroy it while `op`
lives."""
mutable struct MiNNInduced
  op::MiOperator
  plan::SchurSetup
  n_Γ::Int
end

"""`Fem.NeumannNeumannInducedPreconditioner(ctx, ΠSd, A_IΓdd, ind_Id_g2l, ind_Γ_g2l, ind_Γd_Γ2l, node_Γ_cnt,
not_dirichlet_inds_g2l, plan; storage, coupling)`: a method added to the constructor of Fem's struct. `plan` is a
`SchurSetup` of the same subdomains after `keep_levels!` and an `assemble_local_schurs(plan, …)`. `coupling = :reference`
is EPDD.jl:2411 as written — the interior coupled to the local, unweighted, unassembled `z_Γd`: neither symmetric nor
positive definite, the reference's "only seems to work with deflation" (EPDD.jl:2302); `:assembled` couples it to
`z_Γ[gather_d]`, the symmetric positive definite form. `storage = Float32` holds the ΠS_d as fp32 on the device."""
function Fem.NeumannNeumannInducedPreconditioner(ctx::MiContext, ΠSd::Vector{Matrix{Float64}}, A_IΓdd::Vector{SparseMatrixCSC{Float64,Int}},
                                                 ind_Id_g2l::Vector{Dict{Int,Int}}, ind_Γ_g2l::Dict{Int,Int},
                                                 ind_Γd_Γ2l::Vector{Dict{Int,Int}}, node_Γ_cnt::Vector{Int},
                                                 not_dirichlet_inds_g2l::Dict{Int,Int}, plan::SchurSetup;
                                                 storage::Type=Float64, coupling::Symbol=:reference)
  ndom = length(A_IΓdd); n_Γ = length(ind_Γ_g2l)
  pI, pΓ = lorasc_maps(ind_Id_g2l, ind_Γ_g2l, not_dirichlet_inds_g2l)                     # EPDD.jl:2383-2391
  ni = Int64[length(p) for p in pI]
  g = flatten_maps(ind_Γd_Γ2l); nd = Int64[length(x) for x in g]
  cnt = Vector{Int64}(node_Γ_cnt)
  igp, igi, igv = csc_parts(A_IΓdd)
  storage === Float64 || storage === Float32 || error("storage must be Float64 or Float32")
  sto = storage === Float32 ? Cint(1) : Cint(0)   # MI_STORE_F32 / MI_STORE_F64
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve pI g igp igi igv ΠSd begin
    check(ccall((:mi_nn_induced_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Int64},
                 Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cint, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, ndom, sum(ni) + n_Γ, n_Γ, nd, ni, ptrs(pI), pΓ, ptrs(g), cnt, ptrs(igp), ptrs(igi), ptrs(igv), Ptr{Float64}[pointer(B) for B in ΠSd],
                sto, plan.h, nni_coupling(coupling), 1, r))
  end
  MiNNInduced(wrap(ctx, r), plan, n_Γ)
end

"""`Fem.prepare_neumann_neumann_induced_precond(ctx, A_IIdd, A_IΓdd, A_ΓΓdd, ind_Id_g2l, ind_Γ_g2l, ind_Γd_Γ2l, node_Γ_cnt,
node_Γ, not_dirichlet_inds_g2l; storage, coupling)`: Example03:299-308 (EPDD.jl:2305-2353) on the device. The dense S_d come
from the exact level elimination of a set-up plan (in place of `Array(Sd)` through the interior CG at reltol 1e-12,
:2322-2338), ΠS_d = pinv(S_d, rtol = sqrt(eps)) from `mi_nn_pinv` (:2339), and the plan's kept levels stand in for
`cholesky(A_IIdd[idom])` (:2340)."""
function Fem.prepare_neumann_neumann_induced_precond(ctx::MiContext, A_IIdd::Vector{SparseMatrixCSC{Float64,Int}},
                                                     A_IΓdd::Vector{SparseMatrixCSC{Float64,Int}}, A_ΓΓdd::Vector{SparseMatrixCSC{Float64,Int}},
                                                     ind_Id_g2l, ind_Γ_g2l, ind_Γd_Γ2l, node_Γ_cnt, node_Γ, not_dirichlet_inds_g2l;
                                                     storage::Type=Float64, coupling::Symbol=:reference)
  plan = SchurSetup(ctx, A_IIdd, A_IΓdd, A_ΓΓdd)
  keep_levels!(plan)
  Sd = assemble_local_schurs(plan, A_IIdd, A_IΓdd, A_ΓΓdd)
  nd = Int64[size(S, 1) for S in Sd]
  cat = reduce(vcat, [vec(S) for S in Sd]); out = similar(cat)
  check(ccall((:mi_nn_pinv, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Float64, Ptr{Float64}), ctx.h, length(Sd), nd, cat, 0.0, out))
  ends = cumsum(nd .^ 2)
  ΠSd = [reshape(out[(e - n * n + 1):e], n, n) for (e, n) in zip(ends, nd)]
  Fem.NeumannNeumannInducedPreconditioner(ctx, ΠSd, A_IΓdd, ind_Id_g2l, ind_Γ_g2l, ind_Γd_Γ2l, Vector{Int}(node_Γ_cnt),
                                          not_dirichlet_inds_g2l, plan; storage=storage, coupling=coupling)
end

Fem.apply_neumann_neumann_induced(Π::MiNNInduced, r::Vector{Float64}) = Π.op * r                    # EPDD.jl:2363-2423
\(Π::MiNNInduced, x::Vector{Float64}) = Fem.apply_neumann_neumann_induced(Π, x)                    # EPDD.jl:2427-2429
ldiv!(z::Vector{Float64}, Π::MiNNInduced, r::Vector{Float64}) = mul!(z, Π.op, r)                   # EPDD.jl:2431-2435
ldiv!(Π::MiNNInduced, r::Vector{Float64}) = (r .= Fem.apply_neumann_neumann_induced(Π, copy(r)))   # EPDD.jl:2437-2440
"""New values of all A_IΓdd (same patterns) for a new realization; the interior factors move with
`assemble_local_schurs(Π.plan, …)`, the blocks with `set_blocks!(Π, ΠSd)`."""
set_values!(Π::MiNNInduced, A_IΓdd::Vector{SparseMatrixCSC{Float64,Int}}) =
  check(ccall((:mi_nn_induced_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), Π.op.h, reduce(vcat, [A.nzval for A in A_IΓdd])))
set_blocks!(Π::MiNNInduced, ΠSd::Vector{Matrix{Float64}}) =
  check(ccall((:mi_nn_induced_set_blocks, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), Π.op.h, reduce(vcat, [vec(B) for B in ΠSd])))
"""`:reference` (EPDD.jl:2411 as written) or `:assembled`."""
set_coupling!(Π::MiNNInduced, coupling::Symbol) =
  check(ccall((:mi_nn_induced_set_coupling, lib), Cint, (Ptr{Cvoid}, Cint), Π.op.h, nni_coupling(coupling)))
pcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiNNInduced; maxit=0) = solve(:pcg, A, M.op, b, x, nothing, maxit)   # Example03:317
defpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, M::MiNNInduced; maxit=0) =
  solve(:defpcg, A, M.op, b, x, W, maxit)                                                                                          # Example03:313

# ---------------------------------------------------------------- smoothed-aggregation AMG (Example01:49-61)
"""`MiAMGPreconditioner`: the device form of `Preconditioners.AMGPreconditioner{SmoothedAggregation}(A)`, the `Π_amg` of
`pcg(A, b, zeros(n), Π_amg)` in Example01:49-61 (`mi_amg_create`). `Π \\ r` is one V(1,1) cycle; the smoother is Jacobi damped
by ω_l = 4 / (3 g_l), g_l = max_i Σ_j |a_ij| / a_ii, where the reference sweeps symmetric Gauss-Seidel.

`MiAMGPreconditioner(ctx, A_l, P_l, omega_over_d, coarse_inv)`: the hierarchy as arrays — the symmetric level matrices
(`length(A_l)` levels), the prolongators `P_l[l]` (n_l × n_{l+1}), ω_l ./ diag(A_l) per smoothed level and the dense
symmetric inverse of the last level. `MiAMGPreconditioner(ctx, ml)`: the same from a multilevel object with `ml.levels[l].A`,
`ml.levels[l].P` and `ml.final_A`, as `AlgebraicMultigrid.smoothed_aggregation(A)` returns it."""
mutable struct MiAMGPreconditioner
  op::MiOperator
  n_levels::Int
end

function MiAMGPreconditioner(ctx::MiContext, A_l::Vector{SparseMatrixCSC{Float64,Int}}, P_l::Vector{SparseMatrixCSC{Float64,Int}},
                             omega_over_d::Vector{Vector{Float64}}, coarse_inv::Matrix{Float64})
  L = length(A_l)
  (length(P_l) == L - 1 && length(omega_over_d) == L - 1) || throw(ArgumentError("$L levels need $(L - 1) prolongators and ω ./ d vectors"))
  n_l = Int64[A.n for A in A_l]
  ap, ai, av = csc_parts(A_l)                                           # symmetric: the CSC arrays are the CSR arrays
  pp, px, pv = csc_parts(SparseMatrixCSC{Float64,Int}[SparseMatrixCSC(copy(transpose(P))) for P in P_l])   # CSC of P' = CSR of P
  wd = reduce(vcat, omega_over_d; init=Float64[])
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve ap ai av pp px pv begin
    check(ccall((:mi_amg_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}},
                 Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, L, n_l, ptrs(ap), ptrs(ai), ptrs(av), ptrs(pp), ptrs(px), ptrs(pv), wd, coarse_inv, 1, r))
  end
  MiAMGPreconditioner(wrap(ctx, r), L)
end

function MiAMGPreconditioner(ctx::MiContext, ml)
  A_l = SparseMatrixCSC{Float64,Int}[SparseMatrixCSC{Float64,Int}(lev.A) for lev in ml.levels]
  push!(A_l, SparseMatrixCSC{Float64,Int}(ml.final_A))
  P_l = SparseMatrixCSC{Float64,Int}[SparseMatrixCSC{Float64,Int}(lev.P) for lev in ml.levels]
  wd = Vector{Float64}[]
  for A in A_l[1:end-1]
    d = Vector{Float64}(diag(A))
    g = maximum(vec(sum(abs, A; dims=2)) ./ d)
    push!(wd, (4 / (3g)) ./ d)
  end
  Ac = Matrix(A_l[end])
  Z = inv((Ac + Ac') / 2)
  MiAMGPreconditioner(ctx, A_l, P_l, wd, (Z + Z') / 2)
end

"""`MiAMGPreconditioner(ctx, A, agg; device_setup=true)`: the hierarchy's NUMBERS made on the device (`mi_amg_plan_create`) from
the matrix and frozen aggregates — `agg[l][i]` ∈ 1:n_{l+1}, the aggregate of node i of level l, one vector per smoothed level
(any standard aggregation of the first realization; the aggregation sees values only through `!= 0`, so it is the same for
every realization on one mesh). `set_values!(Π, A)` then redoes them for a new realization on the same pattern — the
per-realization `Π_amg_t = AMGPreconditioner{SmoothedAggregation}(A)` of Example06:182 without a host set-up. A symmetric
`A` with sorted columns is its own CSR form."""
function MiAMGPreconditioner(ctx::MiContext, A::SparseMatrixCSC{Float64,Int}, agg::Vector{Vector{Int}}; device_setup::Bool=true)
  device_setup || throw(ArgumentError("without device_setup pass the hierarchy itself: MiAMGPreconditioner(ctx, A_l, P_l, omega_over_d, coarse_inv)"))
  L = length(agg) + 1
  n_l = Int64[A.n; [maximum(a) for a in agg]]
  cp, rv = Vector{Int64}(A.colptr), Vector{Int64}(A.rowval)
  ag = Vector{Int64}[Vector{Int64}(a) for a in agg]
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve ag begin
    check(ccall((:mi_amg_plan_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, A.n, cp, rv, A.nzval, L, n_l, ptrs(ag), 1, r))
  end
  MiAMGPreconditioner(wrap(ctx, r), L)
end
"""`set_values!(Π, A)`: the values of `A` (same pattern as at creation) — a new realization (`mi_amg_set_values`); needs
the `device_setup` constructor. A matrix that is not positive definite throws and leaves the previous hierarchy in place."""
set_values!(Π::MiAMGPreconditioner, A::SparseMatrixCSC{Float64,Int}) =
  check(ccall((:mi_amg_set_values, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), Π.op.h, A.nzval))

function amg_stats(Π::MiAMGPreconditioner)
  a, b, c, d = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
  check(ccall((:mi_amg_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), Π.op.h, a, b, c, d))
  (n_levels=Int(a[]), coarse_n=Int(b[]), operator_nnz=Int(c[]), bytes_kept=Int(d[]))
end

\(Π::MiAMGPreconditioner, r::Vector{Float64}) = Π.op * r
ldiv!(z::Vector{Float64}, Π::MiAMGPreconditioner, r::Vector{Float64}) = mul!(z, Π.op, r)
ldiv!(Π::MiAMGPreconditioner, r::Vector{Float64}) = (r .= Π.op * copy(r))
pcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGPreconditioner; maxit=0) = solve(:pcg, A, M.op, b, x, nothing, maxit)   # Example01:58
defpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, M::MiAMGPreconditioner; maxit=0) =
  solve(:defpcg, A, M.op, b, x, W, maxit)
eigpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGPreconditioner, nvec::Int, spdim::Int; maxit=0) =
  eigsolve(:eigpcg, A, M.op, b, x, nothing, nvec, spdim, maxit)
eigdefpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGPreconditioner, W::Matrix{Float64}, spdim::Int; maxit=0) =
  eigsolve(:eigdefpcg, A, M.op, b, x, W, size(W, 2), spdim, maxit)
initpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGPreconditioner, W::Matrix{Float64}; maxit=0) = initsolve(A, M.op, b, x, W, maxit)

# ---------------------------------------------------------------- P hierarchies on one plan (Example12_…_Functions.jl:85-113)
"""`MiAMGBank(ctx, A, agg, capacity)`: `capacity` smoothed-aggregation hierarchies on the pattern of `A` and the frozen
aggregates `agg` (as for `MiAMGPreconditioner(ctx, A, agg)`), sharing one plan, one set of index arrays and one set-up engine
on the device (`mi_amg_bank_create`) — the constant preconditioners of `get_centroidal_preconds`, one member per centroid, a
member being numbers only. `set_values!(bank, p, A_p)` makes member `p` (1-based, as everything on the Julia side). The bank
is not an operator: `MiAMGBankView(bank, max_terms)` is, `select!(Π, p)` is the `Πs[find_precond(ξ, hXt)]` of Example12:106
and `combine!(Π, members, coefficients)` the `InterpolatingPreconditioner` of Example14 — both rewrite small device arrays,
so the solve graphs captured with the view serve every selection. A view roots its bank; the bank's slab is freed at the
first collection after its last view is gone."""
mutable struct MiAMGBank
  op::MiOperator
  capacity::Int
  n_levels::Int
end
function MiAMGBank(ctx::MiContext, A::SparseMatrixCSC{Float64,Int}, agg::Vector{Vector{Int}}, capacity::Int)
  capacity >= 1 || throw(ArgumentError("capacity = $capacity: a bank holds at least 1 member"))
  L = length(agg) + 1
  n_l = Int64[A.n; [maximum(a) for a in agg]]
  cp, rv = Vector{Int64}(A.colptr), Vector{Int64}(A.rowval)
  ag = Vector{Int64}[Vector{Int64}(a) for a in agg]
  r = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve ag begin
    check(ccall((:mi_amg_bank_create, lib), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Int64}}, Int64, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, A.n, cp, rv, L, n_l, ptrs(ag), capacity, 1, r))
  end
  n = Ref{Int64}(0)
  check(ccall((:mi_op_size, lib), Cint, (Ptr{Cvoid}, Ref{Int64}), r[], n))
  MiAMGBank(finalizer(bank_release, MiOperator(r[], n[], n[], ctx, nothing)), capacity, L)
end
# The library refuses to destroy a bank under a live view and leaves the handle valid. A view that becomes garbage in the
# same collection may be finalized after its bank: the bank then asks again at the next collection instead of leaking its slab.
function bank_release(o::MiOperator)
  rc = ccall((:mi_op_destroy, lib), Cint, (Ptr{Cvoid},), o.h)
  rc == 0 || finalizer(bank_release, o)
  return
end
member0(bank::MiAMGBank, p::Integer) = 1 <= p <= bank.capacity ? Int64(p - 1) : throw(BoundsError(1:bank.capacity, p))
"""`set_values!(bank, p, A)`: member `p` from the values of `A` (the pattern of creation; `mi_amg_bank_set_values`). A matrix
that is not positive definite throws and leaves the member as it was."""
set_values!(bank::MiAMGBank, p::Integer, A::SparseMatrixCSC{Float64,Int}) =
  check(ccall((:mi_amg_bank_set_values, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), bank.op.h, member0(bank, p), A.nzval))
function amg_bank_stats(bank::MiAMGBank)
  a, b, c, d, e = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
  check(ccall((:mi_amg_bank_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), bank.op.h, a, b, c, d, e))
  (capacity=Int(a[]), members_set=Int(b[]), bytes_shared=Int(c[]), bytes_per_member=Int(d[]), views=Int(e[]))
end

mutable struct MiAMGBankView
  op::MiOperator
  bank::MiAMGBank
  max_terms::Int
end
function MiAMGBankView(bank::MiAMGBank, max_terms::Int=1)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:mi_amg_bank_view, lib), Cint, (Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), bank.op.h, max_terms, r))
  MiAMGBankView(wrap(bank.op.ctx, r, bank), bank, max_terms)
end
"""`combine!(Π, members, coefficients)`: Π \\ r = Σ_i coefficients[i] (Π_{members[i]} \\ r), 1-based members that were set before
(`mi_amg_bank_select`)."""
function combine!(Π::MiAMGBankView, members::Vector{Int}, coefficients::Vector{Float64})
  length(members) == length(coefficients) || throw(ArgumentError("$(length(coefficients)) coefficients for $(length(members)) members"))
  m0 = Int64[member0(Π.bank, p) for p in members]
  check(ccall((:mi_amg_bank_select, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}), Π.op.h, length(m0), m0, coefficients))
end
"""`select!(Π, p)`: member `p` alone, coefficient 1."""
select!(Π::MiAMGBankView, p::Integer) = combine!(Π, Int[p], [1.0])

\(Π::MiAMGBankView, r::Vector{Float64}) = Π.op * r
ldiv!(z::Vector{Float64}, Π::MiAMGBankView, r::Vector{Float64}) = mul!(z, Π.op, r)
ldiv!(Π::MiAMGBankView, r::Vector{Float64}) = (r .= Π.op * copy(r))
pcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGBankView; maxit=0) = solve(:pcg, A, M.op, b, x, nothing, maxit)   # Example12:106
defpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, W::Matrix{Float64}, M::MiAMGBankView; maxit=0) =
  solve(:defpcg, A, M.op, b, x, W, maxit)
eigpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGBankView, nvec::Int, spdim::Int; maxit=0) =
  eigsolve(:eigpcg, A, M.op, b, x, nothing, nvec, spdim, maxit)
eigdefpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGBankView, W::Matrix{Float64}, spdim::Int; maxit=0) =
  eigsolve(:eigdefpcg, A, M.op, b, x, W, size(W, 2), spdim, maxit)
initpcg(A::MiOperator, b::Vector{Float64}, x::Vector{Float64}, M::MiAMGBankView, W::Matrix{Float64}; maxit=0) = initsolve(A, M.op, b, x, W, maxit)

# ---------------------------------------------------------------- k realizations in one Krylov loop (Examples 06, 12, 14, 19, 20: `for ireal in 1:nreals`)
"""`MiCsrBatch(ctx, A, capacity)`: `capacity` sparse matrices on the pattern of `A`, sharing one set of index arrays and row
blocks on the device (`mi_csr_batch_create`) — the systems `A_t` of a Monte-Carlo loop over realizations, a slot being numbers
only. `set_values!(batch, s, A_s)` fills slot `s` (1-based, as everything on the Julia side). The batch is not an operator:
`pcg_batch(batch, slots, B, X, Π, members)` solves `length(slots)` of its slots in one Krylov loop on the device, system `t`
under member `members[t]` of the bank view `Π`, and returns `(X, its, res_norms)`: column `t` of `X`, `its[t]` and
`res_norms[t]` are those of `pcg(A_t, B[:, t], X[:, t], Π)` after `select!(Π, members[t])`."""
mutable struct MiCsrBatch
  op::MiOperator
  capacity::Int
  nnz::Int
end
function MiCsrBatch(ctx::MiContext, A::SparseMatrixCSC{Float64,Int}, capacity::Int)
  capacity >= 1 || throw(ArgumentError("capacity = $capacity: a batch holds at least 1 slot"))
  cp, rv = Vector{Int64}(A.colptr), Vector{Int64}(A.rowval)
  r = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:mi_csr_batch_create, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Cint, Ref{Ptr{Cvoid}}),
              ctx.h, A.n, cp, rv, capacity, 1, r))
  MiCsrBatch(wrap(ctx, r), capacity, length(A.nzval))
end
slot0(batch::MiCsrBatch, s::Integer) = 1 <= s <= batch.capacity ? Int64(s - 1) : throw(BoundsError(1:batch.capacity, s))
function set_values!(batch::MiCsrBatch, s::Integer, A::SparseMatrixCSC{Float64,Int})
  length(A.nzval) == batch.nnz || throw(ArgumentError("$(length(A.nzval)) values for the $(batch.nnz) stored entries of the batch's pattern"))
  check(ccall((:mi_csr_batch_set_values, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), batch.op.h, slot0(batch, s), A.nzval))
end
function csr_batch_stats(batch::MiCsrBatch)
  a, b, c, d = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
  check(ccall((:mi_csr_batch_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), batch.op.h, a, b, c, d))
  (capacity=Int(a[]), slots_set=Int(b[]), bytes_shared=Int(c[]), bytes_per_slot=Int(d[]))
end
function pcg_batch(A::MiCsrBatch, slots::Vector{Int}, B::Matrix{Float64}, X::Matrix{Float64}, M::MiAMGBankView, members::Vector{Int}; maxit=0)
  n, k = A.op.n, length(slots)
  length(members) == k || throw(ArgumentError("$(length(members)) members for $k slots"))
  size(B) == (n, k) && size(X) == (n, k) || throw(DimensionMismatch("B and X must be $n x $k"))
  s0 = Int64[slot0(A, s) for s in slots]
  m0 = Int64[member0(M.bank, p) for p in members]
  res = Matrix{Float64}(undef, n, k)                   # cg.jl:23 `res_norm = Array{T,1}(undef, n)`, one column per system
  its = zeros(Int64, k)
  check(ccall((:mi_pcg_batch, lib), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Float64, Ptr{Float64}, Int64, Ptr{Int64}),
              A.op.h, k, s0, M.op.h, m0, B, n, X, n, maxit, 1e-7, res, n, its))
  return X, Vector{Int}(its), [res[1:its[t], t] for t in 1:k]
end
"""`set_values!(bank, members, batch, slots)`: the hierarchies of `length(members)` (at most 16) bank members in one sequence of
launches (`mi_amg_bank_set_values_batch`), member `members[t]` from the values in slot `slots[t]` of the batch, read on the
device where they lie; 1-based members and slots. A member carries the bits of `set_values!(bank, members[t], A_t)`. Returns
the per-term success; a term that fails leaves its member as it was, the healthy terms are committed, and with `strict` (the
default) the call then throws as `set_values!(bank, p, A)` does."""
function set_values!(bank::MiAMGBank, members::Vector{Int}, batch::MiCsrBatch, slots::Vector{Int}; strict::Bool=true)
  k = length(members)
  length(slots) == k || throw(ArgumentError("$(length(slots)) slots for $k members"))
  m0 = Int64[member0(bank, p) for p in members]
  s0 = Int64[slot0(batch, s) for s in slots]
  status = zeros(Cint, k)
  check(ccall((:mi_amg_bank_set_values_batch, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cint}),
              bank.op.h, k, m0, batch.op.h, s0, status))
  ok = status .== 0
  strict && !all(ok) && check(MI_ERR_SINGULAR)         # the library's message names the failed terms
  return ok
end

# ---------------------------------------------------------------- realization sampler (Example06:160, Example09 `draw!(sampler)`)
"""`MiKlField`: the step from a latent vector ξ to the field g = Σ_α sqrt(Λ_α) ξ_α Ψ[:, α] on the device (`mi_kl_field_t`).
`MiKlField(ctx, Λ, Ψ)` keeps Ψ; `MiKlField(ctx, nnode, Λ, Φ, Φd, inds_l2gd)` keeps the factors of
`draw(mesh, Λ, Φ, Φd, inds_l2gd)` (KLDD.jl:850-883) and never forms Ψ. The methods below are ADDED to Fem's `set!`, `draw!` and
`get_kl_coordinates` (exports at Fem/Fem.jl:101-104); they take the handle first, so they cannot collide with the reference's
`(Λ, Ψ, ξ, g)` methods. The calls of this section are written with `@ccall`, argument and C type side by side;
tests/test_julia_shim_klfield_cpu.py checks them against include/mi355schur.h."""
mutable struct MiKlField
  h::Ptr{Cvoid}; n::Int; m::Int; ctx::MiContext
end
function klfield_wrap(ctx::MiContext, r::Ref{Ptr{Cvoid}}, n::Int, m::Int)
  f = MiKlField(r[], n, m, ctx)
  finalizer(q -> @ccall(lib.mi_kl_field_destroy(q.h::Ptr{Cvoid})::Cint), f)
end
function MiKlField(ctx::MiContext, Λ::Vector{Float64}, Ψ::Matrix{Float64})
  n, m = size(Ψ)
  length(Λ) == m || throw(ArgumentError("Ψ has $m columns, Λ $(length(Λ)) entries"))
  r = Ref{Ptr{Cvoid}}(C_NULL)
  check(@ccall lib.mi_kl_field_create(ctx.h::Ptr{Cvoid}, n::Int64, m::Int64, Λ::Ptr{Float64}, Ψ::Ptr{Float64}, n::Int64, r::Ref{Ptr{Cvoid}})::Cint)
  klfield_wrap(ctx, r, n, m)
end
function MiKlField(ctx::MiContext, nnode::Int, Λ::Vector{Float64}, Φ::Matrix{Float64}, Φd::Vector{Matrix{Float64}}, inds_l2gd::Vector{Vector{Int}})
  ndom, m = length(Φd), length(Λ)
  n_d, md = Int64[size(P, 1) for P in Φd], Int64[size(P, 2) for P in Φd]
  (length(inds_l2gd) == ndom && all(length(inds_l2gd[d]) == n_d[d] for d in 1:ndom)) || throw(ArgumentError("Φd[d] must have length(inds_l2gd[d]) rows"))
  size(Φ) == (sum(md), m) || throw(ArgumentError("Φ is $(size(Φ)), expected $((sum(md), m))"))
  inds = Vector{Int64}(reduce(vcat, inds_l2gd))
  blocks = reduce(vcat, [vec(P) for P in Φd])                          # column-major blocks, one after the other
  r = Ref{Ptr{Cvoid}}(C_NULL)
  check(@ccall lib.mi_kl_field_create_dd(ctx.h::Ptr{Cvoid}, nnode::Int64, m::Int64, Λ::Ptr{Float64}, ndom::Int64, n_d::Ptr{Int64}, md::Ptr{Int64},
                                         inds::Ptr{Int64}, 1::Cint, blocks::Ptr{Float64}, Φ::Ptr{Float64}, size(Φ, 1)::Int64, r::Ref{Ptr{Cvoid}})::Cint)
  klfield_wrap(ctx, r, nnode, m)
end

"""`set!(f, ξ, g)`: `set!(Λ, Ψ, ξ, g)` (KLDD.jl:1150-1164) on the device; g has the bits of the host loop (dense form)."""
function Fem.set!(f::MiKlField, ξ::Vector{Float64}, g::Vector{Float64})
  (length(ξ) == f.m && length(g) == f.n) || throw(DimensionMismatch("ξ needs $(f.m) entries, g $(f.n)"))
  check(@ccall lib.mi_kl_field_set(f.h::Ptr{Cvoid}, 1::Int64, ξ::Ptr{Float64}, f.m::Int64, g::Ptr{Float64}, f.n::Int64, C_NULL::Ptr{Float64}, f.n::Int64)::Cint)
  return g
end
"""`draw!(f, ξ, g)`: `draw!(Λ, Ψ, ξ, g)` (KLDD.jl:1026-1044, Example06:160): ξ .= N(0, I) on the host (m numbers), the field on
the device."""
function Fem.draw!(f::MiKlField, ξ::Vector{Float64}, g::Vector{Float64})
  ξ .= randn(f.m)
  Fem.set!(f, ξ, g)
  return
end
"""`coefficient!(a, f, ξ)`: a = exp.(g(ξ)) without the field crossing to the host (the `exp.(g)` of Example06:161)."""
function coefficient!(a::Vector{Float64}, f::MiKlField, ξ::Vector{Float64})
  (length(ξ) == f.m && length(a) == f.n) || throw(DimensionMismatch("ξ needs $(f.m) entries, a $(f.n)"))
  check(@ccall lib.mi_kl_field_set(f.h::Ptr{Cvoid}, 1::Int64, ξ::Ptr{Float64}, f.m::Int64, C_NULL::Ptr{Float64}, f.n::Int64, a::Ptr{Float64}, f.n::Int64)::Cint)
  return a
end
"""`get_kl_coordinates(f, g, M)`: `get_kl_coordinates(g, Λ, Ψ, M)` (KLDD.jl:1109-1124); `M = MiOperator(ctx, mass_matrix)`."""
function Fem.get_kl_coordinates(f::MiKlField, g::Vector{Float64}, M::MiOperator)
  ξ = Vector{Float64}(undef, f.m)
  check(@ccall lib.mi_kl_field_coords(f.h::Ptr{Cvoid}, M.h::Ptr{Cvoid}, g::Ptr{Float64}, ξ::Ptr{Float64})::Cint)
  return ξ
end
function klfield_stats(f::MiKlField)
  a, b = Ref{Int64}(0), Ref{Int64}(0)
  check(@ccall lib.mi_kl_field_stats(f.h::Ptr{Cvoid}, a::Ref{Int64}, b::Ref{Int64})::Cint)
  (bytes_kept=Int(a[]), bytes_per_set=Int(b[]))
end

"""`MiMcmcSampler(f)`: `prepare_mcmc_sampler(Λ, Ψ)` (Samplers.jl:130-152) on a `MiKlField`; `draw!(smp)` is the reference's
(Samplers.jl:165-199) with the field on the device and returns `cnt`; `smp.g`, `smp.a = exp.(smp.g)` as Example09 reads them."""
mutable struct MiMcmcSampler
  n::Int; m::Int
  σ2::Float64; ξ::Vector{Float64}
  ϑ2::Float64; χ::Vector{Float64}
  field::MiKlField
  g::Vector{Float64}; a::Vector{Float64}
end
function MiMcmcSampler(f::MiKlField)
  σ2 = 1.
  ξ = sqrt(σ2) .* randn(f.m)
  ϑ2 = 2.38^2 * σ2 / f.m
  χ = ξ .+ sqrt(ϑ2) .* randn(f.m)
  smp = MiMcmcSampler(f.n, f.m, σ2, ξ, ϑ2, χ, f, zeros(f.n), zeros(f.n))
  Fem.set!(smp, ξ)
  return smp
end
function Fem.set!(smp::MiMcmcSampler, ξ::Vector{Float64})
  smp.ξ .= ξ
  Fem.set!(smp.field, smp.ξ, smp.g)
  smp.a .= exp.(smp.g)
  return
end
function Fem.draw!(smp::MiMcmcSampler)
  sq_norm_of_ξ = smp.ξ'smp.ξ
  cnt = 0
  while true
    smp.χ .= smp.ξ .+ sqrt(smp.ϑ2) .* randn(smp.m)
    sq_norm_of_χ = smp.χ'smp.χ
    cnt += 1
    α = sq_norm_of_ξ < sq_norm_of_χ ? exp((sq_norm_of_ξ - sq_norm_of_χ) / 2 / smp.σ2) : 1.
    rand() > α || break
  end
  Fem.set!(smp, smp.χ)
  return cnt
end

end # module
