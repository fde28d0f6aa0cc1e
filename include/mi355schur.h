/* mi355schur.h — C ABI of libmi355schur: the MI355X (gfx950) Schur-complement PCG hot path.
 *
 * Drop-in boundary for the domain-decomposition hot path of venkovic/julia-phd-krylov-spdes.
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference root; "EPDD.jl" = Fem/EllipticPdeDomainDecomposition.jl). The reference is pure
 * Julia: a `ccall` shim (julia/MI355Schur.jl, shown in INTEGRATION.md) binds exactly these
 * symbols and re-exports the reference's own function names on top of them.
 *
 * Conventions
 *   - Plain C: opaque handles, pointers and sizes. No C++ / torch types cross this ABI.
 *   - Every function returns an int status: MI_OK (0) or a negative MI_ERR_* code;
 *     mi_last_error() returns a thread-local description of the last failure. No exception
 *     crosses the ABI (Julia side turns non-zero into `error(...)`; MI_ERR_SINGULAR maps to
 *     LinearAlgebra.SingularException as thrown by `WtAW \ mu`, defcg.jl:53,273).
 *   - Arithmetic is IEEE fp64 throughout; indices passed in are int64 with an explicit
 *     `index_base` (1 for Julia arrays, 0 for C/numpy); they are stored as int32 on the device.
 *   - `*_create` functions read HOST arrays and copy what they need to the device; the caller
 *     keeps ownership and may free or mutate its arrays afterwards (Julia GC owns them).
 *   - Vector arguments of apply/solve calls (`x`, `y`, `b`, `W`) are host pointers by default,
 *     or device pointers after mi_ctx_set_pointer_mode(ctx, MI_PTR_DEVICE). Scalar/history
 *     outputs (`it`, `res_norm`, dot results) are always host pointers.
 *   - A context owns one HIP stream; handles are thread-compatible, not thread-safe. In
 *     multi-GPU use there is one process (or thread) and one context per GPU and every rank
 *     enters collective calls (applies and solves on a SHARDED operator, see below) together.
 *   - There is no CPU fallback: with no gfx950 device mi_ctx_create fails with MI_ERR_NO_DEVICE.
 */
#ifndef MI355SCHUR_H
#define MI355SCHUR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_ERR_BAD_ARG (-1)      /* NULL/negative/out-of-range argument, index out of bounds          */
#define MI_ERR_HIP (-2)          /* a HIP runtime call failed                                          */
#define MI_ERR_SINGULAR (-3)     /* WtAW is singular to working precision (Julia: SingularException)   */
#define MI_ERR_RES_CAPACITY (-4) /* res_norm capacity exhausted (Julia: BoundsError on res_norm[it])   */
#define MI_ERR_COMM (-5)         /* RCCL not loadable / communicator failure                           */
#define MI_ERR_NO_DEVICE (-6)    /* no usable gfx950 device                                            */
#define MI_ERR_CALLBACK (-7)     /* the interior-solve callback reported failure                       */
#define MI_ERR_BOUNDS (-8)       /* eigCG family: an index the reference would throw BoundsError on     */

#define MI_PTR_HOST 0
#define MI_PTR_DEVICE 1

typedef struct mi_ctx_s *mi_ctx_t; /* device + stream + workspaces (+ RCCL communicator)            */
typedef struct mi_op_s *mi_op_t;   /* anything usable as `A` (A*x, mul!) or as `M` (M \ r)          */
typedef struct mi_event_s *mi_event_t;
typedef struct mi_plan_s *mi_plan_t; /* index half of prepare_local_schurs for a fixed mesh / partition          */

/* Interior solve callback: sol = A_II[idom]^{-1} rhs on HOST memory, called from the calling
 * thread only (Julia @cfunction safe). Replaces `IterativeSolvers.cg(A_IIdd, rhs; Pl, reltol)`
 * inside apply_local_schur / apply_global_schur (EPDD.jl:609-619, 648-650). Return 0 on success. */
typedef int (*mi_interior_solve_fn)(void *user, int64_t idom, int64_t n, const double *rhs, double *sol);

/* ---------------------------------------------------------------- library / context */
int mi_version(void);                 /* MAJOR*10000 + MINOR*100 + PATCH */
const char *mi_last_error(void);
int mi_device_count(int *count);
int mi_ctx_create(int device, mi_ctx_t *ctx);
int mi_ctx_destroy(mi_ctx_t ctx);
int mi_ctx_set_pointer_mode(mi_ctx_t ctx, int mode);
int mi_ctx_set_stream(mi_ctx_t ctx, void *hip_stream); /* borrow a hipStream_t; NULL = context's own */
int mi_ctx_get_stream(mi_ctx_t ctx, void **hip_stream);
int mi_ctx_synchronize(mi_ctx_t ctx);
/* Iterations per follow-up hipGraph replay between host convergence checks (default 8; the first replay of a
 * solve is sized from the previous solve with the same operators). 0 disables graphs (eager launches, host check
 * every iteration). Results do not depend on it. */
int mi_ctx_set_chunk(mi_ctx_t ctx, int iterations_per_graph);

/* ---------------------------------------------------------------- multi-GPU (RCCL over xGMI)
 * The Γ-interface sum over subdomains — the reference's (dead) `@distributed (+) for idom`,
 * Fem/EllipticPdePllDomainDecomposition.jl:10-14 — is one ncclAllReduce(sum, fp64, n_Γ).
 * Rank 0 calls mi_comm_unique_id and ships the 128 bytes to the other ranks by any means
 * (torch.distributed / MPI / Julia Distributed); every rank then calls mi_ctx_comm_init. */
#define MI_COMM_ID_BYTES 128
int mi_comm_unique_id(void *id_out);
int mi_ctx_comm_init(mi_ctx_t ctx, const void *id, int rank, int n_ranks);
int mi_ctx_comm_destroy(mi_ctx_t ctx);
/* The one-shot PEER EXCHANGE (the same `(+)` over subdomains, EllipticPdePllDomainDecomposition.jl:10-14, without a
 * collective library in the loop): every rank owns an arena of peer-visible device memory; after a sharded launch a rank
 * WRITES its entries of the contribution table into every rank's arena (xGMI peer stores), releases them, stores its
 * exchange number into one flag per arena and continues when its own flags have all arrived (bounded wait: an expired
 * wait makes the solve return MI_ERR_COMM, never hang). No arithmetic on the way: the tables of the ranks are disjoint,
 * so the bits are the single-GPU loop's. Everything is kernels on the context's stream — captured into the iteration
 * graphs. Call order, on every rank: mi_ctx_peer_init; mi_ctx_peer_export and ship the MI_PEER_HANDLE_BYTES to the other
 * ranks by any means (torch.distributed / MPI / Julia Distributed); mi_ctx_peer_import for every other rank (ranks that
 * are contexts of the SAME process pass the exporter's `base` instead of a handle); mi_ctx_peer_ready. With RCCL also
 * attached the peer exchange carries the tables of the folded PCG launches and RCCL the generic all-reduces; alone it
 * carries both. mi_ctx_set_exchange(ctx, 0) switches it off again (RCCL for everything), 1 on. Sharded operators must be
 * created in the same order with the same sizes on every rank (their tables sit at equal offsets of every arena).
 * Who produces and who waits: the folded PCG launches store their results into every arena themselves (write-through
 * stores; the last tile of a launch stores the flags) and a one-wave kernel behind the launch waits — mode 1, safe when
 * several ranks share a GPU (in-process ranks, tests). Mode 2 (mi_ctx_set_exchange(ctx, 2), fine-grained arena only —
 * otherwise it is mode 1): no kernel in between, the NEXT launch polls the flags with its first matrix loads already in
 * flight. A waiting launch keeps its compute units, so mode 2 is for one GPU per rank; bench.py selects it then. */
#define MI_PEER_HANDLE_BYTES 64
int mi_ctx_peer_init(mi_ctx_t ctx, int rank, int n_ranks, int64_t arena_bytes /* 0: 64 MiB */);
int mi_ctx_peer_export(mi_ctx_t ctx, void *handle_out /* MI_PEER_HANDLE_BYTES */, void **base_out);
int mi_ctx_peer_import(mi_ctx_t ctx, int rank, const void *handle, void *same_process_base);
int mi_ctx_peer_ready(mi_ctx_t ctx);
int mi_ctx_set_exchange(mi_ctx_t ctx, int use_peer_exchange);
/* Introspection for tests and benchmarks: which path ran. NO_GRAPH: 1 when this context launches eagerly (a collective
 * that cannot be captured); PEER_EXCHANGE: 0 off, 1 on, 2 on with a fine-grained arena, 3 on with in-launch waits; GRAPH_REPLAYS: hipGraphLaunch
 * calls of the solvers so far; EXCHANGES: exchanges this rank has signalled (synchronises the stream). */
#define MI_QUERY_NO_GRAPH 0
#define MI_QUERY_PEER_EXCHANGE 1
#define MI_QUERY_GRAPH_REPLAYS 2
#define MI_QUERY_EXCHANGES 3
#define MI_QUERY_EXPERIMENTAL 5    /* always 0: the EXPERIMENTAL build (persistent on-chip PCG, rocBLAS/rocSOLVER set-up route) was removed */
#define MI_QUERY_SPECTRAL_PINV 4   /* blocks of mi_nn_pinv that went to the eigen-decomposition (rocSOLVER) so far, process-wide */
#define MI_QUERY_FOLDED_PCG 6      /* launches of the folded PCG kernel issued (captured or direct) so far, process-wide */
#define MI_QUERY_GRAPH_CAPTURES 7  /* graphs the solvers have captured on this context so far (a solve that replays a cached graph adds none) */
int mi_ctx_query(mi_ctx_t ctx, int what, int64_t *out);
/* Test facility: in-process ranks. `n_ranks` contexts of ONE process (one host thread each, typically all on the same
 * device) call mi_ctx_loopback_init with the same group and then behave like ranks of a multi-GPU job: operators built
 * from a slice of the subdomains are sharded. RCCL refuses two ranks on one device; this is how the sharded paths are
 * exercised on a single-GPU box (tests/test_gpu_multirank.py, tests/test_gpu_parity.py). The group joins its contexts by
 * the peer exchange above (same-process arenas): device-side flags, graph-captured like the production path. Kernels of
 * one rank then wait for kernels of another, which needs one hardware queue per rank and copies that do not queue up
 * behind each other: set GPU_MAX_HW_QUEUES >= n_ranks and GPU_FORCE_BLIT_COPY_SIZE=1048576 in the environment BEFORE the
 * first HIP call (the runtime's defaults are 4 queues and 16 KiB). mi_ctx_loopback_init runs trial exchanges with a short
 * bound; if one expires (or GPU_MAX_HW_QUEUES < n_ranks) the whole group falls back to host-side rendezvous with eager
 * launches, as does mode 1. mode: 0 automatic, 1 host rendezvous. One process per GPU needs neither setting. */
int mi_loopback_group_create(int n_ranks, void **group);
int mi_loopback_group_destroy(void *group);
int mi_ctx_loopback_init(mi_ctx_t ctx, void *group, int rank);
int mi_loopback_group_set_mode(void *group, int mode);
int mi_ctx_allreduce_sum(mi_ctx_t ctx, double *buf, int64_t n); /* in place, follows pointer mode */

/* ---------------------------------------------------------------- operators
 * mi_csr_create — a symmetric `SparseMatrixCSC{Float64,Int64}` used as `A` in cg/pcg/defcg/defpcg
 * (`A*x` cg.jl:28,83; `mul!(Ap,A,p)` cg.jl:36,93). Pass colptr/rowval/nzval as
 * rowptr/colidx/val: for a symmetric matrix the CSC arrays are its CSR arrays.
 * A non-symmetric CSC matrix passed this way yields `A'*x` (the stdlib's gather form). */
int mi_csr_create(mi_ctx_t ctx, int64_t n_rows, int64_t n_cols, const int64_t *rowptr,
                  const int64_t *colidx, const double *val, int index_base, mi_op_t *op);

/* mi_diag_create — `M \ r` with M = diag: z = dinv .* r, or the identity when dinv == NULL
 * (Example01's AMG preconditioner is out of scope; Jacobi / none stand in). */
int mi_diag_create(mi_ctx_t ctx, int64_t n, const double *dinv, mi_op_t *op);

/* mi_spd_direct_create — `M \ r` for a sparse SPD `M::SparseMatrixCSC{Float64,Int64}`: RecyclingKrylovSolvers' pcg applies
 * its preconditioner as `z .= M \ r` (cg.jl:85, 100), a sparse Cholesky solve per call in Julia; Example07:412/416 pass
 * the interface block itself, `pcg(S, b_schur, zeros(S.N), A_ΓΓ)`. Exact, by one level of nested dissection for an
 * interface-like graph: pieces of at most 64 nodes grown breadth-first, a separator Σ from a greedy vertex cover of the
 * edges between pieces, dense inverses of the pieces' diagonal blocks and of the Schur complement s of Σ, all formed on the
 * device (no atomics: bitwise reproducible). The apply is two launches and is captured into the solvers' graphs.
 *   create    : colptr (n + 1), rowval, nzval (nnz) of the CSC matrix, HOST arrays, `index_base`-based indices. The pattern
 *               must be structurally symmetric without duplicates. |Σ| above 2048 (s^-1 would exceed 32 MB: the graph is not
 *               interface-like) is MI_ERR_BAD_ARG naming both numbers. Recursive dissection is not provided.
 *   set_values: new nzval on the same pattern (a new realization, Example07:416), host or device pointer per the context's
 *               pointer mode; only the numeric phase runs again. Synchronous.
 *   Both return MI_ERR_SINGULAR when a pivot is not positive (M not positive definite) or the certificate of s^-1 fails
 *   (||v - s^-1 s v||_inf > 4 |Σ| eps ||s^-1||_inf ||s||_inf, v = ±1); set_values then keeps the previous factor.
 * mi_spd_direct_stats — the number of pieces and |Σ| (either pointer may be NULL). */
int mi_spd_direct_create(mi_ctx_t ctx, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval,
                         int index_base, mi_op_t *op);
int mi_spd_direct_set_values(mi_op_t op, const double *nzval);
int mi_spd_direct_stats(mi_op_t op, int64_t *pieces, int64_t *separator);

/* mi_block_jacobi_create — the reference's `BJPreconditioner(nb, A)` (MyPreconditioners/BJPreconditioner.jl:1-32), the M of
 * pcg / defpcg / eigpcg / eigdefpcg on the full matrix in Examples 06, 09 (`bj$(nbj)_0`), 15, 17 and 19: nb contiguous
 * index slices of A, each factorised exactly,
 *     bsize = floor(n / nb);  slice(i) = (i-1) bsize + 1 : i bsize  for i < nb,  (i-1) bsize + 1 : n  for i = nb
 *     y[slice(i)] = cholesky(A[slice(i), slice(i)]) \ x[slice(i)]
 * on the device by the breadth-first level elimination of mi_schur_setup_* used as a complete block LDL' (block_jacobi.hpp):
 * per block a seed set G, levels grown from the nodes next to it, the level inverses kept, S_G^-1 dense. One apply is ONE
 * forward and one backward sweep over the kept inverses (3 steps + 2 plain launches, steps = the deepest block's levels),
 * captured into the solvers' graphs; no atomics, fixed summation orders: bitwise reproducible. nb = 1 is `A \ b`.
 *   create    : colptr (n + 1), rowval, nzval (nnz) of the CSC matrix, HOST arrays, `index_base`-based indices.
 *               seed_ptr (nb + 1, starting at index_base) / seed_idx (block-local, `index_base`-based): explicit seeds per block;
 *               seed_ptr == NULL selects the default rule, per connected component of a block's graph (components in ascending
 *               order of their lowest node): the nodes with a stored entry of A in a column before the slice; else those with
 *               one in a column after it; else the component's lowest node.
 *               MI_ERR_BAD_ARG, the message naming the numbers: nb < 1 or nb > n (the reference's bsize = 0 is not
 *               reproduced); a pattern that is not structurally symmetric; a component of a block without a seed (block
 *               and node); a level or a seed set of more than 2048 nodes; a context that is one rank of several (the
 *               operator is replicated only).
 *   set_values: new nzval on the same pattern (a new realization, Example06:600), host or device pointer per the context's
 *               pointer mode: one gather and the numeric phase. Synchronous.
 *   Both return MI_ERR_SINGULAR when a block is singular or not positive definite as far as the factor shows it (a value
 *   that is not finite, a diagonal entry of a kept inverse or of S_G^-1 that is not positive, or a failed certificate of
 *   S_G^-1: mi_nn_pinv's probe, the plain inverse only); set_values then keeps the previous factor.
 * mi_block_jacobi_stats — per block (arrays of nb, any may be NULL): seeds, levels, widest level; kept_bytes = 8 Σ n_level². */
int mi_block_jacobi_create(mi_ctx_t ctx, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, int64_t nb,
                           const int64_t *seed_ptr, const int64_t *seed_idx, int index_base, mi_op_t *op);
int mi_block_jacobi_set_values(mi_op_t op, const double *nzval);
int mi_block_jacobi_stats(mi_op_t op, int64_t *n_g, int64_t *n_levels, int64_t *max_level, int64_t *kept_bytes);

/* mi_amg_create — the reference's `Preconditioners.AMGPreconditioner{SmoothedAggregation}(A)`, the M of `pcg(A, b, 0, Π_amg)`
 * in Example01:49-61 (and Examples 06, 09, 10, 12-20): one V(1,1) cycle of smoothed-aggregation AMG per `M \ r` (amg.hpp),
 *     coarsest: x = A_c^-1 b;  else  x = (ω/d) b;  r = b - A_l x;  e = cycle(l + 1, P_l' r);  x += P_l e;  x += (ω/d) (b - A_l x)
 * The smoother is Jacobi damped by ω_l where the reference sweeps symmetric Gauss-Seidel (sequential). The
 * hierarchy comes from the host (fem.prepare_amg_precond, or any other set-up); all arrays are HOST arrays:
 *   nlevels, n_l[nlevels]          rows of every level, strictly decreasing; the last one at most 4096
 *   a_rowptr / a_colidx / a_val    [nlevels] pointers: CSR of the symmetric A_l (`index_base`-based)
 *   p_rowptr / p_colidx / p_val    [nlevels - 1] pointers: CSR of P_l, n_l x n_{l+1} (may be NULL when nlevels == 1)
 *   omega_over_d                   ω_l / diag(A_l) of the levels l < nlevels - 1, back to back (Σ n_l doubles)
 *   coarse_inv                     the symmetric inverse of the coarsest level, n_c x n_c, column-major
 * R_l = P_l' is built here in CSR; one apply is 4 (nlevels - 1) + 1 launches with fixed summation orders (bitwise
 * reproducible), no atomics and no host synchronisation, captured into the solvers' graphs. nlevels == 1 is `A \ b` by the
 * dense inverse. MI_ERR_BAD_ARG with a mi_last_error() text: nlevels < 1, level sizes that do not chain, a P_l that is not
 * n_l x n_{l+1}, a value that is not finite, a coarsest level above 4096 rows, a context that is one rank of several.
 * mi_amg_stats — levels, rows of the coarsest level, Σ_l nnz(A_l), and bytes_kept = Σ_{l < nlevels-1} (12 nnz(A_l) +
 * 24 nnz(P_l) + 8 n_l) + 8 n_c² (values and column indices of the smoothed A_l, of P_l and R_l; ω/d; the inverse). Any pointer may be NULL. */
int mi_amg_create(mi_ctx_t ctx, int64_t nlevels, const int64_t *n_l, const int64_t *const *a_rowptr, const int64_t *const *a_colidx,
                  const double *const *a_val, const int64_t *const *p_rowptr, const int64_t *const *p_colidx, const double *const *p_val,
                  const double *omega_over_d, const double *coarse_inv, int index_base, mi_op_t *op);
int mi_amg_stats(mi_op_t op, int64_t *n_levels, int64_t *coarse_n, int64_t *operator_nnz, int64_t *bytes_kept);
/* mi_amg_plan_create / mi_amg_set_values — the same operator with the NUMBERS of the hierarchy made on the device, for the
 * studies that rebuild `AMGPreconditioner{SmoothedAggregation}(A)` per realization (`Π_amg_t` of Example06:167-182;
 * Example12:106, Example14:153, Example19:101, Example20:111; the `Π_IId` of Example07:174). The aggregation sees the values
 * of a matrix only through `!= 0`, so on one mesh every realization has the aggregates — and every sparsity pattern of the
 * hierarchy — of the first; the symbolic part is done once on the host (amg_plan.hpp), the numeric chain per nzval on the
 * device (amg_setup.hpp): g_l, ω_l = 4 / (3 g_l), ω_l / d, P_l = (I - ω_l D^-1 A_l) T_l, R_l = P_l', A_{l+1} = sym(R_l A_l P_l) on
 * the STRUCTURAL product patterns (no entry is dropped because it cancels), and the dense inverse of the last level by the
 * SPD route of mi_nn_pinv with its certificate. No atomics, every sum in a fixed order: two refreshes give the same bits.
 *   create    : HOST arrays, `index_base`-based. rowptr (n + 1) / colidx / val: the CSR of A_0, rows sorted without
 *               duplicates, stored zeros are entries; n_l[nlevels]: rows per level; agg[l] (l < nlevels - 1, n_l[l] entries):
 *               the aggregate of every node, in index_base .. index_base + n_l[l+1] - 1 (fem.prepare_amg_precond(A).agg).
 *               The result is an AMG operator like that of mi_amg_create (apply, solvers, mi_amg_stats).
 *               MI_ERR_BAD_ARG, the message naming the numbers: a pattern that is not sorted, has duplicates or is not
 *               structurally symmetric; an aggregate id out of range; an empty aggregate; level sizes that do not chain; a
 *               coarsest level above 4096 rows; a context that is one rank of several.
 *   set_values: new `val` on the pattern of create (a new realization), host or device pointer per the context's pointer
 *               mode. Synchronous. MI_ERR_BAD_ARG on an operator of mi_amg_create.
 *   Both return MI_ERR_SINGULAR when a diagonal entry of a level is missing or not positive, a value is not finite, or the
 *   certificate of the coarse inverse fails; set_values then keeps the previous hierarchy: new values are computed into a
 *   second set of buffers and committed by device copies, the addresses the cycle and captured solve graphs read never change.
 *   Limit: the aggregates are those handed to create. A later matrix with a different set of stored non-zeros gets a valid
 *   hierarchy, but not the one a fresh host set-up would build.
 * mi_amg_stats of such an operator: bytes_kept additionally counts the plan and the second buffers,
 *   Σ_levels 4 (2 n_l + 2 nnz(A_l) + 1) + Σ_{l < nlevels-1} [4 (4 nnz(P_l) + nnz(A_l) + nnz(A_l P_l) + 3 n_l + n_{l+1} + 4) + 8 n_{l+1}]   (the plan)
 *   + Σ_{l >= 1} 8 nnz(A_l) + Σ_{l < nlevels-1} (16 nnz(P_l) + 8 n_l) + 8 (max_l nnz(A_l P_l) + max_{l >= 1} nnz(A_l)) + 32 n_c²
 *   + 12 nnz(A_{nlevels-1})   (candidates, product work, dense work, and the coarsest matrix kept for the read-back).
 * Read-back (operators of either create route; HOST arrays, 0-based; any output pointer may be NULL):
 *   mi_amg_level_sizes: rows of `level`, rows of the next (0 on the last level), nnz(A_level), nnz(P_level) (0 on the last)
 *   mi_amg_level_get  : CSR of A_level (n + 1, nnz, nnz) and of P_level, ω_level (one double) and ω_level / d (n doubles);
 *                       the P, ω outputs are left alone on the last level. An operator of mi_amg_create was given ω/d only:
 *                       its ω_level is (ω/d)_0 a_00, one rounding away.
 *   mi_amg_coarse_inverse: the n_c x n_c inverse of the last level, column-major.
 * mi_amg_refresh_profile — diagnostic (operators of mi_amg_plan_create): one refresh on the values the operator holds, timed
 *   by HIP events on the context's stream; ms[6] = Gershgorin bound and ω; prolongator and R; A P; R (A P) and its
 *   symmetrisation; the coarsest level (scatter, inverse, certificate, with their host synchronisations); the commit copies. */
int mi_amg_plan_create(mi_ctx_t ctx, int64_t n, const int64_t *rowptr, const int64_t *colidx, const double *val, int64_t nlevels,
                       const int64_t *n_l, const int64_t *const *agg /* [nlevels - 1] */, int index_base, mi_op_t *op);
int mi_amg_set_values(mi_op_t op, const double *val);
int mi_amg_level_sizes(mi_op_t op, int64_t level, int64_t *n_rows, int64_t *n_cols, int64_t *a_nnz, int64_t *p_nnz);
int mi_amg_level_get(mi_op_t op, int64_t level, int64_t *a_rowptr, int64_t *a_colidx, double *a_val, int64_t *p_rowptr,
                     int64_t *p_colidx, double *p_val, double *omega, double *omega_over_d);
int mi_amg_coarse_inverse(mi_op_t op, double *coarse_inv);
int mi_amg_refresh_profile(mi_op_t op, double *ms /* 6 */);

/* mi_amg_bank_* — P hierarchies of mi_amg_plan_create on ONE plan (amg_bank.hpp): the constant preconditioners of the
 * quantization studies, one per centroid on frozen aggregates (`get_centroidal_preconds`, Example12_…_Functions.jl:85-113;
 * Examples 13, 14, 18, 20). The plan, the index arrays and row blocks of every A_l, P_l, R_l and the numeric set-up engine
 * (candidate buffers, dense work) are held once; a member is numbers only, one slot of a value slab that is allocated at
 * creation and never moves. Every handle is an mi_op_t; members are 0-based.
 *   create     : as mi_amg_plan_create without `val` (HOST arrays, `index_base`-based), and `capacity` >= 1 slots. No member
 *                is set yet. The bank is NOT applicable: mi_op_apply, mi_op_combine and every solver refuse it with
 *                MI_ERR_BAD_ARG before any launch; mi_op_size gives n. mi_op_destroy is refused (MI_ERR_BAD_ARG, "... live
 *                view(s) (mi_amg_bank_view) borrow this AMG bank; destroy them first") while a view lives. A slab that does
 *                not fit is MI_ERR_HIP, the message naming the bytes asked for.
 *   set_values : the numeric chain of mi_amg_set_values on `val` (host or device pointer per the context's pointer mode, on
 *                the pattern of create), then — only on success — the result is copied into the member's slot. Synchronous.
 *                MI_ERR_SINGULAR leaves the slot bit for bit as it was; a slot never set stays unset.
 *   view       : an operator of size n that borrows the bank, usable wherever an AMG operator is (M of mi_pcg, mi_defpcg,
 *                mi_eigpcg, mi_eigdefpcg, mi_initpcg; a child of mi_op_combine; mi_op_apply), with its own level vectors for
 *                `max_terms` (1 .. 16) members. z = Σ_i coef[i] (Π_{members[i]} \ r), i ascending as mi_op_combine sums: the
 *                V(1,1) cycles of all k members in ONE sequence of 4 (nlevels - 1) + 1 launches (the member is the grid's
 *                second dimension) and one combination launch. A member's cycle has the bits of the operator of
 *                mi_amg_plan_create / mi_amg_set_values on the same values. A new view selects k = 1, member 0, coefficient 1.
 *   select     : k HOST member indices and k finite HOST coefficients into the view's device arrays, a blocking copy on the
 *                context's stream. The kernels read k and the members on the device, so solve graphs captured with the view
 *                stay valid and the next solve uses the new selection.
 *   stats      : capacity; members set so far; bytes_shared (mi_amg_stats' bytes_kept of the engine: patterns, plan,
 *                candidates, work and the buffers a member is staged in); views alive; and
 *                  bytes_per_member = 8 (Σ_l nnz(A_l) + 2 Σ_{l<L-1} nnz(P_l) + Σ_{l<L-1} n_l + n_c² + 2 (L - 1)) + padding,
 *                L = nlevels, for the values of every A_l (the coarsest as given, for the read-back), of P_l and R_l, ω_l/d, the
 *                coarse inverse and the (ω_l, g_l) pairs. padding = 8 bytes for every one of the arrays A_l (L of them), P_l,
 *                R_l, ω_l/d (L - 1 each) and the inverse whose count of doubles is odd: each array is padded to an even
 *                count, so every array of every member starts on a 16-byte boundary (the cycle loads values in pairs).
 *   level_sizes / level_get / coarse_inverse: the read-back of mi_amg_level_sizes / mi_amg_level_get /
 *                mi_amg_coarse_inverse for one member (the sizes are those of every member).
 * MI_ERR_BAD_ARG, the message naming the numbers: everything mi_amg_plan_create refuses; capacity < 1; a member outside
 * 0 .. capacity - 1; a selected or read member that was never set — at select, and at apply or solve entry when the default
 * member 0 is unset; k < 1 or k > max_terms; max_terms outside 1 .. 16; a coefficient that is not finite; a handle of the wrong
 * kind; a context that is one rank of several. */
int mi_amg_bank_create(mi_ctx_t ctx, int64_t n, const int64_t *rowptr, const int64_t *colidx, int64_t nlevels, const int64_t *n_l,
                       const int64_t *const *agg /* [nlevels - 1] */, int64_t capacity, int index_base, mi_op_t *bank);
int mi_amg_bank_set_values(mi_op_t bank, int64_t member, const double *val);
int mi_amg_bank_view(mi_op_t bank, int64_t max_terms, mi_op_t *view);
int mi_amg_bank_select(mi_op_t view, int64_t k, const int64_t *members, const double *coef);
int mi_amg_bank_stats(mi_op_t bank, int64_t *capacity, int64_t *members_set, int64_t *bytes_shared, int64_t *bytes_per_member,
                      int64_t *views);
int mi_amg_bank_level_sizes(mi_op_t bank, int64_t level, int64_t *n_rows, int64_t *n_cols, int64_t *a_nnz, int64_t *p_nnz);
int mi_amg_bank_level_get(mi_op_t bank, int64_t member, int64_t level, int64_t *a_rowptr, int64_t *a_colidx, double *a_val,
                          int64_t *p_rowptr, int64_t *p_colidx, double *p_val, double *omega, double *omega_over_d);
int mi_amg_bank_coarse_inverse(mi_op_t bank, int64_t member, double *coarse_inv);

/* mi_csr_batch_* / mi_pcg_batch — k realizations in ONE Krylov loop (csr_batch.hpp, batch_solvers.hpp): the Monte-Carlo loops
 * `for ireal in 1:nreals … pcg(A_t, b_t, 0, Π[p(ξ_t)])` of Examples 06, 12, 14, 19, 20, whose systems are independent, share
 * every launch. Slots and members are 0-based; every handle is an mi_op_t.
 *   create     : the pattern (HOST arrays, `index_base`-based, as mi_csr_create without values; n >= 1, square) and `capacity`
 *                >= 1 value slots. rowptr, col, the row blocks and their XCD ranges are held once; the value slab is allocated
 *                here and never moves. No slot is set yet. The batch is NOT applicable: mi_op_apply, mi_op_combine and the
 *                single-system solvers refuse it with MI_ERR_BAD_ARG before any launch; mi_op_size gives n.
 *   set_values : nnz values on the pattern into slot `slot` (host or device pointer per the context's pointer mode; a device
 *                pointer is copied asynchronously on the context's stream).
 *   get_values : the read-back of a slot that was set (pointer mode as set_values; synchronous).
 *   stats      : capacity; slots set so far; bytes_shared (the index arrays and row blocks); and
 *                  bytes_per_slot = 8 (nnz + nnz mod 2):
 *                the slot stride is padded to an even count of doubles, so every slot starts on a 16-byte boundary (the
 *                SpMV loads values in pairs at the even offsets of the row blocks). mi_csr_batch_stride(nnz, &doubles) is
 *                that stride in doubles, host arithmetic only.
 *   mi_full_assembly_update_batch: mi_full_assembly_update with the values written straight into slot `slot` — the same
 *                kernel, the same bits; b as there. The pattern is compared in full the first time a plan meets a batch.
 *   mi_pcg_batch: for t < k, X[:, t] = pcg(A_t, B[:, t], X[:, t], Π_{members[t]}) with A_t = slot slots[t] of the batch and
 *                Π_m = member m of the bank under the view `M_view` (M_view == NULL: cg, `members` is not read). B (n x k,
 *                ldb) and X (n x k, ldx; X0 in, the iterates out) are column-major and follow the context's pointer mode;
 *                slots, members, it[k] and res_norm (ldres x k, column-major: res_norm[0 .. it[t]) of system t in column t)
 *                are HOST arrays. A slot or a member may appear several times. maxit, eps: as mi_pcg, for every system.
 *                One form: the arithmetic of the multi-workgroup loop of mi_pcg on a sparse matrix with a non-diagonal M,
 *                system t as the grid's second dimension and every partial sum in the single solve's order — x, it and
 *                res_norm of system t carry the bits of the single solve of that system with the view selecting members[t].
 *                A system whose stop rule has fired is frozen; the loop ends when none is active. The view's own selection
 *                (mi_amg_bank_select) is not touched. k, slots and members are read on the device, so the graphs captured
 *                for (batch, view) serve every later selection; MI_QUERY_GRAPH_REPLAYS / _CAPTURES count them, and
 *                mi_op_destroy of the batch or the view drops them. Replay policy: as mi_pcg (the first graph holds the set-up
 *                and the iterations the longest system of the previous batch on this (batch, view) took).
 *                MI_ERR_RES_CAPACITY after the solve has completed if some it[t] > ldres: it is filled and X is valid.
 * MI_ERR_BAD_ARG, the message naming the numbers: everything mi_csr_create refuses of a pattern; n < 1; capacity < 1; a slot
 * outside 0 .. capacity - 1; a solved or read slot, or a member, that was never set; k < 1, k > 16 or k above the view's
 * max_terms; ldb or ldx below n; a handle of the wrong kind; A and M of different size or context; a pattern that is not the
 * plan's; a context that is one rank of several. */
int mi_csr_batch_create(mi_ctx_t ctx, int64_t n, const int64_t *rowptr, const int64_t *colidx, int64_t capacity, int index_base,
                        mi_op_t *batch);
int mi_csr_batch_set_values(mi_op_t batch, int64_t slot, const double *val);
int mi_csr_batch_get_values(mi_op_t batch, int64_t slot, double *val);
int mi_csr_batch_stats(mi_op_t batch, int64_t *capacity, int64_t *slots_set, int64_t *bytes_shared, int64_t *bytes_per_slot);
int mi_csr_batch_stride(int64_t nnz, int64_t *doubles);
int mi_pcg_batch(mi_op_t A_batch, int64_t k, const int64_t *slots, mi_op_t M_view /* NULL: cg */, const int64_t *members,
                 const double *B, int64_t ldb, double *X, int64_t ldx, int64_t maxit, double eps, double *res_norm, int64_t ldres,
                 int64_t *it /* [k] */);

/* mi_amg_bank_set_values_batch — the numeric set-up of k <= 16 bank members in ONE sequence of launches
 * (csrc/amg_bank_setup.hpp): term t builds member members[t] from the values in slot slots[t] of `A_batch`, read on the
 * device where they lie (no staging copy of A_0, no host round trip of values); the term is the grid's second dimension.
 * members, slots and status are HOST arrays, 0-based. A member built here carries the bits of mi_amg_bank_set_values on the
 * same values. Every term is committed separately: a term whose chain fails (a value that is not finite, a diagonal entry of a
 * level missing or not positive, a coarse inverse without its certificate) leaves its member bit for bit as it was (unset, if
 * it never was set); the healthy terms of the same call are committed. status[t] = MI_OK or MI_ERR_SINGULAR. Returns MI_OK when
 * every term succeeded, and when `status` is given and only terms failed; with status == NULL a failed term makes the call
 * return MI_ERR_SINGULAR after the healthy terms are committed, the message naming the failed terms and their reasons.
 * Synchronous. Slot addresses never move: solve graphs captured on views of the bank stay valid. The workspace (k candidate
 * slots and the per-term work) is allocated at the first call, grows only when a call has more terms than any before, and is
 * counted in mi_amg_bank_stats' bytes_shared from then on.
 * MI_ERR_BAD_ARG before any launch, the message naming the numbers: k < 1 or k > 16; a member or slot out of range; a slot
 * never set; the same member twice (the same slot twice is allowed); a handle of the wrong kind; bank and batch of different
 * contexts or sizes; a batch whose pattern is not the bank's (compared in full the first time this bank meets this batch); a
 * context that is one rank of several. */
int mi_amg_bank_set_values_batch(mi_op_t bank, int64_t k, const int64_t *members, mi_op_t A_batch, const int64_t *slots,
                                 int *status /* [k], may be NULL */);

/* mi_schur_assembled_create — `apply_local_schurs(Sd, ind_Γd_Γ2l, node_Γ_cnt, x)`, EPDD.jl:761-785:
 * Sx = Σ_d R_d' S_d R_d x with dense local Schur complements.
 *   Sd[d]          n_gamma_d[d]^2 doubles, column-major (Julia `Array(Sd[d])`)
 *   gather_idx[d]  n_gamma_d[d] entries: Γ index of Γ_d slot l (the flattened Dict ind_Γd_Γ2l[d]:
 *                  gather_idx[d][lΓd] = lΓ). Pass the lists of ALL subdomains on every rank, also outside
 *                  [dom_begin, dom_end): they fix each subdomain's slot in the per-node contribution table, so that
 *                  the ranks' tables are disjoint and their all-reduce reproduces the single-GPU Γ-sum bit for bit
 * The local slice [dom_begin, dom_end) of the ndom subdomains is applied by this rank. On a context with a
 * communicator a proper slice makes the operator SHARDED: its applies end with one RCCL all-reduce (of the table of
 * per-subdomain contributions, so the Γ-sum keeps the single-GPU order and bits). An operator created with
 * dom_begin = 0, dom_end = ndom is REPLICATED and never communicates, with or without a communicator (single-GPU
 * use; or e.g. the Neumann-Neumann blocks copied to every rank while S is sharded: one all-reduce per PCG
 * iteration instead of two). Arrays of subdomains outside the slice may be NULL. */
int mi_schur_assembled_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                              const int64_t *const *gather_idx, const double *const *Sd, int index_base,
                              int64_t dom_begin, int64_t dom_end, mi_op_t *op);

/* mi_nn_create — `NeumannNeumannSchurPreconditioner(ΠSd, ind_Γd_Γ2l, node_Γ_cnt)` (EPDD.jl:1111-1137)
 * used through `Πnn \ r` / `ldiv!` = apply_neumann_neumann_schur (EPDD.jl:1361-1403):
 * z = Σ_d R_d' D_d ΠS_d D_d R_d r, D = diag(1 ./ node_Γ_cnt). ΠSd[d] column-major dense. */
int mi_nn_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                 const int64_t *const *gather_idx, const double *const *PiSd, const int64_t *node_gamma_cnt,
                 int index_base, int64_t dom_begin, int64_t dom_end, mi_op_t *op);

/* mi_nn_create_stored — the same operator (EPDD.jl:1111-1137, applied as EPDD.jl:1361-1403) with the ΠS_d blocks HELD in
 * `storage`: MI_STORE_F64 (what mi_nn_create does) or MI_STORE_F32. PiSd[d] is fp64 column-major either way; with
 * MI_STORE_F32 every entry is rounded once to fp32 (nearest even, subnormals kept: a C `(float)` cast) and the apply is
 * the fp64 apply of the blocks double(float(ΠS_d)) up to summation order — operand r / cnt, products, sums, scaling
 * and everything the solvers do stay fp64, half the bytes are streamed. Rounding a symmetric block element-wise keeps it
 * symmetric, and PCG asks nothing of M but to be symmetric positive definite.
 * Precedent: the reference's low-precision preconditioner wrappers Cholesky32 / Cholesky16
 * (MyPreconditioners/CholPreconditioners.jl:32-56). Deliberately NOT their semantics: those also round r and solve in
 * fp32; here fp32 is a storage format only.
 * A block entry that is not finite or exceeds FLT_MAX in magnitude is MI_ERR_BAD_ARG (the message names the block), as
 * is an unknown `storage`. mi_dense_set_blocks keeps taking fp64 blocks and converts on the way (host pointers are
 * checked like at creation; device pointers are converted asynchronously, unchecked). S_d has no fp32 form. */
#define MI_STORE_F64 0
#define MI_STORE_F32 1
int mi_nn_create_stored(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                        const int64_t *const *gather_idx, const double *const *PiSd, const int64_t *node_gamma_cnt,
                        int index_base, int64_t dom_begin, int64_t dom_end, int storage, mi_op_t *op);
/* Storage kind of an operator's dense blocks: MI_STORE_F32 for an fp32-stored Neumann-Neumann operator, MI_STORE_F64 for
 * every other operator. */
int mi_op_storage(mi_op_t op, int *storage);

/* mi_schur_matfree_create — `apply_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt, x)`,
 * EPDD.jl:711-747 (per subdomain apply_local_schur, EPDD.jl:639-654):
 * S_d x_d = A_ΓΓdd x_d − A_IΓdd' (A_IIdd^{-1} (A_IΓdd x_d)). The three sparse products run on the
 * device; A_IIdd^{-1} is the host callback (BASELINE north_star: interior solve stays on the host).
 *   A_IΓdd[d]: CSC arrays (colptr n_gamma_d[d]+1, rowval, nzval) of the n_i[d] x n_gamma_d[d] block
 *   A_ΓΓdd[d]: CSC arrays of the symmetric n_gamma_d[d] x n_gamma_d[d] block */
int mi_schur_matfree_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                            const int64_t *n_i, const int64_t *const *gather_idx,
                            const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                            const double *const *ig_nzval, const int64_t *const *gg_colptr,
                            const int64_t *const *gg_rowval, const double *const *gg_nzval,
                            mi_interior_solve_fn solve, void *user, int index_base,
                            int64_t dom_begin, int64_t dom_end, mi_op_t *op);

/* mi_schur_matfree_device_create — the same operator with the interior solve ON THE DEVICE, as the reference
 * does it: `IterativeSolvers.cg(A_IIdd, A_IΓdd*xd, reltol=reltol)` from a zero initial guess (EPDD.jl:648-650,
 * default reltol 1e-9; no preconditioner — the reference's AMG `Pl` is out of scope). All local subdomains are
 * iterated together on the block-diagonal A_II with per-subdomain scalars; a subdomain stops when its residual
 * is <= reltol * ||rhs|| or after n_i iterations.
 *   A_IIdd[d]: CSC arrays of the symmetric n_i[d] x n_i[d] interior block. */
int mi_schur_matfree_device_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                                   const int64_t *n_i, const int64_t *const *gather_idx,
                                   const int64_t *const *ii_colptr, const int64_t *const *ii_rowval,
                                   const double *const *ii_nzval, const int64_t *const *ig_colptr,
                                   const int64_t *const *ig_rowval, const double *const *ig_nzval,
                                   const int64_t *const *gg_colptr, const int64_t *const *gg_rowval,
                                   const double *const *gg_nzval, double reltol, int index_base,
                                   int64_t dom_begin, int64_t dom_end, mi_op_t *op);

/* mi_schur_global_create — `apply_global_schur(A_IId, A_IΓd, A_ΓΓ, x)`, EPDD.jl:596-625:
 * Sx = A_ΓΓ x − Σ_d A_IΓd' (A_IId^{-1} (A_IΓd x)), Γ-global column indices (no gather maps).
 *   A_IΓd[d]: CSC arrays of the n_i[d] x n_gamma block;  A_ΓΓ: CSC arrays, symmetric. */
int mi_schur_global_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_i,
                           const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                           const double *const *ig_nzval, const int64_t *gg_colptr,
                           const int64_t *gg_rowval, const double *gg_nzval,
                           mi_interior_solve_fn solve, void *user, int index_base, mi_op_t *op);
/* The same with the interior solves on the device, as for mi_schur_matfree_device_create: `IterativeSolvers.cg(A_IId[idom],
 * A_IΓd[idom]*x)` (EPDD.jl:609-619) restated; the reference calls it with the package default reltol = sqrt(eps). */
int mi_schur_global_device_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_i,
                                  const int64_t *const *ii_colptr, const int64_t *const *ii_rowval,
                                  const double *const *ii_nzval, const int64_t *const *ig_colptr,
                                  const int64_t *const *ig_rowval, const double *const *ig_nzval,
                                  const int64_t *gg_colptr, const int64_t *gg_rowval, const double *gg_nzval,
                                  double reltol, int index_base, mi_op_t *op);

/* mi_schur_interior_precond — the `precond` / `preconds` keyword of apply_local_schur / apply_global_schur (EPDD.jl:648-650,
 * 609-619: `IterativeSolvers.cg(A_IIdd, rhs, Pl=precond, reltol=reltol)`) for an operator made by one of the two
 * *_device_create calls above. kind 0: none (the default, plain CG); kind 1: Pl = Diagonal(A_IIdd) (Jacobi). The reference's own
 * choice, an AMG hierarchy from Preconditioners.jl, is outside the hot path; the diagonal costs nothing per
 * iteration (it is folded into the update kernel) and about halves the iteration counts on lognormal coefficient fields. */
int mi_schur_interior_precond(mi_op_t op, int kind);
/* Diagnostic: iterations the interior CG of such an operator has run so far (slowest subdomain, rounded up to replays). */
int mi_schur_interior_iterations(mi_op_t op, int64_t *iterations);
/* mi_schur_interior_amg — Pl = smoothed-aggregation AMG in that interior CG: the reference's own choice, the Π_IId of
 * `IterativeSolvers.cg(A_IId, rhs; Pl = Π_IId, reltol)` (EPDD.jl:609-619, 648-650, 813-815, 1021; Example07:174), for an operator
 * of mi_schur_matfree_device_create or mi_schur_global_device_create. ONE hierarchy of the stacked block-diagonal matrix
 * A_II = blockdiag(A_IIdd) of the operator's subdomains, built on the device from the operator's own pattern and current values
 * by the machinery of mi_amg_plan_create: n_l[nlevels] the level sizes (n_l[0] = Σ_d n_i[d]), agg[l] (n_l[l] entries,
 * l < nlevels - 1) the aggregate of every stacked node of level l, `index_base`-based. ω_l is the Gershgorin maximum over all
 * subdomains and the coarsest level has one dense inverse: the result is a block-diagonal SPD operator, so the subdomains'
 * iterations stay independent (it differs from a hierarchy per subdomain in ω_l and in the level count). One V(1,1) cycle per
 * iteration on the whole stacked vector; the loop always has three launches plus the cycle's per iteration (MI355_ICG_FUSED is
 * ignored meanwhile) and 4 iterations per graph replay unless MI355_ICG_CHUNK says otherwise.
 *   MI_ERR_BAD_ARG: a host-callback operator, a sharded operator, a context with a communicator, everything
 *                   mi_amg_plan_create refuses (level sizes, aggregate ids, an A_II pattern that is not sorted or not
 *                   structurally symmetric), an aggregate that holds nodes of two subdomains.
 *   MI_ERR_SINGULAR: as mi_amg_plan_create. Either way the `Pl` selected before stays.
 * A later mi_schur_interior_precond(op, 0 | 1) deselects it and releases the hierarchy.
 * mi_schur_matfree_set_values(ii_val != NULL) then redoes the numbers of the hierarchy on the device for the new values (host
 * or device pointer, as the context's pointer mode says) BEFORE it stores anything: when the refresh fails (MI_ERR_SINGULAR:
 * a diagonal entry of a level that is not positive, a value that is not finite, a coarse inverse that fails its certificate)
 * the call returns the error and the operator — matrices, diagonal, hierarchy — is the one of before.
 * mi_schur_interior_amg_stats: levels, rows of the coarsest level, bytes the hierarchy keeps (any pointer may be NULL). */
int mi_schur_interior_amg(mi_op_t op, int64_t nlevels, const int64_t *n_l, const int64_t *const *agg, int index_base);
int mi_schur_interior_amg_stats(mi_op_t op, int64_t *levels, int64_t *coarse_n, int64_t *bytes_kept);

int mi_op_size(mi_op_t op, int64_t *n);
/* y = A*x (operator) or y = M \ x (preconditioner); x and y must not alias. */
int mi_op_apply(mi_op_t op, const double *x, double *y);
/* Algorithmic bytes of one apply (SURVEY.md §8d formulas) and of its dominant kernel alone; dense blocks count in the
 * format they are stored in (fp32-stored Neumann-Neumann: Σ_d 4 n_Γd² + 20 n_Γd for the kernel). */
int mi_op_bytes(mi_op_t op, int64_t *bytes_apply, int64_t *bytes_dominant_kernel);
/* Diagnostic: launch only the dominant kernel of the apply `reps` times (x as in mi_op_apply). */
int mi_op_apply_dominant(mi_op_t op, const double *x, int reps);
/* Diagnostic: average duration (microseconds) of the dominant kernel over `reps` launches replayed from one
 * graph, measured with HIP events on the context's stream (what bench.py reports as roofline.us_per_launch). */
int mi_op_time_dominant(mi_op_t op, const double *x, int reps, double *us_per_launch);
/* Synchronises the context's stream, drops every solve graph and iteration prediction captured with the operator (as A or M,
 * directly or inside a combined or LORASC M), then frees it: an operator created later may live at the same address, with
 * device arrays at the same addresses, and is a new operator to every solver and plan. NULL is a no-op.
 * MI_ERR_BAD_ARG, nothing changed, while another live operator borrows this one: a LORASC operator its A_ΓΓ solver ("... live
 * LORASC operator(s) use this operator; destroy them first"), a combined operator its children ("this operator holds k
 * place(s) among the children of live combined operator(s) (mi_op_combine); destroy them first"). Destroy the borrower
 * first. An operator must be destroyed before its context. */
int mi_op_destroy(mi_op_t op);

/* ---------------------------------------------------------------- BLAS-1 on the device
 * `dot`, `norm2`, `axpy!`, `axpby!` as imported at RecyclingKrylovSolvers.jl:3 (level-1 drop-ins). */
int mi_dot(mi_ctx_t ctx, int64_t n, const double *x, const double *y, double *result);
int mi_norm2(mi_ctx_t ctx, int64_t n, const double *x, double *result);
int mi_axpy(mi_ctx_t ctx, int64_t n, double a, const double *x, double *y);            /* y += a x     */
int mi_axpby(mi_ctx_t ctx, int64_t n, double a, const double *x, double b, double *y); /* y = a x + b y */

/* ---------------------------------------------------------------- solvers (whole loop on the device)
 * Reference signatures (RecyclingKrylovSolvers/cg.jl:14-18, 67-72; defcg.jl:24-29, 242-248):
 *     cg(A,b,x;maxit=0)  pcg(A,b,x,M;maxit=0)  defcg(A,b,x,W;maxit=0)  defpcg(A,b,x,W,M;maxit=0)
 *     -> (x, it, res_norm[1:it])
 * x is read as the initial guess and overwritten with the solution (the reference mutates x).
 * maxit == 0 means n (cg.jl:25). eps is the module constant 1e-7 (RecyclingKrylovSolvers.jl:21)
 * made explicit; pass eps <= 0 for that default. Stop rule (cg.jl:34, 91): iterate while
 * it < maxit && res_norm[it] > eps*norm2(b), with res_norm[it] = sqrt(r'r) of the recurrence
 * residual; `it` counts from 1. res_norm receives it entries (capacity res_cap >= it required,
 * else MI_ERR_RES_CAPACITY after the solve completed). W is n x nvec, column-major. */
int mi_cg(mi_op_t A, const double *b, double *x, int64_t maxit, double eps, double *res_norm,
          int64_t res_cap, int64_t *it);
int mi_pcg(mi_op_t A, mi_op_t M, const double *b, double *x, int64_t maxit, double eps,
           double *res_norm, int64_t res_cap, int64_t *it);
int mi_defcg(mi_op_t A, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit,
             double eps, double *res_norm, int64_t res_cap, int64_t *it);
int mi_defpcg(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec,
              int64_t maxit, double eps, double *res_norm, int64_t res_cap, int64_t *it);

/* ---------------------------------------------------------------- on-device block assembly (per-realization update)
 * Replaces the element loop of `prepare_local_schurs(cells, points, epart, ..., coeff, f, uexact)`
 * (EPDD.jl:389-546) when only the nodal coefficient vector `a` changes between calls — Example07:162-171 redoes the
 * whole loop on the host for every realization. The caller prepares the index half once:
 *   cells  3 x nel node indices (row i contiguous: vertex i of every element), `index_base` 0 or 1
 *   G      9 x nel, G[3i+j] = Δy_i Δy_j + Δx_i Δx_j (:448-453, 470);  area  nel (:456)
 *   ue     3 x nel, uexact at vertex i (Dirichlet lifting, :498-507); be  3 x nel, Δb_i = (2f_i+f_j+f_k) Area/12 (:516-525)
 *   cptr / ccode: entry k of the output is the sum, IN ORDER, of the contributions ccode[cptr[k] .. cptr[k+1]), each
 *   coded 12*element + 3i + j (ΔK_ij = Δa G_ij/4/Area with Δa = (a_1+a_2+a_3)/3; for k >= n_matrix_entries the
 *   lifting term -(ΔK_ij ue_i)) or 12*element + 9 + i (Δb_i); 0-based. The order inside an entry is the order in which
 *   `sparse(I,J,V)` / `b[k] +=` met the terms (ascending element), so results are bit-identical to the host loop.
 * mi_assembly_run: a_nodal (n_node) -> values (n_entries); host or device pointers per the context's pointer mode
 *   (device pointers: asynchronous on the context's stream, like mi_op_apply).
 * mi_schur_matfree_set_values: new block values for a matrix-free operator, same sparsity as at create; each array is
 *   the concatenation over the operator's subdomains [dom_begin, dom_end) of the arrays passed at create (A_IIdd: its
 *   CSC/CSR values; A_IΓdd: CSC values; A_ΓΓdd); NULL leaves a block unchanged; ii_val needs the device interior solve.
 * mi_schur_matfree_rhs: `get_schur_rhs` (EPDD.jl:835-864): b_schur = b_Γ - Σ_d R_d' A_IΓdd' (A_IIdd \ b_Id) with the
 *   operator's own interior solve; b_I is the concatenation of the b_Id. Collective on a sharded operator. Also accepts
 *   a global Schur operator (mi_schur_global_*create): the Γ-global form, EPDD.jl:798-821; likewise
 *   mi_schur_matfree_interior_solutions (there it is the reference's own signature, A_IΓd with global columns). */
int mi_assembly_plan_create(mi_ctx_t ctx, int64_t nel, int64_t n_node, const int64_t *cells, int index_base,
                            const double *G, const double *area, const double *ue, const double *be, int64_t n_entries,
                            int64_t n_matrix_entries, const int64_t *cptr, const int64_t *ccode, mi_plan_t *plan);
int mi_assembly_run(mi_plan_t plan, const double *a_nodal, double *values);
int mi_assembly_plan_destroy(mi_plan_t plan);
/* ---------------------------------------------------------------- on-device FULL-system assembly (per-realization update)
 * `do_isotropic_elliptic_assembly` / `update_isotropic_elliptic_assembly!(A_mat, b_vec, ..., coeff, f, u_exact)`
 * (Fem/EllipticPde.jl:187-275 / :291-377) when only the nodal coefficient `a` changes: the loop of Examples 06, 09, 12-17,
 * 19 and 20 in front of `pcg(A_t, b_t, 0, Π)`.
 * mi_full_assembly_plan_create: the ROW-OWNED index plan (csrc/full_assembly_plan.hpp), derived here from
 *   cells         3 x nel node indices (row i contiguous), `index_base` 0 or 1;  points  2 x n_node (x row, then y row)
 *   point_marker  n_node, 1 = Dirichlet node; the free nodes, ascending, are the rows of A (`not_dirichlet_inds_g2l`)
 *   n, rowptr, colidx   the CSR pattern the caller holds for A (sorted rows, `index_base`; A is bitwise symmetric, so the CSC
 *                 arrays of Julia's A_mat are the same arrays): it must be the pattern the mesh produces
 *   ue, be        3 x nel, as for mi_assembly_plan_create
 *   The handle is a mi_plan_t: mi_assembly_plan_destroy frees it; mi_assembly_run on it is MI_ERR_BAD_ARG, as is
 *   mi_full_assembly_run on a plan of mi_assembly_plan_create. MI_ERR_BAD_ARG, with a message that names the number, for:
 *   a cell index outside the mesh, an element with a repeated vertex, a zero-area element, a row with more stored entries
 *   than one workgroup's segment (4096), 4 nel >= 2^31, a pattern that is not the mesh's.
 * mi_full_assembly_run: a_nodal (n_node) -> values (nnz(A), CSR order) and b (n); pointers per the context's pointer mode
 *   (device pointers: asynchronous on the context's stream, legal inside a stream capture). One thread owns one row and adds
 *   the contributions of the elements around its node in ascending element number, the order of `sparse(I,J,V)` and
 *   `b[k] +=`: no atomics, bit-identical to the host loop and from run to run.
 * mi_full_assembly_update: the same numbers; the values go straight into the device array of the mi_csr_create operator A
 *   (same context, same pattern: checked in full the first time a plan meets an operator), b per the pointer mode.
 * mi_full_assembly_stats: row blocks, incidences (free element vertices) and the device bytes the plan keeps.
 * mi_csr_set_values: new values (nnz, pointer mode) on the pattern of mi_csr_create, into the same device array: solve
 *   graphs captured for the operator stay valid. MI_ERR_BAD_ARG for any other operator.
 * mi_diag_set_from_csr: dinv[r] = 1.0 / A[r, r] on the device, into the same device array of the mi_diag_create operator M.
 *   MI_ERR_BAD_ARG (M unchanged) if M is the identity or not diagonal, of another size or context than A, or if a row of A
 *   stores no diagonal entry. Synchronous. */
int mi_full_assembly_plan_create(mi_ctx_t ctx, int64_t nel, int64_t n_node, const int64_t *cells, int index_base,
                                 const double *points, const int64_t *point_marker, int64_t n, const int64_t *rowptr,
                                 const int64_t *colidx, const double *ue, const double *be, mi_plan_t *plan);
int mi_full_assembly_run(mi_plan_t plan, const double *a_nodal, double *values, double *b);
int mi_full_assembly_update(mi_plan_t plan, const double *a_nodal, mi_op_t A, double *b);
int mi_full_assembly_update_batch(mi_plan_t plan, const double *a_nodal, mi_op_t batch, int64_t slot, double *b);   /* see mi_csr_batch_* */
int mi_full_assembly_stats(mi_plan_t plan, int64_t *row_blocks, int64_t *incidences, int64_t *bytes_kept);
int mi_csr_set_values(mi_op_t op, const double *val);
int mi_diag_set_from_csr(mi_op_t M, mi_op_t A);
int mi_schur_matfree_set_values(mi_op_t op, const double *ii_val, const double *ig_val, const double *gg_val);
int mi_schur_matfree_rhs(mi_op_t op, const double *b_I, const double *b_gamma, double *b_schur);
/* `get_subdomain_solutions(u_Γ, A_IId, A_IΓd, b_Id)` (EPDD.jl:1014-1025): u_Id = A_IIdd \ (b_Id - A_IΓdd u_Γd) for the
 * operator's subdomains with its own interior solve; b_I and u_I are concatenations over those subdomains. */
int mi_schur_matfree_interior_solutions(mi_op_t op, const double *u_gamma, const double *b_I, double *u_I);

/* ---------------------------------------------------------------- set-up of the assembled mode on the device
 * mi_schur_setup_* — `assemble_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, ...)` (EPDD.jl:667-695): the dense local Schur complements
 * S_d = A_ΓΓdd - A_IΓdd' A_IIdd^{-1} A_IΓdd of ALL subdomains, symmetrised from the upper triangle as the reference does
 * (`Symmetric(Array(...))`, :692), and — optionally — the condensed right-hand sides w_d = A_IΓdd' (A_IIdd \ b_Id) that
 * `get_schur_rhs` subtracts from b_Γ (EPDD.jl:853-861). The reference applies apply_local_schur (interior CG, reltol 1e-9) to
 * every unit vector; here the interior is eliminated exactly, level by level over breadth-first levels grown from Γ_d, with
 * hand-written kernels: Z_k = T_k^{-1} by block Gauss-Jordan WITHOUT pivoting on the fp64 matrix cores (csrc/setup_gj.hpp;
 * every T_k is SPD), one hipGraph replay per realization — a documented deviation that only tightens S_d (measured against
 * the reference's semantics: tests/test_gpu_setup.py::test_device_setup_against_the_reference_semantics). Break-down: an
 * interior block that is singular or not positive definite (the reference's CHOLMOD paths would throw PosDefException)
 * shows as Inf / NaN in S_d: host-pointer mode returns MI_ERR_SINGULAR from run; device-pointer mode is asynchronous and
 * the next mi_nn_pinv on such blocks returns MI_ERR_SINGULAR.
 *   create: the sparsity of the blocks (CSC colptr / rowval as for mi_schur_matfree_device_create), once per mesh / partition
 *   run   : one realization. ii_val / ig_val / gg_val: the concatenations over the subdomains of the blocks' CSC nzval arrays
 *           (the layout mi_assembly_run produces and mi_schur_matfree_set_values takes); b_I: concatenated b_Id or NULL.
 *           Sd receives the concatenated column-major n_Γd x n_Γd blocks, w (may be NULL) the concatenated w_d. Host or
 *           device pointers per the context's pointer mode; with device pointers the call is asynchronous on the stream.
 * mi_nn_pinv — `prepare_neumann_neumann_schur_precond(Sd, ...)` (EPDD.jl:1201-1220): ΠS_d = pinv(S_d, rtol) of the symmetric
 * blocks; rtol <= 0 means sqrt(eps(Float64)), the reference's value. LinearAlgebra.pinv drops the singular values
 * <= rtol * the largest. Three routes, tried in this order per block, all giving that result: (1) 1/||S^{-1}||_inf >
 * rtol ||S||_inf proves that nothing is dropped: the pseudo-inverse is the inverse (the Gauss-Jordan kernels of the set-up),
 * used only if the probe residual ||v - Z S v||_inf <= 4 n eps ||Z||_inf ||S||_inf (v = ±1) shows Z accurate (routes 1, 2);
 * (2) floating subdomains, ||S 1||_inf <= rtol max(max_i |S_ii|, ||S||_inf / sqrt(n)) (lower bounds on the largest singular
 * value, so pinv drops an eigenvalue as well): S^+ = (S + α u u')^{-1} - u u'/α, u = 1/sqrt(n), α = ||S||_inf, the same kernels
 * and the same certificate on the shifted matrix, plus ||S 1||_inf ||(S + α u u')^{-1}||_inf <= rtol (u close to the dropped
 * eigenvector); (3) anything else (rank deficiency > 1, an eigenvalue near the cut-off): eigen-decomposition
 * (rocSOLVER dsyevd, bound with dlopen; singular values = |eigenvalues|). MI_QUERY_SPECTRAL_PINV counts route (3).
 * mi_dense_set_blocks — new blocks (concatenated, column-major) for an existing mi_schur_assembled / mi_nn operator on the same
 * maps: the per-realization update of S (Example07:180-199) without re-creating the operator. */
typedef struct mi_setup_s *mi_setup_t;
int mi_schur_setup_create(mi_ctx_t ctx, int64_t ndom, const int64_t *n_gamma_d, const int64_t *n_i,
                          const int64_t *const *ii_colptr, const int64_t *const *ii_rowval,
                          const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                          const int64_t *const *gg_colptr, const int64_t *const *gg_rowval, int index_base,
                          mi_setup_t *plan);
int mi_schur_setup_run(mi_setup_t plan, const double *ii_val, const double *ig_val, const double *gg_val,
                       const double *b_I, double *Sd, double *w);
/* Level solves — the interior solve of the matrix-free applies as the north-star words it ("the A_II^{-1} interior solve stays
 * ... sparse Cholesky"): EXACT, on the device. mi_schur_setup_keep_levels(plan, 1) makes every following run keep the
 * inverses Z_k of all breadth-first levels (block LDL' of A_IIdd; Σ n_level² doubles — 6.2 GB at config 3); then
 * mi_schur_setup_interior_solve: u = A_IIdd \ f for ALL subdomains at once (f, u: concatenated interior vectors in the order
 * of b_I), a forward and a backward sweep over the kept inverses, one hipGraph replay — in place of the reference's inexact
 * `IterativeSolvers.cg(A_IIdd, rhs; reltol)` (EPDD.jl:609-619, 648-650, 813-815, 1021) and of its thousands of A_II SpMVs.
 * mi_schur_matfree_interior_levels(op, plan): a matrix-free or global Schur operator built on the same subdomains uses
 * these solves for every interior solve (apply, get_schur_rhs, get_subdomain_solutions); plan = NULL restores its own
 * (callback / interior CG). Values are those of the plan's last run. The plan counts the operators bound to it: up here,
 * down when the operator is given plan = NULL or another plan, or is destroyed. While the count is above 0
 * mi_schur_setup_destroy returns MI_ERR_BAD_ARG ("... live matrix-free Schur operator(s) solve with this plan; destroy them
 * first"). mi_schur_setup_keep_levels(plan, 0) is not refused for these users: their next interior solve raises
 * MI_ERR_BAD_ARG ("level solves need ...") until the levels are kept and run again. That is safe because nothing of theirs is
 * captured: a matrix-free Schur operator is never part of a solve graph (its solves run launch by launch), every level solve
 * checks the plan's state before its first launch, and keep_levels(plan, 0) waits for the stream and destroys the plan's own
 * level-solve graph before the level storage goes back to the pool.
 * mi_schur_setup_keep_levels(plan, 0) IS refused (MI_ERR_BAD_ARG, plan unchanged) while a LORASC or a Neumann-Neumann induced
 * operator is bound to the plan ("... live LORASC operator(s) solve with the kept levels", "... live Neumann-Neumann induced
 * operator(s) solve with the kept levels"): their level solves are launches inside captured solve graphs. */
int mi_schur_setup_keep_levels(mi_setup_t plan, int on);
int mi_schur_setup_interior_solve(mi_setup_t plan, const double *f, double *u);
int mi_schur_matfree_interior_levels(mi_op_t op, mi_setup_t plan);
int mi_schur_setup_destroy(mi_setup_t plan);

/* mi_lorasc_create — the reference's `LorascPreconditioner` (EPDD.jl:1406-1428) with `apply_lorasc` (EPDD.jl:1908-1976) as
 * its apply: the M of `pcg(A, b, zeros, ΠA_lorasc)` and `defpcg(A, b, zeros, ϕ, ΠA_lorasc)` on the FULL system
 * (Example03:245-268; Examples 06, 09, 17), n = Σ n_i + n_gamma. With x indexed like the rows of A
 * (`not_dirichlet_inds_g2l`):
 *     y_Id = A_IId \ x_Id;  z_Γ = x_Γ - Σ_d A_IΓd' y_Id  (d ascending)         (EPDD.jl:1935-1942)
 *     x_Γ  = A_ΓΓ \ z_Γ                                                        (EPDD.jl:1950, the Cholesky branch)
 *     x_Γ += Σ_k coef[k] (E[:,k]' z_Γ) E[:,k]                (k ascending)      (EPDD.jl:1954-1957)
 *     u_Id = y_Id - A_IId \ (A_IΓd x_Γ);  u_Γ = x_Γ                             (EPDD.jl:1959-1973)
 * Both solves are exact and already on the device: `interior` is a set-up plan with mi_schur_setup_keep_levels(plan, 1) and
 * a run after it (all A_IId at once), `a_gg_solver` a mi_spd_direct operator of size n_gamma. The operator borrows both:
 * while it is alive, mi_schur_setup_destroy(interior), mi_schur_setup_keep_levels(interior, 0) and
 * mi_op_destroy(a_gg_solver) return MI_ERR_BAD_ARG and change nothing. A later mi_schur_setup_run /
 * mi_spd_direct_set_values moves them, and with them this operator, to a new realization. The apply is plain launches (two
 * level solves, the A_ΓΓ solve, five small kernels), no atomics, fixed summation orders: bitwise reproducible, captured into
 * the solvers' graphs.
 *   create: HOST arrays, `index_base`-based. n_i[d] as in the plan; pos_I[d][i] / pos_gamma[g]: the row of A of interior
 *           node i of subdomain d / of Γ node g (together a permutation of the n rows); ig_*[d]: the CSC arrays of A_IΓd,
 *           n_i[d] x n_gamma with Γ-GLOBAL columns (`prepare_global_schur`, EPDD.jl:212-369); E: n_gamma x nev, column-major
 *           (NULL with nev = 0); nev <= 1024.
 *   coef:   NULL means ones — the reference AS WRITTEN: its loop `for (k, σ) in enumerate(Πlorasc.Σ)` (EPDD.jl:1954) never
 *           uses σ, although prepare_lorasc_precond stores Σ[k] = (ε - σ_k)/σ_k (EPDD.jl:1596) beside A_ΓΓ-orthonormal
 *           E[k]. The correction of Grigori, Nataf and Yousef is coef = Σ.
 *   mi_lorasc_set_values: the concatenated CSC nzval of all A_IΓd for a new realization (host or device pointer per the
 *           context's pointer mode); mi_lorasc_set_correction: new nev, E, coef (same pointer rule; coef NULL: ones).
 * MI_ERR_BAD_ARG with a message: maps that are no permutation, an n_i that differs from the plan's, a plan without kept
 * levels, an a_gg_solver that is no sparse direct operator of size n_gamma, indices out of range, nev above 1024, a context
 * that is one rank of several (the operator is replicated only). The AMG/CG branch of EPDD.jl:1946 is not provided. */
int mi_lorasc_create(mi_ctx_t ctx, int64_t ndom, int64_t n, int64_t n_gamma, const int64_t *n_i,
                     const int64_t *const *pos_I, const int64_t *pos_gamma, const int64_t *const *ig_colptr,
                     const int64_t *const *ig_rowval, const double *const *ig_nzval, mi_setup_t interior,
                     mi_op_t a_gg_solver, int64_t nev, const double *E, const double *coef, int index_base, mi_op_t *op);
int mi_lorasc_set_values(mi_op_t op, const double *ig_val);
int mi_lorasc_set_correction(mi_op_t op, int64_t nev, const double *E, const double *coef);

/* mi_nn_induced_create — the reference's `NeumannNeumannInducedPreconditioner` (EPDD.jl:2274-2285; prepared by
 * `prepare_neumann_neumann_induced_precond`, EPDD.jl:2305-2353) with `apply_neumann_neumann_induced` (EPDD.jl:2363-2423) as
 * its apply: the M of `defpcg(A, b, ϕ, M=ΠA_induced_nn_local_mat)` and `pcg(A, b, M=ΠA_induced_nn_local_mat)` on the FULL
 * system (Example03:300-319), n = Σ n_i + n_gamma. With r indexed like the rows of A (`not_dirichlet_inds_g2l`):
 *     y_Id = A_IId \ r_Id;  r_schur = r_Γ;  r_schur[gather_d] -= A_IΓdd' y_Id  (d ascending)     (EPDD.jl:2393-2400)
 *     z_Γd = ΠS_d (r_schur[gather_d] / cnt[gather_d]);  z_Γ[gather_d] += z_Γd / cnt[gather_d]     (EPDD.jl:2403-2410)
 *     z_Id = A_IId \ (r_Id - A_IΓdd v_d);  z[pos_I[d]] = z_Id;  z[pos_gamma] = z_Γ                (EPDD.jl:2411-2420)
 * `coupling` chooses v_d:
 *   MI_NNI_AS_WRITTEN  v_d = z_Γd, the local, unweighted, unassembled product — EPDD.jl:2411 as the reference has it. The
 *                      operator is then neither symmetric nor positive definite (the reference's own notice: "this
 *                      preconditioner only seems to work with deflation", EPDD.jl:2302).
 *   MI_NNI_ASSEMBLED   v_d = z_Γ[gather_d]: the symmetric positive definite form
 *                      [I -A_II⁻¹A_IΓ; 0 I] diag(A_II⁻¹, M_NN) [I 0; -A_ΓI A_II⁻¹ I].
 * `interior` is a set-up plan with mi_schur_setup_keep_levels(plan, 1) and a run after it (all A_IId \ f at once, exact).
 * The operator borrows it: while it is alive, mi_schur_setup_destroy(interior) and mi_schur_setup_keep_levels(interior, 0)
 * return MI_ERR_BAD_ARG and change nothing. A later mi_schur_setup_run moves the plan, and with it this operator, to a new
 * realization. The ΠS_d blocks are owned, in the layout and storage kinds of mi_nn_create_stored (MI_STORE_F64 /
 * MI_STORE_F32); for the same r_schur the Γ part carries the bits of that operator's apply. The apply is plain launches
 * (two level solves, the batched ΠS_d GEMV, five small kernels), no atomics, fixed summation orders: bitwise reproducible,
 * captured into the solvers' graphs.
 *   create: HOST arrays, `index_base`-based. n_gamma_d[d], n_i[d] as in the plan; pos_I[d][i] / pos_gamma[g]: the row of A
 *           of interior node i of subdomain d / of Γ node g (together a permutation of the n rows); gather_idx[d][l]: the Γ
 *           index of local interface node l (`ind_Γd_Γ2l`); cnt[g]: `node_Γ_cnt`; ig_*[d]: the CSC arrays of A_IΓdd,
 *           n_i[d] x n_gamma_d[d] with LOCAL columns — what the plan itself was created from (EPDD.jl:2278); PiSd[d]:
 *           n_gamma_d[d] x n_gamma_d[d], column-major fp64.
 *   mi_nn_induced_set_values: the concatenated CSC nzval of all A_IΓdd for a new realization; mi_nn_induced_set_blocks: the
 *           new ΠS_d, concatenated column-major fp64 (both: host or device pointer per the context's pointer mode);
 *           mi_nn_induced_set_coupling: the other form of EPDD.jl:2411 on the same operator.
 * MI_ERR_BAD_ARG with a message that names the offending numbers: maps that are no permutation, an index out of range,
 * n != Σ n_i + n_gamma, an n_i or n_gamma_d that differs from the plan's, a plan of another context, a plan without kept
 * levels or with no run since keeping them, a gather_idx outside [0, n_gamma), a cnt[g] that is not the number of
 * subdomains whose gather_idx holds g, an unknown storage or coupling, a context that is one rank of several (the operator
 * is replicated only). */
#define MI_NNI_AS_WRITTEN 0
#define MI_NNI_ASSEMBLED 1
int mi_nn_induced_create(mi_ctx_t ctx, int64_t ndom, int64_t n, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *n_i,
                         const int64_t *const *pos_I, const int64_t *pos_gamma, const int64_t *const *gather_idx,
                         const int64_t *cnt, const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                         const double *const *ig_nzval, const double *const *PiSd, int storage, mi_setup_t interior,
                         int coupling, int index_base, mi_op_t *op);
int mi_nn_induced_set_values(mi_op_t op, const double *ig_val);
int mi_nn_induced_set_blocks(mi_op_t op, const double *PiSd);
int mi_nn_induced_set_coupling(mi_op_t op, int coupling);
int mi_nn_pinv(mi_ctx_t ctx, int64_t ndom, const int64_t *n_gamma_d, const double *Sd, double rtol, double *PiSd);
int mi_dense_set_blocks(mi_op_t op, const double *blocks);

/* ---------------------------------------------------------------- eigCG family and Init-CG (recycling solvers)
 * Reference signatures (RecyclingKrylovSolvers/eigcg.jl:27-33, 143-150; defcg.jl:111-116, 337-343; initcg.jl:28-33,
 * 106-111; callers: Example09_DefPcgMcmcStochasticEllipticPde_Functions.jl:314, 345, 364 on the NN-preconditioned
 * Schur system, with nvec = floor(1.25 ndom), spdim = 3 ndom):
 *     eigcg(A,b,x,nvec,spdim;maxit=0)      eigpcg(A,b,x,M,nvec,spdim;maxit=0)
 *     eigdefcg(A,b,x,W,spdim;maxit=0)      eigdefpcg(A,b,x,M,W,spdim;maxit=0)     -> (x, it, res_norm[1:it], V[:,1:nvec])
 *     initcg(A,b,x,W;maxit=0)              initpcg(A,b,x,M,W;maxit=0)             -> (x, it, res_norm[1:it])
 * x, it, res_norm as for mi_cg & co. V_out receives n x nvec doubles (column-major, host or device pointer like x):
 * the approximate least-dominant eigenvectors of A (of M^{-1}A for the preconditioned kinds) to hand to
 * mi_defpcg / mi_eigdefpcg / mi_initpcg as W for the next system. For the deflated kinds nvec is the column count of W.
 * The iteration runs on the device; at each thick restart (every spdim - nev iterations) the spdim x spdim projected
 * matrix visits the host for the dense eigen/SVD step. V_out is determined up to the sign/rotation of eigenvectors.
 * spdim >= 2 nvec + 1 is required (MI_ERR_BOUNDS otherwise: the reference's `V[:, nev+1]` would be out of bounds);
 * MI_ERR_BOUNDS is also returned — after x, it, res_norm have been written — where the reference's final Ritz
 * extraction indexes out of bounds (a preconditioned solve that ends with exactly nvec search directions).
 * initpcg: the reference's body reads an unallocated `z` (initcg.jl:127, UndefVarError); implemented as documented
 * there (Init-PCG: deflated initial guess, then pcg). */
int mi_eigcg(mi_op_t A, const double *b, double *x, int64_t nvec, int64_t spdim, int64_t maxit, double eps,
             double *res_norm, int64_t res_cap, int64_t *it, double *V_out);
int mi_eigpcg(mi_op_t A, mi_op_t M, const double *b, double *x, int64_t nvec, int64_t spdim, int64_t maxit,
              double eps, double *res_norm, int64_t res_cap, int64_t *it, double *V_out);
int mi_eigdefcg(mi_op_t A, const double *b, double *x, const double *W, int64_t nvec, int64_t spdim, int64_t maxit,
                double eps, double *res_norm, int64_t res_cap, int64_t *it, double *V_out);
int mi_eigdefpcg(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t spdim,
                 int64_t maxit, double eps, double *res_norm, int64_t res_cap, int64_t *it, double *V_out);
int mi_initcg(mi_op_t A, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit, double eps,
              double *res_norm, int64_t res_cap, int64_t *it);
int mi_initpcg(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit,
               double eps, double *res_norm, int64_t res_cap, int64_t *it);

/* ---------------------------------------------------------------- eigensolver (thick-restart Lanczos on the device)
 * mi_eigsolve — the reference's calls for extremal eigenpairs of its operators:
 *     KrylovKit.eigsolve(x -> S_local_mat*x, n_Γ, nev, :SR | :LR, krylovdim=2*nev)   (Example03:209/219: the `ld` / `md`
 *         deflation bases W of `defpcg(S, b, 0, W, ΠSnn)`)                                          -> B = Binv = NULL
 *     KrylovKit.geneigsolve(x -> (S*x, A_ΓΓ*x), n_Γ, nvec, :SR, krylovdim=2*nvec, isposdef=true)  (EPDD.jl:1546-1549: the
 *         LORASC pairs that mi_lorasc_set_correction takes)                -> B = A_ΓΓ (mi_csr), Binv = mi_spd_direct of it
 *     Arpack.eigs(A | S, nev, :SM)  (Example03:260/291/313; Example07:246, 494)   -> the LR pairs of an exact inverse
 *         operator (mi_block_jacobi_create with nb = 1 is `A \ b`), λ = 1/θ; :LM is MI_EIG_LR on the operator itself.
 * For a symmetric operator KrylovKit's Krylov-Schur method is thick-restart Lanczos; here with full re-orthogonalisation
 * (classical Gram-Schmidt twice) of every new vector against the whole window, the window and the re-orthogonalisation on
 * the device, one hipGraph replay and one host synchronisation per restart (csrc/lanczos.hpp has the algorithm).
 *   A        symmetric operator; B (SPD) and Binv (B^-1, exact) select the generalized problem A x = λ B x, Lanczos on
 *            B^-1 A in the B inner product: the returned vectors satisfy X' B X = I (X' X = I for the standard problem).
 *   which    MI_EIG_SR: the nev smallest eigenvalues, ascending; MI_EIG_LR: the nev largest, descending.
 *   krylovdim  columns of the window; 0 means max(2 nev, 8); clamped to n (then one window is exact and no restart is made).
 *   tol      ABSOLUTE bar on the residual estimate |beta Y[m, i]| of a Ritz pair, as KrylovKit's `tol`.
 *   maxiter  restarts allowed. Running out of them is no error (KrylovKit's `info.converged` convention): MI_OK with
 *            *nconv < nev, and vals / vecs / resid the current Ritz pairs.
 *   v0       start vector, n entries (host or device pointer like vecs), or NULL: a fixed seeded vector.
 *   vals (nev), resid (nev, may be NULL): HOST arrays; vecs: n x nev, column-major, host or device pointer per the context's
 *            pointer mode. nconv: leading pairs with resid <= tol (at most nev); nrestart; napply: applies of A (each of
 *            nconv / nrestart / napply may be NULL).
 * A basis that becomes invariant (beta <= 64 eps max|T|) ends the call with the exact pairs of that subspace when it holds
 * nev columns, and is continued with a fresh orthogonalised vector otherwise.
 * MI_ERR_BAD_ARG with a message: nev < 1 or nev > n; which unknown; krylovdim negative, or below nev + 1 without reaching n;
 * a window above 1024 columns; tol or maxiter negative; exactly one of B / Binv; operators of different size or context;
 * a context that is one rank of several (sharded eigensolves are not provided).
 * MI_ERR_SINGULAR: a start vector that is zero or not finite, or a beta / T entry that is not finite (NaN or Inf from an
 * operator). Nothing is carried from one call to the next: all buffers of a call are its own. */
#define MI_EIG_SR 0
#define MI_EIG_LR 1
int mi_eigsolve(mi_op_t A, mi_op_t B /*NULL: standard*/, mi_op_t Binv /*NULL iff B is*/,
                int64_t nev, int which, int64_t krylovdim /*0: max(2*nev, 8)*/, double tol, int64_t maxiter,
                const double *v0 /*NULL: seeded host vector*/, double *vals /*nev*/, double *vecs /*n x nev, col-major*/,
                double *resid /*nev, may be NULL*/, int64_t *nconv, int64_t *nrestart, int64_t *napply);

/* ---------------------------------------------------------------- Karhunen-Loève: matrix-free covariance operators
 * The reference's KL layer (Fem/KarhunenLoeve.jl, Fem/KarhunenLoeveDomainDecomposition.jl = "KLDD.jl", Fem/Covariances.jl)
 * assembles the dense Galerkin matrix C[i, j] = ∫∫ ϕ_i(P) cov(P, P') ϕ_j(P') by two O(nnode nel) element loops and hands it to
 * `Arpack.eigs(C, M)`. The first loop builds R = M K, the second C = R M (KarhunenLoeve.jl:40-105), with M the consistent P1
 * mass matrix and K[i, j] = cov(p_i, p_j) the nodal covariance: C = M K M, and K is applied on the fly (csrc/cov_kernels.hpp)
 * instead of being stored.
 * Covariance models: MI_COV_SEXP, c = sig2 exp(-((x1 - x2)² + (y1 - y2)²) / L²) (`cov_sexp`, Covariances.jl:23-28);
 * MI_COV_EXP, c = sig2 exp(-sqrt((x1 - x2)² + (y1 - y2)²) / L), the "Exp" of get_root_filename
 * (KarhunenLoeveDomainDecompositionHelper.jl:54). The exponent is evaluated as written there (a true division).
 *
 * mi_cov_apply — Y[0:nt, 0:m] = Σ_j c(pt[:, i], ps[:, j]) X[j, 0:m]: the `cov(x[r], y[r], xj, yj)` evaluations of
 *   KarhunenLoeve.jl:75-77, KLDD.jl:171-173 and of the rectangular (idom, jdom) loop KLDD.jl:508-547, applied to a panel.
 *   pt (2 x nt) and ps (2 x ns) in the reference's `points` layout (x and y of a node adjacent); X column-major with ldx >= ns,
 *   Y column-major with ldy >= nt; only rows [0, ns) resp. [0, nt) of a column are read resp. written. All four pointers follow
 *   the context's pointer mode; either way the call returns when Y is complete (its workspace is its own and is handed back
 *   before it returns; the capture-safe form is the operator below). pt == ps is allowed, Y must not
 *   overlap X. Sources are split over workgroups when the targets alone do not fill the device; partial sums are added in a
 *   fixed order (no atomics): equal calls give equal bits.
 * mi_cov_tiling — the tiling mi_cov_apply uses for these sizes, a pure host function (no device, no context): target rows per
 *   workgroup, sources per LDS chunk, columns per thread, and the number of source splits (a function of nt, ns, m only).
 *   Any output pointer may be NULL.
 * mi_kl_cov_create — the operator x -> C x = M (K (M x)) on the n nodes `points` (2 x n): what do_mass_covariance_assembly
 *   (KarhunenLoeve.jl:27-108) and do_local_mass_covariance_assembly (KLDD.jl:120-204) return, as the `A` of
 *   mi_eigsolve(C, B = M, Binv = M^-1, MI_EIG_LR) — `Arpack.eigs(C, M, nev=nev)` (KarhunenLoeve.jl:138, KLDD.jl:679); the vectors
 *   come back with Φ' M Φ = I, the normalisation of KarhunenLoeve.jl:183-185. m_rowptr / m_colidx / m_val: CSR (= CSC) arrays
 *   of the symmetric n x n mass matrix (get_mass_matrix, EllipticPde.jl:412-466; do_local_mass_assembly, KLDD.jl:236-293),
 *   0-based HOST arrays like `points`. One apply is SpMV, covariance launch (+ its reduction), SpMV; all workspace is allocated
 *   here, the apply neither allocates nor synchronises (it is replayed inside the eigensolver's graphs). mi_op_bytes names the
 *   covariance launch as the dominant kernel (32 n bytes of points, as targets and as sources, + 16 n of vectors; it is compute bound: n² exp), and
 *   mi_op_apply_dominant / mi_op_time_dominant launch it.
 * MI_ERR_BAD_ARG with a mi_last_error() text, nothing written: an unknown model; L <= 0, sig2 < 0 or either not finite; points
 *   that are not finite (host arrays); nt, ns or m < 1 (or above 2^30); ldx < ns or ldy < nt; a NULL pointer; a CSR matrix that
 *   is not n x n; a context that is one rank of several (sharded KL operators are not provided). */
#define MI_COV_SEXP 0
#define MI_COV_EXP 1
int mi_cov_apply(mi_ctx_t ctx, int model, double sig2, double L, int64_t nt, const double *pt, int64_t ns, const double *ps,
                 int64_t m, const double *X, int64_t ldx, double *Y, int64_t ldy);
int mi_cov_tiling(int64_t nt, int64_t ns, int64_t m, int64_t *row_tile, int64_t *src_chunk, int64_t *col_block, int64_t *splits);
int mi_kl_cov_create(mi_ctx_t ctx, int model, double sig2, double L, int64_t n, const double *points, const int64_t *m_rowptr,
                     const int64_t *m_colidx, const double *m_val, mi_op_t *op);

/* ---------------------------------------------------------------- realization sampler: latent vector -> field -> coefficient
 * The step between the KL modes and the per-realization update (mi_assembly_run, mi_schur_setup_run, mi_amg_set_values): from a
 * latent vector ξ to g = Σ_α sqrt(Λ_α) ξ_α Ψ[:, α] and a = exp(g), on the device (csrc/kl_field.hpp). It is the field half of
 * `draw!(Λ, Ψ, ξ, g)` (KLDD.jl:1026-1044; the loop :1037-1040), of `set!(Λ, Ψ, ξ, g)` (KLDD.jl:1150-1164) and of the samplers'
 * `draw!` / `set!` (Fem/Samplers.jl:62-87, 165-199); the random numbers stay with the caller (m per draw).
 *
 * mi_kl_field_create — the dense form on Ψ (n x m, column-major, ldpsi >= n) and Λ (m): HOST arrays, copied to the device once.
 * mi_kl_field_create_dd — the factored form of `draw(mesh, Λ, Φ, Φd, inds_l2gd)` (KLDD.jl:850-883), which never forms Ψ:
 *   g_i = (1 / cnt_i) Σ_{d ∋ i} Σ_α Φd[d][l, α] (Φ c)[off_d + α], c_γ = sqrt(Λ_γ) ξ_γ. n_d[d] nodes and md[d] local modes per
 *   subdomain; inds_l2gd: the ndom local-to-global maps concatenated (Σ n_d entries, `index_base` 0 or 1); Phid: the ndom
 *   column-major n_d x md_d blocks concatenated; Phi: (Σ md) x m column-major with ldphi >= Σ md. HOST arrays. It keeps
 *   Σ n_d md_d + m Σ md numbers instead of n m. The sums run in a fixed order of their own (γ ascending, α ascending, owners in
 *   ascending d, a true division by cnt_i), not in the reference's (idom, α, γ) nest: equal to it within rounding, not in bits.
 * mi_kl_field_set — G[:, r] = field of the latent vector Ξ[:, r], A[:, r] = exp(G[:, r]), r < nreal. Ξ is m x nreal with
 *   ldxi >= m, G and A are n x nreal with ldg, lda >= n, all column-major; either of G and A may be NULL, not both; only rows
 *   [0, m) resp. [0, n) of a column are read resp. written. The three pointers follow the context's pointer mode. With device
 *   pointers the call only enqueues kernels on the context's stream (all workspace was allocated at creation: no allocation, no
 *   synchronisation, legal inside a stream capture), so it can stand directly in front of mi_assembly_run; with host pointers it
 *   returns when G and A are complete. Up to 8 realizations share one pass over the modes; more run in blocks of 8.
 *   Dense form: the modes are summed in ascending α, each term as acc + (sqrt(Λ_α) ξ_α) Ψ_iα (product, then sum, from +0), never
 *   split: every column of G has the bits of the host loop, whatever nreal. exp is the device library's (1 ulp). No atomics:
 *   equal calls give equal bits. A non-finite ξ is not an error (IEEE results).
 * mi_kl_field_coords — `get_kl_coordinates(g, Λ, Ψ, M)` (KLDD.jl:1109-1124): ξ_α = (Σ_i Ψ[i, α] (M g)[i]) / sqrt(Λ_α). M is a
 *   mi_csr_create operator (n x n, same context); g (n) and xi (m) follow the pointer mode; device pointers: asynchronous, no
 *   allocation. The column sums are split over row blocks (a function of n and m only) and the partial sums added in ascending
 *   order; the sum is divided once (the reference divides every term: a rounding difference). Dense form only, and m <= 524 280 (65 535 blocks of 8 modes).
 * mi_kl_field_tiling — pure host function: nodes per workgroup, modes per LDS chunk, realizations per pass, and the number of
 *   row splits of the coordinates launch for these sizes. Any output pointer may be NULL.
 * mi_kl_field_stats — bytes the handle keeps on the device (without workspace), and the bytes one set of one realization with
 *   one output streams.
 * MI_ERR_BAD_ARG with a mi_last_error() text, nothing written: n, m or nreal < 1 (or above 2^30); a leading dimension below its
 *   row count; a NULL required pointer, or G and A both NULL; a Λ_α that is negative or not finite (the reference's sqrt would
 *   throw); Λ_α == 0 in mi_kl_field_coords only; md_d < 1 or n_d < 1; an index outside [0, n) after the base shift; a node
 *   repeated within one subdomain; a node owned by no subdomain (the reference would divide by cnt = 0); an M that is not an
 *   n x n sparse matrix; coordinates of a factored handle or of more than 524 280 modes; a context that is one rank of several. */
typedef struct mi_kl_field_s *mi_kl_field_t;
int mi_kl_field_create(mi_ctx_t ctx, int64_t n, int64_t m, const double *lambda, const double *Psi, int64_t ldpsi, mi_kl_field_t *field);
int mi_kl_field_create_dd(mi_ctx_t ctx, int64_t n, int64_t m, const double *lambda, int64_t ndom, const int64_t *n_d, const int64_t *md,
                          const int64_t *inds_l2gd, int index_base, const double *Phid, const double *Phi, int64_t ldphi,
                          mi_kl_field_t *field);
int mi_kl_field_set(mi_kl_field_t field, int64_t nreal, const double *Xi, int64_t ldxi, double *G, int64_t ldg, double *A, int64_t lda);
int mi_kl_field_coords(mi_kl_field_t field, mi_op_t M, const double *g, double *xi);
int mi_kl_field_tiling(int64_t n, int64_t m, int64_t nreal, int64_t *row_tile, int64_t *mode_chunk, int64_t *real_block,
                       int64_t *coord_splits);
int mi_kl_field_stats(mi_kl_field_t field, int64_t *bytes_kept, int64_t *bytes_per_set);
int mi_kl_field_destroy(mi_kl_field_t field);

/* ---------------------------------------------------------------- vector quantization of ξ and the operators it selects
 * The reference's quantization studies (Examples 12-14, 18, 20) cluster draws of ξ into a Voronoi quantizer with
 * `kmeans(X, P, tol=1e-8, maxiter=1_000)` (Clustering.jl; Example20_QuantizedPreconditioner_Functions.jl:56-73 = "Ex20F",
 * Example12_Quantization_Functions.jl:29-59 = "Ex12F", Example13_CLVQ_Functions.jl:129-159 = "Ex13F"), build one constant
 * preconditioner per centroid and solve every realization with the nearest one (`find_precond`, Ex20F:39-54; the loop of
 * test_solver_with_centroidal_preconds, Ex12F:147-155) or with a Shepard combination of a few
 * (Example14_QuantizationAndShepardLocalInterpolation_Functions.jl:73-113, 174-206 = "Ex14F"). Kernels: csrc/vq.hpp.
 * X is d x ns (a sample per column, ldx >= d), C is d x P (a centroid per column, ldc >= d), column-major as Julia passes them;
 * rows past d of a column are neither read nor written. Indices are 0-based int64_t. Array pointers (X, C, assign, dist2,
 * counts, u, picked) follow the context's pointer mode; objv, iters and converged are HOST pointers. Every call returns when
 * its outputs are complete (its workspace is its own). No float atomics, fixed orders: equal calls give equal bits.
 *
 * mi_vq_tiling — pure host function (no device, no context): points per workgroup, centroids staged at a time, coordinates per
 *   LDS chunk, the number of centroid splits mi_vq_assign uses for these sizes, and the chunk of the ordered sums. Any output
 *   pointer may be NULL.
 * mi_vq_assign — for every column of X the nearest centroid and its squared distance: the scan of find_precond (Ex20F:44-52),
 *   of get_distortion (Ex13F:53-69) and of clvq's competitive phase (Ex13F:77-85) for ns samples at once. dist2[s] carries the
 *   bits of the reference's `(x .- c)' * (x .- c)` as a loop (t = x_k - c_k; acc = acc + t * t; k ascending from +0); the winner
 *   is the smallest dist2, among equals the lowest p (the strict `<` scan, started at centroid 0 as the reference starts it: a
 *   NaN distance to centroid 0 stays, a NaN distance to another centroid never wins). objv = Σ_s dist2[s] in the chunked order:
 *   sum_chunk consecutive samples ascending from +0, then the chunk totals ascending (get_distortion's w2 is objv / ns). assign,
 *   dist2 and objv may each be NULL. P > ns is allowed.
 * mi_vq_update — Lloyd's centre update for the assignments `assign`: counts[p] members; C[:, p] = (Σ X[:, s] over the members
 *   in ascending s, from +0) / counts[p], a true division — the bits of `for s: sum[:, a[s]] += X[:, s]`. A cluster without a
 *   member keeps its centre bit for bit and has count 0 (Clustering.jl repicks such a centre at random: a deviation).
 * mi_vq_seed — k-means++ (Clustering.jl's default `init`) on P uniforms u[j] in [0, 1) drawn by the caller: centre 0 is sample
 *   floor(u[0] ns); for j >= 1, mind[s] = min(mind[s], dist2(x_s, c_{j-1})), prefix(s) = (ascending sum of the totals of the
 *   earlier chunks) + (ascending sum within the chunk of s up to and including s), total = prefix(ns - 1), and the pick is the
 *   smallest s with prefix(s) > u[j] total (where rounding leaves none: the smallest s with prefix(s) >= total). picked (P
 *   sample indices) and C (the P centres) are written. total == 0 — fewer distinct points than centres — is MI_ERR_BAD_ARG.
 * mi_vq_kmeans — Lloyd's algorithm from the initial centres in C:
 *     a, c = assign(X, C); objv = Σc; t = 0; converged = false
 *     while !converged && t < maxiter:
 *         t += 1; C = update(X, a, C); a, c = assign(X, C); prev = objv; objv = Σc; converged = |objv - prev| < tol
 *   with one 8-byte readback per iteration. assign, counts, dist2 (arrays, may be NULL) and objv, iters, converged (host, may be
 *   NULL) describe the final state. A non-finite objective after the first assignment is MI_ERR_BAD_ARG and C is untouched.
 * mi_op_combine — z = Σ_i coef[i] (ops[i] applied to r), i ascending: `InterpolatingPreconditioner` / apply_local_interpolation
 *   (Ex14F:73-97; the coefficients of shepard_interpolating_precond, Ex14F:174-206). 1 <= k <= 16 operators of this context and
 *   of one size; coef: k finite HOST numbers. The children stay the caller's and the combination borrows them: every place a
 *   child holds in `ops` (of this and of any other live combination) is counted, and while the count is above 0
 *   mi_op_destroy(child) returns MI_ERR_BAD_ARG ("... among the children of live combined operator(s) (mi_op_combine);
 *   destroy them first") and changes nothing. Destroying the combination releases its places and leaves the children usable.
 *   A refresh of a child that changes the arguments of its launches (mi_lorasc_set_correction, mi_nn_induced_set_coupling)
 *   also drops the solve graphs captured with a combination that holds it, at any depth; refreshes into the same device
 *   arrays (every *_set_values, mi_dense_set_blocks, a re-run of a bound plan) need not and do not.
 *   apply runs child i into the i-th temporary, then one kernel forms z = z + coef[i] * t_i
 *   from z = +0 (product, then sum); it honours the solvers' `done` word, allocates nothing, and is captured into the solve
 *   graphs of mi_pcg, mi_defpcg and the eigCG family iff every child can be.
 * mi_op_combine_set_coefficients — new coefficients (k finite HOST numbers) into the same device array: a captured graph keeps
 *   working.
 * MI_ERR_BAD_ARG with a mi_last_error() text, nothing written: d, ns or P < 1; ns or P >= 2^31; P > ns in mi_vq_kmeans and
 *   mi_vq_seed; a leading dimension below d; a NULL required pointer; an assignment outside [0, P) (mi_vq_update); a negative
 *   or non-finite tol, maxiter < 0; a context that is one rank of several; k outside [1, 16], operators of different sizes or
 *   contexts, a coefficient that is not finite. */
int mi_vq_tiling(int64_t d, int64_t ns, int64_t P, int64_t *point_tile, int64_t *cent_tile, int64_t *k_chunk,
                 int64_t *cent_splits, int64_t *sum_chunk);
int mi_vq_assign(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, const double *C, int64_t ldc,
                 int64_t *assign /*NULL ok*/, double *dist2 /*NULL ok*/, double *objv /*NULL ok; host*/);
int mi_vq_update(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, const int64_t *assign, double *C,
                 int64_t ldc, int64_t *counts);
int mi_vq_seed(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, const double *u, int64_t *picked,
               double *C, int64_t ldc);
int mi_vq_kmeans(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, double *C /*in: initial, out: final*/,
                 int64_t ldc, double tol, int64_t maxiter, int64_t *assign, int64_t *counts, double *dist2, double *objv,
                 int64_t *iters, int *converged);
int mi_op_combine(mi_ctx_t ctx, int64_t k, const mi_op_t *ops, const double *coef, mi_op_t *op);
int mi_op_combine_set_coefficients(mi_op_t op, const double *coef);

/* ---------------------------------------------------------------- timing on the context's stream */
int mi_event_create(mi_event_t *ev);
int mi_event_record(mi_ctx_t ctx, mi_event_t ev);
int mi_event_elapsed_ms(mi_event_t start, mi_event_t stop, double *ms); /* synchronises on stop */
int mi_event_destroy(mi_event_t ev);

#ifdef __cplusplus
}
#endif
#endif /* MI355SCHUR_H */
