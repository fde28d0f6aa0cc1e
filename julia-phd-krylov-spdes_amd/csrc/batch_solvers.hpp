// pcg / cg for k independent systems in ONE Krylov loop (mi_pcg_batch): the realizations of a Monte-Carlo study share every
// launch. System t is the grid's second dimension; its matrix is slot sel[1 + t] of a CsrBatchOp (csr_batch.hpp), its
// preconditioner member bsel[1 + t] of an AMG bank view (AmgBankView::apply_batch), its scalars st[t], its vectors, partials
// and residual norms column t of the BatchWorkspace.
//
// There is one form: the arithmetic of the GENERIC loop of solvers.hpp. The x-grids are the single solve's (vec_grid(n) for
// the vector kernels, ((nblocks + 7) / 8) * 8 for the SpMV), so every partial sum, sum_partials, krylov_beta, krylov_stop,
// krylov_count and krylov_start_one run in the single solve's order: x, it and res_norm of system t carry the bits of
//   pcg(A_t, b_t, x0_t, view.select(member_t))
// in its GENERIC form. The kernels are the batched forms of k_solve_begin, k_spmv_csr<0, DOT> (the row sums through
// amg_block_rows, the same products and the same left-to-right order), k_residual, k_init_state, k_init_p, k_update_xr,
// k_dot_partial, k_update_p and k_solve_end; M == NULL gives cg's recurrences (precond = 0, z is r).
//
// k, the slots and the members are read from small device arrays which the entry kernel writes, the grid's second dimension
// is BATCH_MAX and terms t >= k return at once: one captured graph serves every later selection. A system whose stop rule
// has fired is frozen: every later launch returns for it after reading st[t].done, so its x, it and res_norm are those of
// the reference's `while (it < maxit) && (res_norm[it] > tol)`. `active` counts the systems still iterating (an integer
// atomic, decremented by the one thread that raises a system's flag); the host stops replaying when it reads 0.
//
// Replay policy: that of Krylov::solve without the whole-solve entry — the entry kernel, then one graph with the set-up and
// as many iterations as the longest system of the previous batch on this (A, M) needed, the exit kernel behind it; if
// systems are still active, chunk-sized replays with one replay of run-ahead.
#pragma once
#include "amg_bank.hpp"
#include "csr_batch.hpp"
#include "solvers.hpp"

namespace mi {

constexpr int BATCH_GRAPH_TAG = 1 << 12;   // GraphKey::tag of the batched loop's graphs (the single loop's tags stay below)
static_assert(BATCH_MAX == AMGB_MAX_TERMS, "one term of a bank view per system");

struct BatchSel { int k; int slot[BATCH_MAX]; int member[BATCH_MAX]; };

// in: B, X0 -> workspace; eps / maxit / res_cap -> the state blocks; the selections -> sel (slots), msel (members, or NULL); active = k
__global__ __launch_bounds__(NT) void k_bsolve_begin(int n, BatchSel q, const double *__restrict__ B, long long ldb, const double *__restrict__ X,
                                                     long long ldx, double *__restrict__ b0, double *__restrict__ x0, long long vs, SolverState *st0,
                                                     double eps, long long maxit, long long res_cap, int *sel, int *msel, int *active) {
  const int t = (int)blockIdx.y;
  if (blockIdx.x == 0 && t == 0 && (int)threadIdx.x <= q.k) {
    const int i = (int)threadIdx.x;
    if (i == 0) { sel[0] = q.k; if (msel) msel[0] = q.k; *active = q.k; }
    else { sel[i] = q.slot[i - 1]; if (msel) msel[i] = q.member[i - 1]; }
  }
  if (t >= q.k) return;
  const double *b_in = B + (size_t)t * ldb, *x_in = X + (size_t)t * ldx;
  double *b = b0 + (size_t)t * vs, *x = x0 + (size_t)t * vs;
  SolverState *st = st0 + t;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) { b[i] = b_in[i]; x[i] = x_in[i]; }
  if (blockIdx.x == 0 && threadIdx.x == 0) { st->eps = eps; st->maxit = maxit; st->res_cap = res_cap; st->done = 0; st->x0_zero = 0; }
}

// y_t = A_t x_t; DOT: also part_t[b] = Σ_{rows of block b} w_t[r] * y_t[r]. The products, row sums and the block's partial of k_spmv_csr<0, DOT>.
template <bool DOT>
__global__ __launch_bounds__(NT) void k_bspmv(int nblocks, const SpmvBlock *__restrict__ blk, const int *__restrict__ rowptr, const int *__restrict__ col,
                                              const double *__restrict__ slab, long long stride, const int *__restrict__ sel,
                                              const double *__restrict__ x0, double *__restrict__ y0, const double *__restrict__ w0, long long vs,
                                              double *__restrict__ part0, long long dps, const SolverState *st0) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  if (st0 && st0[t].done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  __shared__ double sm[NT / 64 + 1];
  const int per = (nblocks + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (b >= nblocks) return;
  const double *val = slab + (size_t)sel[1 + t] * (size_t)stride, *x = x0 + (size_t)t * vs;
  const double *w = DOT ? w0 + (size_t)t * vs : nullptr;
  double *y = y0 + (size_t)t * vs;
  double wy = 0.0;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return x[c]; }, [&](int i, double s) {
    y[i] = s;
    if (DOT) wy += w[i] * s;
  });
  if (DOT) {
    wy = block_sum(wy, sm);
    if (threadIdx.x == 0) part0[(size_t)t * dps + b] = wy;
  }
}

// r = b - Ap; partial r'r and b'b (k_residual)
__global__ __launch_bounds__(NT) void k_bresidual(int n, const int *__restrict__ sel, const double *__restrict__ b0, const double *__restrict__ Ap0,
                                                  double *__restrict__ r0, long long vs, double *__restrict__ part_rr, double *__restrict__ part_bb) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  __shared__ double sm[NT / 64 + 1];
  const double *b = b0 + (size_t)t * vs, *Ap = Ap0 + (size_t)t * vs;
  double *r = r0 + (size_t)t * vs;
  double srr = 0.0, sbb = 0.0;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    const double bi = b[i];
    const double ri = bi - Ap[i];
    r[i] = ri;
    srr += ri * ri;
    sbb += bi * bi;
  }
  srr = block_sum(srr, sm);
  sbb = block_sum(sbb, sm);
  if (threadIdx.x == 0) {
    part_rr[(size_t)t * MAX_PARTS + blockIdx.x] = srr;
    part_bb[(size_t)t * MAX_PARTS + blockIdx.x] = sbb;
  }
}

// it = 1; res_norm[1]; tol; the stop rule (k_init_state). A system that stops here leaves the count of active systems.
__global__ __launch_bounds__(NT) void k_binit_state(SolverState *st0, const int *__restrict__ sel, const double *part_rr, const double *part_bb,
                                                    const double *part_rz, int g, double *res_norm0, long long rs, int *active) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  __shared__ double sm[NT / 64 + 1];
  SolverState *st = st0 + t;
  const double eps = st->eps;
  const long long maxit = st->maxit, res_cap = st->res_cap;
  const double rr = sum_partials(part_rr + (size_t)t * MAX_PARTS, g, sm);
  const double bb = sum_partials(part_bb + (size_t)t * MAX_PARTS, g, sm);
  const double rz = part_rz ? sum_partials(part_rz + (size_t)t * MAX_PARTS, g, sm) : rr;
  if (threadIdx.x == 0) {
    st->rTr = rr; st->bnorm = sqrt(bb);
    krylov_start_one(st, res_norm0 + (size_t)t * rs, rr, rz, eps * st->bnorm, maxit, res_cap);
    if (st->done) atomicSub(active, 1);
  }
}

// p = z (k_init_p without deflation)
__global__ __launch_bounds__(NT) void k_binit_p(int n, const int *__restrict__ sel, const double *__restrict__ z0, double *__restrict__ p0, long long vs) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  const double *z = z0 + (size_t)t * vs;
  double *p = p0 + (size_t)t * vs;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) p[i] = z[i];
}

// d = p'Ap (from the SpMV's partials); alpha = num / d; x += alpha p; r -= alpha Ap; partial r'r (k_update_xr with a non-diagonal or no M)
__global__ __launch_bounds__(NT) void k_bupdate_xr(int n, const int *__restrict__ sel, SolverState *st0, const double *part_pAp0, long long dps, int g_in,
                                                   const double *__restrict__ p0, const double *__restrict__ Ap0, double *__restrict__ x0,
                                                   double *__restrict__ r0, long long vs, double *__restrict__ part_rr0, int precond) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  SolverState *st = st0 + t;
  if (st->done) return;
  __shared__ double sm[NT / 64 + 1];
  const double *p = p0 + (size_t)t * vs, *Ap = Ap0 + (size_t)t * vs;
  double *x = x0 + (size_t)t * vs, *r = r0 + (size_t)t * vs;
  const int stride = gridDim.x * NT;
  int i0 = blockIdx.x * NT + threadIdx.x;
  double pv[4], xv[4], rv[4], av[4];
  auto load = [&](int base) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + k * stride;
      const bool ok = i < n;
      pv[k] = ok ? p[i] : 0.0; xv[k] = ok ? x[i] : 0.0; rv[k] = ok ? r[i] : 0.0; av[k] = ok ? Ap[i] : 0.0;
    }
  };
  load(i0);
  const double d = sum_partials(part_pAp0 + (size_t)t * dps, g_in, sm);
  const double num = precond ? st->rTz : st->rTr;
  const double alpha = num / d;
  double srr = 0.0;
  for (;;) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k * stride;
      if (i < n) {
        x[i] = xv[k] + alpha * pv[k];                // axpy!(alpha, p, x)
        const double ri = rv[k] + (-alpha) * av[k];  // axpy!(-alpha, Ap, r)
        r[i] = ri;
        srr += ri * ri;
      }
    }
    i0 += 4 * stride;
    if (i0 >= n) break;
    load(i0);
  }
  srr = block_sum(srr, sm);
  if (threadIdx.x == 0) {
    part_rr0[(size_t)t * MAX_PARTS + blockIdx.x] = srr;
    if (blockIdx.x == 0) {
      st->d = d; st->alpha = alpha;
      st->rTr_prev = st->rTr; st->rTz_prev = st->rTz;
    }
  }
}

// partial x'y (k_dot_partial)
__global__ __launch_bounds__(NT) void k_bdot_partial(int n, const int *__restrict__ sel, const double *__restrict__ x0, const double *__restrict__ y0,
                                                     long long vs, double *__restrict__ part0, const SolverState *st0) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  if (st0 && st0[t].done) return;
  __shared__ double sm[NT / 64 + 1];
  const double *x = x0 + (size_t)t * vs, *y = y0 + (size_t)t * vs;
  double s = 0.0;
  const int stride = gridDim.x * NT;
  for (int i0 = blockIdx.x * NT + threadIdx.x; i0 < n; i0 += 4 * stride) {
    double a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k * stride;
      a[k] = i < n ? x[i] : 0.0;
      b[k] = i < n ? y[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k * stride < n) s += a[k] * b[k];
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) part0[(size_t)t * MAX_PARTS + blockIdx.x] = s;
}

// r'r, r'z from partials; beta; p = beta p + z; it += 1; res_norm[it]; the stop rule (k_update_p without deflation). The thread
// that raises a system's flag takes it out of the count of active systems.
__global__ __launch_bounds__(NT) void k_bupdate_p(int n, const int *__restrict__ sel, SolverState *st0, const double *part_rr0, const double *part_rz0,
                                                  int g_in, const double *__restrict__ z0, double *__restrict__ p0, long long vs, double *res_norm0,
                                                  long long rs, int precond, int *active) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  SolverState *st = st0 + t;
  __shared__ double sm[NT / 64 + 1];
  __shared__ int was_done;  // thread 0 of workgroup 0 sets st->done below: take one uniform snapshot
  if (threadIdx.x == 0) was_done = st->done;
  __syncthreads();
  if (was_done) return;
  const double *z = z0 + (size_t)t * vs;
  double *p = p0 + (size_t)t * vs;
  const int stride = gridDim.x * NT;
  int i0 = blockIdx.x * NT + threadIdx.x;
  double pv[4], zv[4];
  auto load = [&](int base) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + k * stride;
      pv[k] = i < n ? p[i] : 0.0;
      zv[k] = i < n ? z[i] : 0.0;
    }
  };
  load(i0);
  const double rr = sum_partials(part_rr0 + (size_t)t * MAX_PARTS, g_in, sm);
  const double rz = precond ? sum_partials(part_rz0 + (size_t)t * MAX_PARTS, g_in, sm) : rr;
  const double old = precond ? st->rTz_prev : st->rTr_prev;
  const double beta = krylov_beta(old, rz);
  for (;;) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k * stride;
      if (i < n) p[i] = beta * pv[k] + zv[k];     // axpby!(1, z, beta, p)
    }
    i0 += 4 * stride;
    if (i0 >= n) break;
    load(i0);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->rTr = rr; st->rTz = rz; st->beta = beta;
    const long long it = st->it + 1;
    const double res = sqrt(rr);
    const StopRule sr = krylov_stop(it, st->maxit, st->res_cap, res, st->tol);
    krylov_count(st, res_norm0 + (size_t)t * rs, it, res, sr);
    if (sr.stop) atomicSub(active, 1);
  }
}

// out: x_t -> X[:, t]; it / done / overflow of every system, the count of active systems and the first min(it, ncap) residual norms -> pinned memory
__global__ __launch_bounds__(NT) void k_bsolve_end(int n, const int *__restrict__ sel, const SolverState *st0, const double *__restrict__ x0, long long vs,
                                                   double *__restrict__ X, long long ldx, const double *__restrict__ res_norm0, long long rs,
                                                   double *__restrict__ res_stage, long long ncap, BatchFlags *flags, const int *active) {
  const int t = (int)blockIdx.y;
  if (blockIdx.x == 0 && t == 0 && threadIdx.x == 0) flags->active = *active;
  if (t >= sel[0]) return;
  const SolverState *st = st0 + t;
  const long long it = st->it;
  const double *x = x0 + (size_t)t * vs;
  double *xo = X + (size_t)t * ldx;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) xo[i] = x[i];
  if (res_stage) {
    const long long m = it < ncap ? it : ncap;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < m; i += (long long)gridDim.x * NT)
      res_stage[(size_t)t * BATCH_RES_STAGE + i] = res_norm0[(size_t)t * rs + i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { flags->it[t] = it; flags->done[t] = st->done; flags->overflow[t] = st->overflow; }
}

struct BatchKrylov {
  mi_ctx_s *ctx;
  CsrBatchOp *A;
  AmgBankView *M;   // nullptr: cg
  const int pre;
  BatchWorkspace &bw;
  SolverWorkspace &ws;   // of this size: the owner of every solve graph of the context (drop_graphs_of, mi_op_destroy)
  int n, g;
  hipStream_t s;

  BatchKrylov(mi_ctx_s *c, CsrBatchOp *A_, AmgBankView *M_)
      : ctx(c), A(A_), M(M_), pre(M_ != nullptr), bw(A_->workspace()), ws(workspace(c, A_->n)), n((int)A_->n), g(bw.g), s(c->stream) {}

  const int *sel() const { return bw.sel; }
  dim3 vgrid() const { return dim3((unsigned)g, BATCH_MAX); }
  template <bool DOT>
  void spmv(const double *x, double *y, const double *w, const SolverState *st) {
    const CsrDev &C = A->A;
    hipLaunchKernelGGL((k_bspmv<DOT>), dim3((unsigned)(((C.nblocks + 7) / 8) * 8), BATCH_MAX), dim3(NT), 0, s, C.nblocks, (const SpmvBlock *)C.blk.p,
                       (const int *)C.rowptr.p, (const int *)C.col.p, (const double *)A->slab.p, (long long)A->stride, sel(), x, y, w,
                       (long long)bw.vs, bw.dot_part, (long long)bw.dps, st);
  }
  void precondition(const SolverState *st) {   // z_t = Π_{m_t} \ r_t and the partials of r'z
    M->apply_batch(bw.r, (long long)bw.vs, bw.z, (long long)bw.vs, st ? &st->done : nullptr, (long long)(sizeof(SolverState) / sizeof(int)));
    hipLaunchKernelGGL(k_bdot_partial, vgrid(), dim3(NT), 0, s, n, sel(), (const double *)bw.r, (const double *)bw.z, (long long)bw.vs, bw.part_rz, st);
  }
  void setup_tail() {
    spmv<false>(bw.x, bw.Ap, nullptr, nullptr);
    hipLaunchKernelGGL(k_bresidual, vgrid(), dim3(NT), 0, s, n, sel(), (const double *)bw.b, (const double *)bw.Ap, bw.r, (long long)bw.vs, bw.part_rr,
                       bw.part_bb);
    if (pre) precondition(nullptr);
    hipLaunchKernelGGL(k_binit_state, dim3(1, BATCH_MAX), dim3(NT), 0, s, bw.st, sel(), (const double *)bw.part_rr, (const double *)bw.part_bb,
                       pre ? (const double *)bw.part_rz : (const double *)nullptr, g, bw.res_norm, (long long)bw.rs, bw.active);
    hipLaunchKernelGGL(k_binit_p, vgrid(), dim3(NT), 0, s, n, sel(), (const double *)(pre ? bw.z : bw.r), bw.p, (long long)bw.vs);
    MI_HIP(hipGetLastError());
  }
  void iteration() {
    spmv<true>(bw.p, bw.Ap, bw.p, bw.st);
    hipLaunchKernelGGL(k_bupdate_xr, vgrid(), dim3(NT), 0, s, n, sel(), bw.st, (const double *)bw.dot_part, (long long)bw.dps, A->A.nblocks,
                       (const double *)bw.p, (const double *)bw.Ap, bw.x, bw.r, (long long)bw.vs, bw.part_rr, pre);
    if (pre) precondition(bw.st);
    hipLaunchKernelGGL(k_bupdate_p, vgrid(), dim3(NT), 0, s, n, sel(), bw.st, (const double *)bw.part_rr, (const double *)bw.part_rz, g,
                       (const double *)(pre ? bw.z : bw.r), bw.p, (long long)bw.vs, bw.res_norm, (long long)bw.rs, pre, bw.active);
    MI_HIP(hipGetLastError());
  }
  // chunk > 0: `chunk` iterations; chunk < 0: set-up + (-chunk) iterations
  hipGraphExec_t graph(int chunk) {
    GraphKey key{A, M, 0, chunk, BATCH_GRAPH_TAG};
    auto it = ws.graphs.find(key);
    if (it != ws.graphs.end()) return it->second;
    hipGraphExec_t ex = capture_graph(s, "mi_pcg_batch", [&] {
      if (chunk < 0) setup_tail();
      for (int k = 0; k < std::abs(chunk); ++k) iteration();
    });
    ws.graphs[key] = ex;
    ++ctx->n_captures;
    return ex;
  }
  void fetch_active(int slot) {
    MI_HIP(hipMemcpyAsync(&bw.flags[slot].active, bw.active, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipEventRecord(bw.ev[slot], s));
  }

  // B, X: device-visible pointers (column-major, ldb, ldx >= n); slots, members, it_out, res_host: host arrays
  int solve(int k, const int64_t *slots, const int64_t *members, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t maxit, double eps,
            double *res_host, int64_t ldres, int64_t *it_out) {
    if (eps <= 0.0) eps = 1e-7;
    if (maxit == 0) maxit = n;
    const int64_t cap_dev = std::max<int64_t>(1, std::min<int64_t>(maxit, (int64_t)n));
    const int64_t ncap = std::min<int64_t>(ldres, cap_dev);
    const bool spec_res = res_host && ncap > 0;
    BatchSel q{};
    q.k = k;
    for (int t = 0; t < k; ++t) { q.slot[t] = (int)slots[t]; q.member[t] = members ? (int)members[t] : 0; }
    hipLaunchKernelGGL(k_bsolve_begin, vgrid(), dim3(NT), 0, s, n, q, B, (long long)ldb, (const double *)X, (long long)ldx, bw.b, bw.x,
                       (long long)bw.vs, bw.st, eps, (long long)maxit, (long long)cap_dev, bw.sel, M ? M->bsel.p : (int *)nullptr, bw.active);
    MI_HIP(hipGetLastError());
    auto enqueue_results = [&] {
      hipLaunchKernelGGL(k_bsolve_end, vgrid(), dim3(NT), 0, s, n, sel(), (const SolverState *)bw.st, (const double *)bw.x, (long long)bw.vs, X,
                         (long long)ldx, (const double *)bw.res_norm, (long long)bw.rs, spec_res ? bw.res_stage : (double *)nullptr,
                         (long long)std::min<int64_t>(ncap, BATCH_RES_STAGE), &bw.flags[0], (const int *)bw.active);
      MI_HIP(hipGetLastError());
    };
    const bool use_graph = ctx->chunk > 0 && !ctx->no_graph;
    if (use_graph) {
      const GraphKey pk{A, M, 0, 0, BATCH_GRAPH_TAG};
      int &predicted = ws.predicted[pk];
      int64_t first = predicted > 0 ? predicted : ctx->chunk;
      if (first > 64) first -= first % 32;
      first = std::max<int64_t>(1, std::min<int64_t>(first, std::min<int64_t>(maxit, 1024)));
      if (ws.graphs.size() > 48) ws.drop_graphs();
      hipGraphExec_t g0 = graph(-(int)first);
      ++ctx->n_replays; MI_HIP(hipGraphLaunch(g0, s));
      enqueue_results();
      MI_HIP(hipStreamSynchronize(s));
      if (bw.flags[0].active != 0) {
        hipGraphExec_t ex = graph(ctx->chunk);
        const int64_t max_launch = (maxit + ctx->chunk - 1) / ctx->chunk + 2;
        int slot = 0;
        bool stop = false;
        fetch_active(slot);
        for (int64_t l = 0; l < max_launch && !stop; ++l) {
          ++ctx->n_replays; MI_HIP(hipGraphLaunch(ex, s));
          const int prev = slot;
          slot ^= 1;
          fetch_active(slot);
          MI_HIP(hipEventSynchronize(bw.ev[prev]));
          stop = bw.flags[prev].active == 0;
        }
        enqueue_results();
        MI_HIP(hipStreamSynchronize(s));
      }
      long long longest = 1;
      for (int t = 0; t < k; ++t) longest = std::max(longest, bw.flags[0].it[t]);
      predicted = (int)std::max<long long>(1, longest - 1);
    } else {
      setup_tail();
      for (int64_t l = 0; l < maxit + 2; ++l) {
        fetch_active(0);
        MI_HIP(hipEventSynchronize(bw.ev[0]));
        if (bw.flags[0].active == 0) break;
        iteration();
      }
      enqueue_results();
      MI_HIP(hipStreamSynchronize(s));
    }
    const BatchFlags &f = bw.flags[0];
    if (f.active != 0) raise(MI_ERR_HIP, "internal: the batched Krylov loop ended with %d system(s) still active", f.active);
    bool over = false;
    long long worst = 0;
    bool copies = false;
    for (int t = 0; t < k; ++t) {
      const long long it = f.it[t];
      it_out[t] = it;
      if (f.overflow[t] || it > ldres) { over = true; worst = std::max(worst, it); }
      const int64_t ncopy = std::min<int64_t>(it, ncap);
      if (!res_host || ncopy <= 0) continue;
      if (ncopy <= BATCH_RES_STAGE) std::memcpy(res_host + (size_t)t * (size_t)ldres, bw.res_stage + (size_t)t * BATCH_RES_STAGE, sizeof(double) * (size_t)ncopy);
      else {
        MI_HIP(hipMemcpyAsync(res_host + (size_t)t * (size_t)ldres, bw.res_norm + (size_t)t * (size_t)bw.rs, sizeof(double) * (size_t)ncopy,
                              hipMemcpyDeviceToHost, s));
        copies = true;
      }
    }
    if (copies) MI_HIP(hipStreamSynchronize(s));
    if (over) return fail(MI_ERR_RES_CAPACITY, "mi_pcg_batch: res_norm capacity ldres = %lld < it = %lld of some system", (long long)ldres, worst);
    return MI_OK;
  }
};

}  // namespace mi
