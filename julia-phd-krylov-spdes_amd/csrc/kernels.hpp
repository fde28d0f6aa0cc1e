// Device kernels of libmi355schur (gfx950 / CDNA4, wave64). All arithmetic fp64, built with
// -ffp-contract=off so that element-wise updates and the CSR row sums reproduce the
// reference's mul-then-add sequence bit for bit; only tree reductions reorder sums.
//
// Every kernel that runs inside the Krylov loop takes `const int *done`: once the stop rule
// (cg.jl:34,91) has fired, the remaining launches of a captured iteration chunk return at once.
#pragma once
#include <hip/hip_runtime.h>

#include "exchange_dev.hpp"
#include "dense_tiles.hpp"
#include "spmv_blocks.hpp"

namespace mi {

constexpr int NT = 256;        // threads per workgroup for all streaming kernels (4 waves)
constexpr int MAX_PARTS = 512; // max workgroups of a vector kernel = max partial sums per dot

// Scalars of one Krylov solve, resident in HBM (read by every workgroup, written by one).
struct SolverState {
  double rTr, rTz;            // current r'r and r'z
  double rTr_prev, rTz_prev;  // values before this iteration's update (for beta = (1/old)*new)
  double d, alpha, beta;      // diagnostics (each workgroup recomputes them from the partials)
  double tol, bnorm, eps;
  long long it, maxit, res_cap;
  long long it_nxt;           // folded PCG: iteration counter written one launch ahead of `it`
  int done;
  int overflow;               // res_norm capacity hit (BoundsError in the reference)
  int x0_zero;                // the initial guess of this solve is identically zero: `A*x0` need not stream A (set-up only)
};

// What the host reads back after a replay (pinned memory, written by k_solve_end or copied by fetch_flags)
struct PinnedFlags {
  long long it;
  int done;
  int overflow;
  int respec;              // whole-solve graph built for x0 == 0 met a non-zero x0: nothing was done, replay the general one
  int x0z;                 // the initial guess of this solve was identically zero
  long long t_entry, t_exit;  // wall_clock64() (100 MHz) at the entry kernel's start and at the hand-over (MI355_SOLVE_STATS)
  unsigned long long seq;  // whole-solve graph: the solve number, stored LAST by whoever publishes (the host spins on it)
};
// Per-call arguments of a solve whose entry and exit kernels are part of the replayed graph: the host fills this block
// (pinned memory) before the replay, k_solve_begin_g reads it with system-scope loads and leaves a device copy for
// k_solve_end_g.
struct SolveArgs {
  const double *b_in, *x_in;
  double *x_out, *res_stage;
  double eps;
  long long maxit, res_cap, ncap;
  unsigned long long seq;
};

// ------------------------------------------------------------------ the loop's scalar rules, written once
// k_spmv_pcg and k_gemv_pcg<., 0> (the first launch of the two-launch forms, solvers.hpp enum Loop) keep the same rules
// written out: their instruction streams are held to the measured ones (profiles/NOTES.md). A change here goes there too.
// beta = (1/old)*new (cg.jl:39,44 / 96,102): two roundings, as the reference's `beta = 1. / old; beta *= new`.
__device__ __forceinline__ double krylov_beta(double old, double rz) {
  double beta = 1. / old; beta *= rz; return beta;
}
// The stop rule after iteration `it_new` (cg.jl:34,91). over: the reference's `res_norm[it] = ...` throws BoundsError there and
// the loop ends. The negated form stops on a NaN residual.
struct StopRule { bool over, stop; };
__device__ __forceinline__ StopRule krylov_stop(long long it_new, long long maxit, long long cap, double res, double tol) {
  const bool over = it_new > cap;
  return StopRule{over, over || !((it_new < maxit) && (res > tol))};
}
// ... and its stores, by the one thread that writes the state block (GENERIC, FUSED: the counter is `it`).
__device__ __forceinline__ void krylov_count(SolverState *st, double *res_norm, long long it_new, double res, StopRule s) {
  if (!s.over) res_norm[it_new - 1] = res; else st->overflow = 1;
  st->it = it_new; st->done = s.stop;
}
// Start at it = 1 (GENERIC, FUSED; cg.jl:26-33 / 81-89): res_norm[1] and the stop rule. rTr and bnorm are the caller's.
__device__ __forceinline__ void krylov_start_one(SolverState *st, double *res_norm, double rr, double rz, double tol, long long maxit, long long cap) {
  st->rTz = rz; st->rTr_prev = rr; st->rTz_prev = rz; st->tol = tol;
  st->d = 0.0; st->alpha = 0.0; st->beta = 0.0; st->overflow = 0;
  const double res = sqrt(rr);
  krylov_count(st, res_norm, 1, res, krylov_stop(1, maxit, cap, res, tol));
}
// Start at it = 0 (the two-launch forms): the first launch of the loop counts to 1, stores res_norm[1], applies the stop rule. The folded
// loop passes (rTz, rTr_prev) = (0, r'r); the sparse one (r'z, 1): without M its first beta is r'r / rTr_prev, times p = 0, and 1 / r'r can be Inf.
__device__ __forceinline__ void krylov_start_zero(SolverState *st, double rr, double bb, double eps, double rTz, double rTr_prev) {
  st->rTr = rr; st->bnorm = sqrt(bb); st->tol = eps * st->bnorm;
  st->it = 0; st->it_nxt = 0; st->done = 0; st->overflow = 0;
  st->rTz = rTz; st->rTz_prev = 1.0; st->rTr_prev = rTr_prev;
  st->d = 0.0; st->alpha = 0.0; st->beta = 0.0;
}
// Entry of a whole-solve graph: the pinned argument block, read with system-scope loads into `a` (LDS) by every workgroup.
__device__ __forceinline__ unsigned long long sys_load_u64(const void *p) { return __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
constexpr unsigned SOLVE_ARGS_WORDS = sizeof(SolveArgs) / 8;
static_assert(sizeof(SolveArgs) % 8 == 0 && SOLVE_ARGS_WORDS <= 64, "SolveArgs is a block of 8-byte fields");
__device__ __forceinline__ const SolveArgs &load_solve_args(const SolveArgs *pin, unsigned long long *a) {
  if (threadIdx.x < SOLVE_ARGS_WORDS) a[threadIdx.x] = sys_load_u64((const unsigned long long *)pin + threadIdx.x);
  __syncthreads();
  return *reinterpret_cast<const SolveArgs *>(a);
}
// Hand-over of a whole-solve graph, by one thread: the flags, a release to system scope, then ONE store of the solve number.
__device__ __forceinline__ void publish_flags(PinnedFlags *fl, long long it, int done, int overflow, int respec, int x0z, bool stamp_exit, unsigned long long seq) {
  fl->it = it; fl->done = done; fl->overflow = overflow; fl->respec = respec; fl->x0z = x0z;
  if (stamp_exit) fl->t_exit = wall_clock64();
  __threadfence_system();
  __hip_atomic_store(&fl->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------ reductions
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the sum
}
// Deterministic workgroup sum, result broadcast to all threads: per-wave shuffle tree, the NTH/64 wave results through
// LDS, then the same shuffle tree over them in every wave (no serial chain). `sm` has NTH/64 doubles (callers size it
// NTH/64 + 1); the trailing barrier lets the next call reuse it.
template <int NTH>
__device__ __forceinline__ double block_sum_t(double v, double *sm) {
  constexpr int NW = NTH / 64;
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sm[w] = v;
  __syncthreads();
  double t = lane < NW ? sm[lane] : 0.0;
#pragma unroll
  for (int off = NW / 2; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  t = __shfl(t, 0, 64);
  __syncthreads();
  return t;
}
__device__ __forceinline__ double block_sum(double v, double *sm) { return block_sum_t<NT>(v, sm); }
// Two workgroup sums with ONE barrier: per-wave shuffle trees, then every wave reduces the NTH/64 wave results with a
// second shuffle tree (no serial LDS chain, no second barrier). Fixed tree: deterministic, identical in every workgroup.
// `sm` has 2*(NTH/64) doubles and must not be reused before the next barrier.
template <int NTH>
__device__ __forceinline__ void block_sum2_t(double &a, double &b, double *sm) {
  constexpr int NW = NTH / 64;
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sm[w] = a; sm[NW + w] = b; }
  __syncthreads();
  double ta = lane < NW ? sm[lane] : 0.0, tb = lane < NW ? sm[NW + lane] : 0.0;
#pragma unroll
  for (int off = NW / 2; off > 0; off >>= 1) {
    ta += __shfl_down(ta, off, 64);
    tb += __shfl_down(tb, off, 64);
  }
  a = __shfl(ta, 0, 64);
  b = __shfl(tb, 0, 64);
}
// Sum of `g` per-workgroup partials, in a fixed order, identical in every workgroup.
__device__ __forceinline__ double sum_partials(const double *part, int g, double *sm) {
  double v = 0.0;
  for (int i0 = threadIdx.x; i0 < g; i0 += 8 * NT) {  // eight loads in flight per thread (a plain loop pays one round trip each)
    double t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = i0 + k * NT < g ? part[i0 + k * NT] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += t[k];
  }
  return block_sum(v, sm);
}

// (W*mu)[i] in column order (wm += W[i,k]*mu[k], k ascending — the order of a column-axpy gemv), with the loads of
// eight columns issued together: a plain runtime loop serialises one memory round trip per column.
__device__ __forceinline__ double w_times_mu(const double *__restrict__ W, long long n, long long i,
                                             const double *__restrict__ mu, int nvec) {
  double wm = 0.0;
  for (int q0 = 0; q0 < nvec; q0 += 8) {
    double w[8], m[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool ok = q0 + u < nvec;
      w[u] = ok ? W[(long long)(q0 + u) * n + i] : 0.0;
      m[u] = ok ? mu[q0 + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (q0 + u < nvec) wm += w[u] * m[u];
  }
  return wm;
}

// ------------------------------------------------------------------ BLAS-1 building blocks
__global__ __launch_bounds__(NT) void k_dot_partial(int n, const double *__restrict__ x,
                                                    const double *__restrict__ y, double *__restrict__ part,
                                                    const int *done) {
  if (done && *done) return;
  __shared__ double sm[NT / 64 + 1];
  double s = 0.0;
  const int stride = gridDim.x * NT;
  for (int i0 = blockIdx.x * NT + threadIdx.x; i0 < n; i0 += 4 * stride) {  // four elements in flight per thread, summed in order
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
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// out[0] = sum(part[0..g)) (or its square root)
__global__ __launch_bounds__(NT) void k_finish_sum(const double *part, int g, double *out, int take_sqrt) {
  __shared__ double sm[NT / 64 + 1];
  double s = sum_partials(part, g, sm);
  if (threadIdx.x == 0) out[0] = take_sqrt ? sqrt(s) : s;
}
__global__ __launch_bounds__(NT) void k_axpy(int n, double a, const double *__restrict__ x, double *__restrict__ y) {
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) y[i] = y[i] + a * x[i];
}
__global__ __launch_bounds__(NT) void k_axpby(int n, double a, const double *__restrict__ x, double b,
                                              double *__restrict__ y) {
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) y[i] = a * x[i] + b * y[i];
}
// z = dinv .* r (Jacobi) or z = r (identity)
__global__ __launch_bounds__(NT) void k_diag_apply(int n, const double *__restrict__ dinv,
                                                   const double *__restrict__ r, double *__restrict__ z,
                                                   const int *done) {
  if (done && *done) return;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) z[i] = dinv ? dinv[i] * r[i] : r[i];
}

// ------------------------------------------------------------------ CSR SpMV ("CSR-stream")
// One workgroup owns a block of consecutive rows holding <= SPMV_TILE non-zeros. Phase 1 streams
// the block's column indices and values with coalesced loads, gathers x and parks the products in
// LDS; phase 2 gives each row to one thread, which adds its products left to right — the order
// of the reference's CSC scatter SpMV for a symmetric matrix (stdlib SparseArrays `A*x`,
// `y[rowval[k]] += nzval[k]*x[j]`, j ascending), so y is bit-identical to it.
// Row blocks are dealt to XCDs in contiguous ranges (blockIdx % 8 selects the range) so that each
// XCD's L2 caches one slice of x instead of all of it.
// SPMV_TILE, the block record SpmvBlock and the partition of the rows into blocks: spmv_blocks.hpp (host code, no HIP).

template <int MODE, bool DOT>  // MODE 0: y = A x, 1: y = yin - A x;  DOT: also part[b] = Σ_{rows of block b} w[r]*y[r]
__global__ __launch_bounds__(NT) void k_spmv_csr(int nblocks, const SpmvBlock *__restrict__ blk,
                                                 const int *__restrict__ rowptr, const int *__restrict__ col,
                                                 const double *__restrict__ val, const double *__restrict__ x,
                                                 const double *yin, double *y, const double *__restrict__ w,
                                                 double *__restrict__ part, const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  __shared__ double sm[NT / 64 + 1];
  const int per = (nblocks + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (b >= nblocks) return;
  const SpmvBlock bi = blk[b];
  const int r0 = bi.r0, r1 = bi.r1, k0 = bi.k0;
  const int nnz = bi.k1 - k0;
  double wy = 0.0;
  if (nnz <= SPMV_TILE) {
    // row bounds of this thread's first two rows: independent of phase 1, so issue the loads now
    const int ra = r0 + threadIdx.x, rbb = ra + NT;
    int a0 = 0, e0 = 0, a1 = 0, e1 = 0;
    double w0 = 0.0, w1 = 0.0;  // the dot's weights for those rows too: one fewer round trip in the epilogue
    if (ra < r1) { a0 = rowptr[ra] - k0; e0 = rowptr[ra + 1] - k0; if (DOT) w0 = w[ra]; }
    if (rbb < r1) { a1 = rowptr[rbb] - k0; e1 = rowptr[rbb + 1] - k0; if (DOT) w1 = w[rbb]; }
    if ((k0 & 1) == 0) {  // 16-byte aligned values, 8-byte aligned indices: two non-zeros per load
      const int npair = (nnz + 1) >> 1;
      for (int q = threadIdx.x; q < npair; q += NT) {
        const int k = 2 * q;
        if (k + 1 < nnz) {
          const int2 c = *reinterpret_cast<const int2 *>(col + k0 + k);
          const double2 v = *reinterpret_cast<const double2 *>(val + k0 + k);
          *reinterpret_cast<double2 *>(&prod[k]) = make_double2(v.x * x[c.x], v.y * x[c.y]);
        } else {
          prod[k] = val[k0 + k] * x[col[k0 + k]];
        }
      }
    } else {
      for (int k = threadIdx.x; k < nnz; k += NT) prod[k] = val[k0 + k] * x[col[k0 + k]];
    }
    __syncthreads();
    for (int r = ra, i = 0; r < r1; r += NT, ++i) {
      int a, e;
      if (i == 0) { a = a0; e = e0; }
      else if (i == 1) { a = a1; e = e1; }
      else { a = rowptr[r] - k0; e = rowptr[r + 1] - k0; }
      double sum = 0.0;
      for (int k = a; k < e; ++k) sum += prod[k];
      const double yr = MODE ? yin[r] - sum : sum;
      y[r] = yr;
      if (DOT) wy += (i == 0 ? w0 : i == 1 ? w1 : w[r]) * yr;
    }
  } else {
    // a single row longer than the tile (never the case for P1-FEM blocks): tile by tile,
    // thread 0 keeps the running left-to-right sum.
    double sum = 0.0;
    for (int t0 = 0; t0 < nnz; t0 += SPMV_TILE) {
      const int m = min(SPMV_TILE, nnz - t0);
      for (int k = threadIdx.x; k < m; k += NT) prod[k] = val[k0 + t0 + k] * x[col[k0 + t0 + k]];
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < m; ++k) sum += prod[k];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double yr = MODE ? yin[r0] - sum : sum;
      y[r0] = yr;
      if (DOT) wy = w[r0] * yr;
    }
  }
  if (DOT) {
    wy = block_sum(wy, sm);
    if (threadIdx.x == 0) part[b] = wy;
  }
}

// ------------------------------------------------------------------ pcg on a sparse matrix in 2 launches per iteration
// Config 2 (`pcg(A, b, x, M)` on the full matrix, M diagonal or absent; cg.jl:67-109 / 14-50). The three launches of the
// generic loop (SpMV + p'Ap, x/r/z update, p update) become two, and every vector element is written on the XCD that
// reads it next:
//   k_spmv_pcg     : r'r, r'z from the partials -> it += 1, res_norm[it], stop rule, beta (cg.jl:91, 102-106); then the
//                    CSR-stream SpMV of the NEW direction without materialising it first: a gathered entry is
//                    beta*p_old[c] + z[c], computed on the fly from the interleaved pair (p_old[c], z[c]) — one 16-byte
//                    gather per non-zero, the same arithmetic (hence bits) in every workgroup; the row owner stores
//                    p_new[r]; Ap[r]; per-block partial p'Ap (cg.jl:93-94).
//   k_update_xr_blk: alpha = r'z / p'Ap; x += alpha p; r -= alpha Ap; z = M \ r (diagonal); per-block partials r'r, r'z
//                    (cg.jl:95-101), one workgroup per row block with the SpMV's block -> XCD mapping.
// The pairs live in two buffers used alternately (parity of `it`), so no launch reads what it writes; scalars follow the
// it / it_nxt, rTz / rTz_prev hand-off of the folded Schur loop. Start-up: it = 0, p = 0, rTz_prev = 1, so the first
// k_spmv_pcg produces it = 1, res_norm[1] = ||r_0||, p = z_0.
__device__ __forceinline__ int spmv_block_of(int nblocks) {
  const int per = (nblocks + 7) >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}
__global__ __launch_bounds__(NT, 8) void k_spmv_pcg(int nblocks, int precond, const SpmvBlock *__restrict__ blk, SolverState *st,
                                                 const double *part_rr, const double *part_rz, int g_vec,
                                                 const int *__restrict__ rowptr,   // (up to here: preloaded into SGPRs at wave start)
                                                 const int *__restrict__ col, const double *__restrict__ val, double *pz0, double *pz1,
                                                 double *__restrict__ Ap, double *__restrict__ part_pAp, double *res_norm) {
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  __shared__ double sm[NT / 64 + 1];
  const int b = spmv_block_of(nblocks);
  const bool has = b < nblocks;
  // block record, state block and stop flag in one memory round trip (the empty asm keeps the compiler from sinking the
  // loads below the early exit)
  const SpmvBlock bi = blk[has ? b : 0];
  const int done0 = st->done;
  const long long it0 = st->it, maxit = st->maxit, cap = st->res_cap;
  const double tol = st->tol, old = precond ? st->rTz_prev : st->rTr_prev;
  asm volatile("" ::"s"(bi.r0), "s"(bi.r1), "s"(bi.k0), "s"(bi.k1), "s"(done0), "s"(it0), "s"(maxit), "s"(cap), "s"(tol), "s"(old));
  // the partial sums of the previous launch are requested FIRST (they need no index): results return in issue order, so the
  // reduction to beta below waits for these two loads only while the non-zeros and their gathered pairs are still in flight
  double rr = (int)threadIdx.x < g_vec ? part_rr[threadIdx.x] : 0.0;
  double rz = (precond && (int)threadIdx.x < g_vec) ? part_rz[threadIdx.x] : 0.0;
  if (done0) return;
  const int r0 = has ? bi.r0 : 0, r1 = has ? bi.r1 : 0, k0 = has ? bi.k0 : 0, nnz = has ? bi.k1 - bi.k0 : 0;
  const double2 *pz_old = reinterpret_cast<const double2 *>((it0 & 1) ? pz1 : pz0);
  double2 *pz_new = reinterpret_cast<double2 *>((it0 & 1) ? pz0 : pz1);
  // everything that does not depend on beta is requested before the reduction: this thread's non-zeros (SPMV_TILE / NT
  // of them) with their gathered pairs, and the bounds and pairs of its first two rows
  constexpr int KPT = SPMV_TILE / NT;
  double vv[KPT];
  double2 gp[KPT];
  const bool fits = nnz <= SPMV_TILE;
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const int k = q * NT + (int)threadIdx.x;
    vv[q] = 0.0; gp[q] = make_double2(0.0, 0.0);
    if (fits && k < nnz) { vv[q] = val[k0 + k]; gp[q] = pz_old[col[k0 + k]]; }
  }
  const int ra = r0 + threadIdx.x;
  int a0 = 0, e0 = 0;
  double2 o0 = make_double2(0.0, 0.0);
  if (ra < r1) { a0 = rowptr[ra] - k0; e0 = rowptr[ra + 1] - k0; o0 = pz_old[ra]; }
  // ---- scalars (identical in every workgroup): g_vec <= NT partials per sum, one load per thread (above), one barrier for both
  __shared__ double sm2[2 * (NT / 64)];
  block_sum2_t<NT>(rr, rz, sm2);
  if (!precond) rz = rr;
  double beta = 1. / old;
  beta *= rz;
  const long long it_new = it0 + 1;
  const double res = sqrt(rr);
  const bool over = it_new > cap;
  const bool stop = over || !((it_new < maxit) && (res > tol));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->rTr = rr; st->rTz = rz; st->beta = beta;
    st->it_nxt = it_new;
    if (!over) res_norm[it_new - 1] = res; else st->overflow = 1;
    if (stop) st->done = 1;
  }
  if (stop || !has) return;
  double wy = 0.0;
  if (fits) {
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const int k = q * NT + (int)threadIdx.x;
      if (k < nnz) prod[k] = vv[q] * (beta * gp[q].x + gp[q].y);       // A[r,c] * (beta p + z)[c]
    }
    __syncthreads();
    for (int r = ra, i = 0; r < r1; r += NT, ++i) {
      int a, e;
      double2 o;
      if (i == 0) { a = a0; e = e0; o = o0; }
      else { a = rowptr[r] - k0; e = rowptr[r + 1] - k0; o = pz_old[r]; }
      double sum = 0.0;
      for (int k = a; k < e; ++k) sum += prod[k];                      // left to right: the CSC scatter order (bit-exact)
      const double pn = beta * o.x + o.y;                              // axpby!(1, z, beta, p)
      Ap[r] = sum;
      pz_new[r].x = pn;
      wy += pn * sum;
    }
  } else {  // one row longer than the tile: tile by tile, thread 0 keeps the running sum
    double sum = 0.0;
    for (int t0 = 0; t0 < nnz; t0 += SPMV_TILE) {
      const int m = min(SPMV_TILE, nnz - t0);
      for (int k = threadIdx.x; k < m; k += NT) {
        const double2 g = pz_old[col[k0 + t0 + k]];
        prod[k] = val[k0 + t0 + k] * (beta * g.x + g.y);
      }
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < m; ++k) sum += prod[k];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double2 o = pz_old[r0];
      const double pn = beta * o.x + o.y;
      Ap[r0] = sum;
      pz_new[r0].x = pn;
      wy = pn * sum;
    }
  }
  wy = block_sum(wy, sm);
  if (threadIdx.x == 0) part_pAp[b] = wy;
}
// Grid = 8 * nj workgroups: workgroup k works on XCD k & 7 (blocks are dealt round-robin over the XCDs) and takes the
// (k >> 3)-th of nj equal slices of the rows whose SpMV row blocks run on that XCD (`xcd_row[x] .. xcd_row[x + 1]`), so
// that z, r, x are written into the L2 that k_spmv_pcg's gathers and row sums read them from.
__global__ __launch_bounds__(NT) void k_update_xr_blk(const int *__restrict__ xcd_row, SolverState *st, const double *part_pAp,
                                                      int nblocks, double *pz0, double *pz1, const double *__restrict__ Ap,
                                                      double *__restrict__ x, double *__restrict__ r,
                                                      const double *__restrict__ dinv, int diag, int precond,
                                                      double *__restrict__ part_rr, double *__restrict__ part_rz) {
  __shared__ double sm[NT / 64 + 1];
  const int xc = blockIdx.x & 7, j = blockIdx.x >> 3, nj = gridDim.x >> 3;
  const long long R0 = xcd_row[xc], R1 = xcd_row[xc + 1];
  const int done0 = st->done;
  const long long it_n = st->it_nxt;
  const double rTr0 = st->rTr, rTz0 = st->rTz;
  asm volatile("" ::"s"(R0), "s"(R1), "s"(done0), "s"(it_n), "s"(rTr0), "s"(rTz0), "s"(nj));   // one round trip (the grid size, an implicit kernel argument, included), then the exit test
  if (done0) return;
  const int lo = (int)(R0 + (R1 - R0) * j / nj), hi = (int)(R0 + (R1 - R0) * (j + 1) / nj);
  const double num = precond ? rTz0 : rTr0;
  double2 *pz = reinterpret_cast<double2 *>((it_n & 1) ? pz1 : pz0);     // the pairs k_spmv_pcg has just written p into
  // the partial sums of p'Ap first (up to eight per thread in flight; more in the loop below), then the first four rows of this
  // thread: everything is requested ahead of the reduction, and the reduction waits for the partials only
  double dpart = 0.0;
  double t8[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { const int i = (int)threadIdx.x + k * NT; t8[k] = i < nblocks ? part_pAp[i] : 0.0; }
  double pv[4], av[4], xv[4], rv[4], dv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rw = lo + k * NT + (int)threadIdx.x;
    const bool ok = rw < hi;
    pv[k] = ok ? pz[rw].x : 0.0; av[k] = ok ? Ap[rw] : 0.0; xv[k] = ok ? x[rw] : 0.0; rv[k] = ok ? r[rw] : 0.0;
    dv[k] = ok && diag == 2 ? dinv[rw] : 1.0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) dpart += t8[k];                            // (the order sum_partials uses: bit-identical alpha)
  for (int i0 = (int)threadIdx.x + 8 * NT; i0 < nblocks; i0 += 8 * NT) {
    double u8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) u8[k] = i0 + k * NT < nblocks ? part_pAp[i0 + k * NT] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) dpart += u8[k];
  }
  const double d = block_sum(dpart, sm);
  const double alpha = num / d;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->d = d; st->alpha = alpha;
    st->rTr_prev = rTr0; st->rTz_prev = rTz0;
    st->it = it_n;
  }
  double srr = 0.0, srz = 0.0;
  for (int rw = lo + (int)threadIdx.x, i = 0; rw < hi; rw += NT, ++i) {
    double p_, a_, x_, r_, d_;
    if (i < 4) { p_ = pv[i]; a_ = av[i]; x_ = xv[i]; r_ = rv[i]; d_ = dv[i]; }
    else { p_ = pz[rw].x; a_ = Ap[rw]; x_ = x[rw]; r_ = r[rw]; d_ = diag == 2 ? dinv[rw] : 1.0; }
    x[rw] = x_ + alpha * p_;                     // axpy!(alpha, p, x)
    const double ri = r_ + (-alpha) * a_;        // axpy!(-alpha, Ap, r)
    r[rw] = ri;
    const double zi = diag == 2 ? d_ * ri : ri;  // z .= M \ r
    pz[rw].y = zi;
    srr += ri * ri;
    srz += ri * zi;
  }
  srr = block_sum(srr, sm);
  srz = block_sum(srz, sm);
  if (threadIdx.x == 0) { part_rr[blockIdx.x] = srr; part_rz[blockIdx.x] = srz; }
}
// Start-up of that loop after r_0 (and z_0) exist: pairs (0, z_0) into buffer 0; the g_vec partials = (r'r, r'z, 0, 0, ...);
// scalars as k_fused_residual<., true> leaves them for the folded Schur loop.
__global__ __launch_bounds__(NT) void k_csrfold_start(int n, int g_vec, SolverState *st, const double *part_rr_in,
                                                      const double *part_bb_in, const double *part_rz_in, int g_in,
                                                      const double *__restrict__ z, double *__restrict__ pz0,
                                                      double *__restrict__ part_rr, double *__restrict__ part_rz) {
  __shared__ double sm[NT / 64 + 1];
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    pz0[2 * (long long)i] = 0.0;
    pz0[2 * (long long)i + 1] = z[i];
  }
  for (int i = blockIdx.x * NT + threadIdx.x; i < g_vec; i += gridDim.x * NT)
    if (i > 0) { part_rr[i] = 0.0; part_rz[i] = 0.0; }
  if (blockIdx.x == 0) {
    const double eps = st->eps;
    const double rr = sum_partials(part_rr_in, g_in, sm);
    const double bb = sum_partials(part_bb_in, g_in, sm);
    const double rz = part_rz_in ? sum_partials(part_rz_in, g_in, sm) : rr;
    if (threadIdx.x == 0) {
      part_rr[0] = rr; part_rz[0] = rz;
      krylov_start_zero(st, rr, bb, eps, rz, 1.0);
    }
  }
}

// ------------------------------------------------------------------ interior CG on the device
// The reference's matrix-free Schur applies solve A_IIdd v = A_IΓdd xd with `IterativeSolvers.cg(A, b; reltol)`
// (EPDD.jl:648-650; third-party, restated from its published iteration, IterativeSolvers.jl cg.jl `CGIterable`):
//     x = 0, r = b, u = 0, residual = ||r||, prev_residual = 1, tol = reltol*residual, maxiter = n
//     while residual > tol and iteration < maxiter:
//         beta = residual^2 / prev_residual^2;  u = r + beta u;  c = A u
//         alpha = residual^2 / (u'c);  x += alpha u;  r -= alpha c;  prev_residual = residual;  residual = ||r||
// All local subdomains are solved at once on the block-diagonal A_II with per-subdomain scalars; row blocks never
// straddle subdomains. One iteration = k_spmv_csr<0,true> (c = A u with the u'c partials) + k_icg_update<PL> +
// k_icg_direction<PL>. Per-subdomain scalars are double-buffered (cur/nxt) so no launch reads what it writes;
// a converged subdomain is frozen (its workgroups return), the others keep iterating.
// The left preconditioner `Pl` of `cg(A, b; Pl, reltol)`: c = Pl \ r, rho = dot(c, r), beta = rho / rho_prev, u = c + beta u,
// alpha = rho / u'c. The four kernels are instantiated per kind; the kind decides what is read, never a pointer that is NULL.
enum IcgPl {
  ICG_PL_NONE,  // z = r: rho = residual^2
  ICG_PL_DIAG,  // z = dinv .* r, made where it is used
  ICG_PL_EXT    // z = Pl \ r lies in memory as a vector over all subdomains, made by launches of the preconditioner's own
                // between k_icg_update and k_icg_direction (the AMG V-cycle of the stacked A_II, interior_amg.hpp), which also
                // leave partial sums of r'z, a fixed run of them per subdomain
};
// A "piece" of the interior CG's vector kernels: a run of rows of ONE subdomain inside one XCD's share of the SpMV row blocks
struct IcgPiece {
  int lo, hi, dom, slot;  // rows [lo, hi) of subdomain dom; partial slot (consecutive within the subdomain)
  int b0, b1, lead, pad;  // row-block range of the subdomain (partials of u'c); first piece of the subdomain
  int p0, p1;             // partial-slot range of the subdomain (all of its pieces)
};
struct IcgMeta {
  const SpmvBlock *blk;
  const int *blk_dom;          // subdomain of every row block
  const int *dom_b0, *dom_b1;  // row-block range of every subdomain
  double *res_cur, *res_nxt;   // residual norms
  double *tol;
  int *done_cur, *done_nxt, *iters;
  int maxiter_cap;             // 0: maxiter = n_i of the subdomain
  const double *dinv;          // 1 / diagonal of A; read by the DIAG instantiations only
  double *rho_cur, *rho_nxt;
  double *p_rz;                // per-piece partials of r'z (DIAG)
  const int *dom_p0, *dom_p1;  // partial-slot range of every subdomain (pieces of the vector kernels)
  // EXT only (nullptr otherwise)
  const double *z;             // z = Pl \ r, all subdomains
  const double *p_rzq;         // partials of r'z left by the preconditioner's launches
  const int *dom_q0, *dom_q1;  // their range per subdomain, summed in icg_dom_sum's fixed order
  // 1 once every subdomain has stopped: the `done` word of the SpMV and of the preconditioner's launches, so the rest of a
  // graph replay returns at once. It is written by workgroup 0 of k_icg_update<EXT> from the flags the direction kernel of the
  // iteration before left, i.e. never by the launch that reads it.
  int *all_done;
  int ndl;
};
// `while residual > tol`: a NaN residual ends the solve where it stands (at x = 0 when the right-hand side holds it)
__device__ __forceinline__ bool icg_converged(double res, double tol) { return !(res > tol); }
// `while residual > tol && iteration < maxiter`: the one stop rule of the 3-launch and the 2-launch form
__device__ __forceinline__ bool icg_stop(double res, double tol, int it, int maxiter) { return icg_converged(res, tol) || it >= maxiter; }
// the scalars of subdomain d when a solve starts: residual = ||b||, rho, tol = reltol * residual, flags
__device__ __forceinline__ void icg_dom_start(const IcgMeta &m, int d, double res, double rho, double reltol) {
  m.res_cur[d] = res; m.res_nxt[d] = res;
  m.rho_cur[d] = rho; m.rho_nxt[d] = rho;
  m.tol[d] = reltol * res;
  m.iters[d] = 0;
  const int dn = icg_converged(res, m.tol[d]);
  m.done_cur[d] = dn; m.done_nxt[d] = dn;
}
// ... and when an iteration ends: its count, the residual, rho (without `Pl` it is residual^2 and not kept), the stop test
template <IcgPl PL>
__device__ __forceinline__ void icg_dom_next(const IcgMeta &m, int d, double res, double rho, const int *__restrict__ n_i) {
  const int it = m.iters[d] + 1;
  m.iters[d] = it;
  m.res_nxt[d] = res;
  if constexpr (PL != ICG_PL_NONE) m.rho_nxt[d] = rho;
  const int maxiter = m.maxiter_cap > 0 ? m.maxiter_cap : n_i[d];
  m.done_nxt[d] = icg_stop(res, m.tol[d], it, maxiter);
}
__device__ __forceinline__ double icg_dom_sum(const double *part, int b0, int b1, double *sm) {
  double v = 0.0;
  for (int i0 = b0 + (int)threadIdx.x; i0 < b1; i0 += 8 * NT) {  // eight loads in flight per thread, added in order
    double t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = i0 + k * NT < b1 ? part[i0 + k * NT] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += t[k];
  }
  return block_sum(v, sm);
}
// The vector kernels work on "pieces" (IcgPiece: a run of ~2 000 rows of ONE subdomain inside one XCD's share of the SpMV
// row blocks, ~512 workgroups in all, first rows requested ahead of the reduction) instead of one small workgroup per SpMV
// row block (6 800 workgroups of ~146 rows at 1 M DoF, each a chain of round trips): 46 -> 41 us per iteration.
// r = rhs; x = 0; u = z_0 (beta*0); partials of r'r (and r'z). EXT: z_0 = Pl \ b is not made yet, so u waits for k_icg_start;
// all_done = 0 (the first z = Pl \ b always runs)
template <IcgPl PL>
__global__ __launch_bounds__(NT) void k_icg_init(IcgMeta m, const IcgPiece *__restrict__ pieces, const double *__restrict__ rhs,
                                                 double *__restrict__ x, double *__restrict__ r, double *__restrict__ u,
                                                 double *__restrict__ p_rr) {
  __shared__ double sm[NT / 64 + 1];
  if constexpr (PL == ICG_PL_EXT)
    if (blockIdx.x == 0 && threadIdx.x == 0) *m.all_done = 0;
  const IcgPiece pc = pieces[blockIdx.x];
  if (pc.hi <= pc.lo) return;
  double s = 0.0, sz = 0.0;
  for (int i = pc.lo + threadIdx.x; i < pc.hi; i += NT) {
    const double v = rhs[i];
    r[i] = v; x[i] = 0.0;
    s += v * v;
    if constexpr (PL == ICG_PL_NONE) u[i] = v;
    if constexpr (PL == ICG_PL_DIAG) {
      const double z = m.dinv[i] * v;
      u[i] = z;
      sz += v * z;
    }
  }
  s = block_sum(s, sm);
  if constexpr (PL == ICG_PL_DIAG) sz = block_sum(sz, sm);
  if (threadIdx.x == 0) {
    p_rr[pc.slot] = s;
    if constexpr (PL == ICG_PL_DIAG) m.p_rz[pc.slot] = sz;
  }
}
// one workgroup per subdomain: residual = ||b||, rho, tol = reltol*residual, flags. EXT (after z_0 = Pl \ b): the grid is
// npieces + ndl; workgroups [0, npieces): u = z_0 on the piece; workgroup npieces + d: subdomain d with rho = b'z_0
template <IcgPl PL>
__global__ __launch_bounds__(NT) void k_icg_start(IcgMeta m, const IcgPiece *__restrict__ pieces, const double *p_rr, double reltol,
                                                  double *__restrict__ u, int npieces) {
  __shared__ double sm[NT / 64 + 1];
  int d = blockIdx.x;
  if constexpr (PL == ICG_PL_EXT) {
    if (d < npieces) {
      const IcgPiece pc = pieces[d];
      for (int i = pc.lo + threadIdx.x; i < pc.hi; i += NT) u[i] = m.z[i];
      return;
    }
    d -= npieces;
  }
  const int p0 = m.dom_p0[d], p1 = m.dom_p1[d];
  const double rr = icg_dom_sum(p_rr, p0, p1, sm);
  double rz = 0.0;
  // (DIAG sums the same range twice. An empty one sums to 0; leaving it out also keeps the second sum in a basic block of its
  // own, as the run-time test of dinv used to: one VGPR fewer than with both sums in one block. k_icg_direction likewise.)
  if constexpr (PL == ICG_PL_DIAG) { if (p1 > p0) rz = icg_dom_sum(m.p_rz, p0, p1, sm); }
  if constexpr (PL == ICG_PL_EXT) rz = icg_dom_sum(m.p_rzq, m.dom_q0[d], m.dom_q1[d], sm);
  if (threadIdx.x == 0) {
    const double res = sqrt(rr);
    icg_dom_start(m, d, res, PL == ICG_PL_NONE ? res * res : rz, reltol);
  }
}
// alpha = rho / (u'c); x += alpha u; r -= alpha c; partials of r'r (DIAG: and r'z; EXT: r'z comes from the preconditioner's
// launches, and workgroup 0 writes all_done)
template <IcgPl PL>
__global__ __launch_bounds__(NT) void k_icg_update(IcgMeta m, const IcgPiece *__restrict__ pieces, const double *__restrict__ p_uc,
                                                   const double *__restrict__ u, const double *__restrict__ c, double *__restrict__ x,
                                                   double *__restrict__ r, double *__restrict__ p_rr) {
  __shared__ double sm[NT / 64 + 1];
  if constexpr (PL == ICG_PL_EXT) {
    if (blockIdx.x == 0) {
      int a = 1;
      for (int i = threadIdx.x; i < m.ndl; i += NT) a &= m.done_nxt[i] != 0;
      a = __syncthreads_and(a);
      if (threadIdx.x == 0) *m.all_done = a;
    }
  }
  const IcgPiece pc = pieces[blockIdx.x];
  if (pc.hi <= pc.lo) return;
  const int d = pc.dom;
  const bool lead = pc.lead && threadIdx.x == 0;
  const int dn = m.done_nxt[d];
  const double res = m.res_nxt[d];
  double rho = 0.0;
  if constexpr (PL != ICG_PL_NONE) rho = m.rho_nxt[d];
  // the first four rows of this thread: requested together with the scalars, ahead of the reduction
  double uv[4], cv[4], xv[4], rv[4];
  [[maybe_unused]] double dv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rw = pc.lo + k * NT + (int)threadIdx.x;
    const bool ok = rw < pc.hi;
    uv[k] = ok ? u[rw] : 0.0; cv[k] = ok ? c[rw] : 0.0; xv[k] = ok ? x[rw] : 0.0; rv[k] = ok ? r[rw] : 0.0;
    if constexpr (PL == ICG_PL_DIAG) dv[k] = ok ? m.dinv[rw] : 1.0;
  }
  if (dn) { if (lead) m.done_cur[d] = 1; return; }
  const double uc = icg_dom_sum(p_uc, pc.b0, pc.b1, sm);
  if constexpr (PL == ICG_PL_NONE) rho = res * res;
  const double alpha = rho / uc;
  double s = 0.0, sz = 0.0;
  for (int rw = pc.lo + (int)threadIdx.x, i = 0; rw < pc.hi; rw += NT, ++i) {
    double u_, c_, x_, r_;
    [[maybe_unused]] double d_;
    if (i < 4) {
      u_ = uv[i]; c_ = cv[i]; x_ = xv[i]; r_ = rv[i];
      if constexpr (PL == ICG_PL_DIAG) d_ = dv[i];
    } else {
      u_ = u[rw]; c_ = c[rw]; x_ = x[rw]; r_ = r[rw];
      if constexpr (PL == ICG_PL_DIAG) d_ = m.dinv[rw];
    }
    x[rw] = x_ + alpha * u_;
    const double ri = r_ - alpha * c_;
    r[rw] = ri;
    s += ri * ri;
    if constexpr (PL == ICG_PL_DIAG) sz += ri * (d_ * ri);
  }
  s = block_sum(s, sm);
  if constexpr (PL == ICG_PL_DIAG) sz = block_sum(sz, sm);
  if (threadIdx.x == 0) {
    p_rr[pc.slot] = s;
    if constexpr (PL == ICG_PL_DIAG) m.p_rz[pc.slot] = sz;
  }
  if (lead) { m.res_cur[d] = res; m.rho_cur[d] = rho; m.done_cur[d] = 0; }
}
// residual = ||r||; beta = residual^2 / prev_residual^2 (rho / rho_prev with Pl, rho = r'z from the partials); u = z + beta u;
// iteration count and stop test. `r` is read where z is made from it (NONE, DIAG)
template <IcgPl PL>
__global__ __launch_bounds__(NT) void k_icg_direction(IcgMeta m, const IcgPiece *__restrict__ pieces, const double *__restrict__ p_rr,
                                                      const double *__restrict__ r, double *__restrict__ u,
                                                      const int *__restrict__ n_i) {
  __shared__ double sm[NT / 64 + 1];
  const IcgPiece pc = pieces[blockIdx.x];
  if (pc.hi <= pc.lo) return;
  const int d = pc.dom;
  const int dc = m.done_cur[d];
  [[maybe_unused]] const double prev = m.res_cur[d], rho_c = m.rho_cur[d];
  const double *__restrict__ zr = PL == ICG_PL_EXT ? m.z : r;
  int q0 = pc.p0, q1 = pc.p1;   // where the partials of r'z lie
  if constexpr (PL == ICG_PL_EXT) { q0 = m.dom_q0[d]; q1 = m.dom_q1[d]; }
  double zv[4], uv[4];
  [[maybe_unused]] double dv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rw = pc.lo + k * NT + (int)threadIdx.x;
    const bool ok = rw < pc.hi;
    zv[k] = ok ? zr[rw] : 0.0; uv[k] = ok ? u[rw] : 0.0;
    if constexpr (PL == ICG_PL_DIAG) dv[k] = ok ? m.dinv[rw] : 1.0;
  }
  if (dc) return;
  const double rr = icg_dom_sum(p_rr, pc.p0, pc.p1, sm);
  const double res = sqrt(rr);
  double beta, rho = 0.0;
  if constexpr (PL == ICG_PL_NONE) {
    beta = (res * res) / (prev * prev);
  } else {
    if (q1 > q0) rho = icg_dom_sum(PL == ICG_PL_EXT ? m.p_rzq : m.p_rz, q0, q1, sm);   // (the test: see k_icg_start)
    beta = rho / rho_c;
  }
  for (int rw = pc.lo + (int)threadIdx.x, i = 0; rw < pc.hi; rw += NT, ++i) {
    double z_, u_;
    [[maybe_unused]] double d_;
    if (i < 4) {
      z_ = zv[i]; u_ = uv[i];
      if constexpr (PL == ICG_PL_DIAG) d_ = dv[i];
    } else {
      z_ = zr[rw]; u_ = u[rw];
      if constexpr (PL == ICG_PL_DIAG) d_ = m.dinv[rw];
    }
    if constexpr (PL == ICG_PL_DIAG) u[rw] = (d_ * z_) + beta * u_;
    else u[rw] = z_ + beta * u_;
  }
  if (pc.lead && threadIdx.x == 0) icg_dom_next<PL>(m, d, res, rho, n_i);
}

// ---- the same interior CG in 2 launches per iteration (round 2): the config-2 loop above with per-subdomain scalars.
//   k_icg_spmv  : per subdomain: r'r (and r'z) from the partials -> residual, stop test, beta; the CSR-stream SpMV of the NEW
//                 direction u = z + beta u_old computed on the fly from the gathered (u_old, z) pairs; the row owner stores
//                 u_new, c = A u_new, per-block partial u'c.
//   k_icg_update: alpha = rho / u'c; x += alpha u; r -= alpha c; z = r (or dinv .* r: `Pl` = diagonal); per-piece partials.
// A "piece" is a contiguous run of rows of ONE subdomain that also lies inside one XCD's share of the SpMV row blocks, so
// every vector entry is written into the L2 that gathers it next; pieces of a subdomain own consecutive partial slots.
// Subdomain scalars are double-buffered (cur: written by k_icg_update, read by k_icg_spmv; nxt: the other way round);
// a converged subdomain is frozen: both kernels return at once for its workgroups.
struct IcgDomState {
  double rho_prev, tol, res;
  int it, done;
};
struct IcgBlkInfo {       // per SpMV row block, next to its SpmvBlock record: one load instead of a chain of index lookups
  int dom, p0, np, lead;  // subdomain; its partial-slot range (pieces); first block of the subdomain
  int maxit, pad0, pad1, pad2;
};
struct IcgFold {
  const SpmvBlock *blk;
  const IcgBlkInfo *binfo;
  IcgDomState *cur, *nxt;
  double *ur0, *ur1;                     // interleaved (u, z) pairs, two buffers (parity of the subdomain's `it`)
  double *c, *r;
  double *part_uc, *part_rr, *part_rz;
  const double *dinv;                    // nullptr: unpreconditioned
  double reltol;
};
__global__ __launch_bounds__(NT, 8) void k_icg_spmv(int nblocks, IcgFold m, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                 const double *__restrict__ val) {
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  __shared__ double sm[NT / 64 + 1];
  __shared__ double sm2[2 * (NT / 64)];
  const int b = spmv_block_of(nblocks);
  if (b >= nblocks) return;
  const IcgBlkInfo inf = m.binfo[b];
  const SpmvBlock bi = m.blk[b];
  const int d = inf.dom;
  // the subdomain's partials are requested together with its scalars (both addresses come from the block's own record)
  const int p0 = inf.p0, np = inf.np;
  double rr = (int)threadIdx.x < np ? m.part_rr[p0 + threadIdx.x] : 0.0;
  double rz = (m.dinv && (int)threadIdx.x < np) ? m.part_rz[p0 + threadIdx.x] : 0.0;
  const IcgDomState S = m.cur[d];
  if (S.done) return;
  const int r0 = bi.r0, r1 = bi.r1, k0 = bi.k0, nnz = bi.k1 - k0;
  const double2 *ur_old = reinterpret_cast<const double2 *>((S.it & 1) ? m.ur1 : m.ur0);
  double2 *ur_new = reinterpret_cast<double2 *>((S.it & 1) ? m.ur0 : m.ur1);
  constexpr int KPT = SPMV_TILE / NT;
  double vv[KPT];
  double2 gp[KPT];
  const bool fits = nnz <= SPMV_TILE;
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const int k = q * NT + (int)threadIdx.x;
    vv[q] = 0.0; gp[q] = make_double2(0.0, 0.0);
    if (fits && k < nnz) { vv[q] = val[k0 + k]; gp[q] = ur_old[col[k0 + k]]; }
  }
  const int ra = r0 + threadIdx.x;
  int a0 = 0, e0 = 0;
  double2 o0 = make_double2(0.0, 0.0);
  if (ra < r1) { a0 = rowptr[ra] - k0; e0 = rowptr[ra + 1] - k0; o0 = ur_old[ra]; }
  // ---- scalars of this subdomain (identical in all of its workgroups): at most NT pieces per subdomain
  block_sum2_t<NT>(rr, rz, sm2);
  const double res = sqrt(rr);
  const double rho = m.dinv ? rz : res * res;          // IterativeSolvers: residual^2, resp. dot(c, r) with Pl
  const double tol = S.it == 0 ? m.reltol * res : S.tol;
  const bool stop = icg_stop(res, tol, S.it, inf.maxit);  // maxiter = size(A, 2)
  if (inf.lead && threadIdx.x == 0) {
    IcgDomState N;
    N.rho_prev = rho; N.tol = tol; N.res = res; N.it = S.it + (stop ? 0 : 1); N.done = stop;
    m.nxt[d] = N;
  }
  if (stop) return;
  const double beta = rho / S.rho_prev;
  double wy = 0.0;
  if (fits) {
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const int k = q * NT + (int)threadIdx.x;
      if (k < nnz) prod[k] = vv[q] * (beta * gp[q].x + gp[q].y);
    }
    __syncthreads();
    for (int r = ra, i = 0; r < r1; r += NT, ++i) {
      int a, e;
      double2 o;
      if (i == 0) { a = a0; e = e0; o = o0; }
      else { a = rowptr[r] - k0; e = rowptr[r + 1] - k0; o = ur_old[r]; }
      double sum = 0.0;
      for (int k = a; k < e; ++k) sum += prod[k];
      const double un = beta * o.x + o.y;              // u = c + beta u
      m.c[r] = sum;
      ur_new[r].x = un;
      wy += un * sum;
    }
  } else {
    double sum = 0.0;
    for (int t0 = 0; t0 < nnz; t0 += SPMV_TILE) {
      const int mm = min(SPMV_TILE, nnz - t0);
      for (int k = threadIdx.x; k < mm; k += NT) {
        const double2 g = ur_old[col[k0 + t0 + k]];
        prod[k] = val[k0 + t0 + k] * (beta * g.x + g.y);
      }
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < mm; ++k) sum += prod[k];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double2 o = ur_old[r0];
      const double un = beta * o.x + o.y;
      m.c[r0] = sum;
      ur_new[r0].x = un;
      wy = un * sum;
    }
  }
  wy = block_sum(wy, sm);
  if (threadIdx.x == 0) m.part_uc[b] = wy;
}
// One workgroup per piece (pieces[blockIdx.x]; hi <= lo: padding of the XCD interleave).
__global__ __launch_bounds__(NT) void k_icg_update_blk(IcgFold m, const IcgPiece *__restrict__ pieces, double *__restrict__ x) {
  __shared__ double sm[NT / 64 + 1];
  const IcgPiece pc = pieces[blockIdx.x];
  if (pc.hi <= pc.lo) return;
  const int d = pc.dom;
  const IcgDomState N = m.nxt[d];
  const bool lead = pc.lead && threadIdx.x == 0;
  if (N.done) {
    if (lead) { IcgDomState C = N; m.cur[d] = C; }
    return;
  }
  double2 *ur = reinterpret_cast<double2 *>((N.it & 1) ? m.ur1 : m.ur0);   // the pairs k_icg_spmv has just written u into
  double uv[4], cv[4], xv[4], rv[4], dv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rw = pc.lo + k * NT + (int)threadIdx.x;
    const bool ok = rw < pc.hi;
    uv[k] = ok ? ur[rw].x : 0.0; cv[k] = ok ? m.c[rw] : 0.0; xv[k] = ok ? x[rw] : 0.0; rv[k] = ok ? m.r[rw] : 0.0;
    dv[k] = ok && m.dinv ? m.dinv[rw] : 1.0;
  }
  const double uc = icg_dom_sum(m.part_uc, pc.b0, pc.b1, sm);
  const double alpha = N.rho_prev / uc;                 // nxt.rho_prev holds this iteration's rho
  if (lead) { IcgDomState C = N; C.done = 0; m.cur[d] = C; }
  double srr = 0.0, srz = 0.0;
  for (int rw = pc.lo + (int)threadIdx.x, i = 0; rw < pc.hi; rw += NT, ++i) {
    double u_, c_, x_, r_, d_;
    if (i < 4) { u_ = uv[i]; c_ = cv[i]; x_ = xv[i]; r_ = rv[i]; d_ = dv[i]; }
    else { u_ = ur[rw].x; c_ = m.c[rw]; x_ = x[rw]; r_ = m.r[rw]; d_ = m.dinv ? m.dinv[rw] : 1.0; }
    x[rw] = x_ + alpha * u_;
    const double ri = r_ - alpha * c_;
    m.r[rw] = ri;
    const double zi = m.dinv ? d_ * ri : ri;
    ur[rw].y = zi;
    srr += ri * ri;
    srz += ri * zi;
  }
  srr = block_sum(srr, sm);
  srz = block_sum(srz, sm);
  if (threadIdx.x == 0) { m.part_rr[pc.slot] = srr; m.part_rz[pc.slot] = srz; }
}
// x = 0, r = rhs, pairs (0, z_0) into buffer 0, partials of r'r / r'z; the lead piece of a subdomain resets its scalars
__global__ __launch_bounds__(NT) void k_icg_fold_init(IcgFold m, const IcgPiece *__restrict__ pieces, const double *__restrict__ rhs,
                                                      double *__restrict__ x) {
  __shared__ double sm[NT / 64 + 1];
  const IcgPiece pc = pieces[blockIdx.x];
  if (pc.hi <= pc.lo) return;
  double2 *ur = reinterpret_cast<double2 *>(m.ur0);
  double srr = 0.0, srz = 0.0;
  for (int rw = pc.lo + (int)threadIdx.x; rw < pc.hi; rw += NT) {
    const double ri = rhs[rw];
    const double zi = m.dinv ? m.dinv[rw] * ri : ri;
    x[rw] = 0.0; m.r[rw] = ri;
    ur[rw] = make_double2(0.0, zi);
    srr += ri * ri; srz += ri * zi;
  }
  srr = block_sum(srr, sm);
  srz = block_sum(srz, sm);
  if (threadIdx.x == 0) {
    m.part_rr[pc.slot] = srr; m.part_rz[pc.slot] = srz;
    if (pc.lead) {
      IcgDomState C;
      C.rho_prev = 1.0; C.tol = 0.0; C.res = 0.0; C.it = 0; C.done = 0;
      m.cur[pc.dom] = C; m.nxt[pc.dom] = C;
    }
  }
}

// dinv[r] = 1 / A[r,r] of a CSR matrix (1 if the row stores no diagonal entry)
__global__ __launch_bounds__(NT) void k_csr_inv_diag(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                     const double *__restrict__ val, double *__restrict__ dinv) {
  const int r = blockIdx.x * NT + threadIdx.x;
  if (r >= n) return;
  double dg = 1.0;
  for (int k = rowptr[r]; k < rowptr[r + 1]; ++k)
    if (col[k] == r) dg = 1.0 / val[k];
  dinv[r] = dg;
}

// ------------------------------------------------------------------ batched dense GEMV with fused gather
// y_d = M_d * (D_d R_d x)  [* D_d], for all subdomains d of this rank in one launch.
//   S-apply  (SCALE=false): M_d = S_d,  EPDD.jl:775-778  (gather, `Sd[idom]*xd`)
//   NN-apply (SCALE=true) : M_d = ΠS_d, EPDD.jl:1373-1381 (gather r/cnt, `ΠSd[idom]*rd`, result /cnt)
// Layout: every M_d is stored row-major with its leading dimension padded to a multiple of 16
// doubles (128 B), so each row is a contiguous, line-aligned stream. A workgroup owns RPW rows per
// wave (WAVES*RPW rows, 32 by default) described by ONE 32-byte tile record. The operand gather
// (index -> x, two dependent loads) is requested first and the first group of matrix loads right
// behind it — vector-memory results return in issue order — so the stream is in flight while x_d is
// staged into LDS (padded with zeros); then one group of 4 x 16 B per lane and row at a time, 16 waves
// per CU keeping 128 KB in flight. Each lane multiplies against the LDS copy of x_d and the row sum is
// finished with a wave shuffle tree.
// Output: row r of subdomain d goes to out_pos[...] = g*W + j, the j-th contribution slot of Γ node
// g (slots in ascending subdomain order, W = max multiplicity; unused slots stay 0). The
// scatter-add over subdomains `Sx[lΓ] += Sdxd[lΓd]` (EPDD.jl:779-781 / 1379-1381) is then a
// contiguous W-term sum per Γ node, taken by the consumer kernel in the reference's idom order.
struct DenseMeta {
  const void *M;          // all blocks of this rank, row-major, padded: doubles, or floats for fp32-stored blocks (GemvRows<RPW, MT>)
  const GemvTile *tiles;  // [ntiles]
  const int *gidx;        // [nloc] Γ index of every local row/column
  const double *cnt;      // [nloc] node_Γ_cnt as double (NN only)
  const int *out_pos;     // [nloc] slot g*W + j of every local row
};
#ifndef MI355_OPERAND_FIRST
#define MI355_OPERAND_FIRST 1   // 0: matrix stream first (measured 7 % slower in the folded PCG launches)
#endif
#ifndef MI355_GEMV_GU
#define MI355_GEMV_GU 4        // 16-byte loads per lane and row in one group (2 and 8 measured slower, profiles/)
#endif
constexpr int GU = MI355_GEMV_GU;
#ifndef MI355_GEMV_GU_F32
// ... of the fp32-stored blocks. 2, not 4: a group then covers 512 columns like the fp64 group, and its operand (4 doubles
// per load from LDS) and widened floats fit. With 4 the default PHASE 1 launch k_gemv_pcg<2,1,2,16,false,float> sat at the
// 128-VGPR cap of a 1024-thread workgroup with 16 VGPRs spilled (60 B/lane of scratch) and k_gemv_batched<2,true,16,float>
// took 125 VGPRs (4 waves/SIMD); with 2: 109 VGPRs, no scratch (fp64 twin: 102) and 62 VGPRs, 8 waves/SIMD (fp64: 78, 6).
#define MI355_GEMV_GU_F32 2
#endif
// Default-policy loads on purpose: the 136 MB working set of a PCG iteration is re-read from the Infinity
// Cache every iteration; non-temporal loads made the stand-alone GEMV 3 % faster and the solve 4 % slower.
// Storage type MT of a block: double (two columns per 16-byte load, 128 columns per wave load) or float (four columns per
// load, 256 per wave load: the fp32-stored Neumann-Neumann blocks, MI_STORE_F32). A float is widened in registers
// (v_cvt_f64_f32, exact) and multiplied against the same fp64 LDS copy of x_d: fp32 is a storage format, every product and
// sum stays fp64. Per row the accumulation order is fixed by (lane, load, column), whatever the tiling.
template <typename MT> struct GemvElem;
template <> struct GemvElem<double> {
  using Vec = double2; static constexpr int CPL = 2; static constexpr int G = GU;
  static __device__ __forceinline__ double2 zero() { return make_double2(0.0, 0.0); }
};
template <> struct GemvElem<float> {
  using Vec = float4; static constexpr int CPL = 4; static constexpr int G = MI355_GEMV_GU_F32;
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <typename MT> constexpr int gemv_wave_cols() { return 64 * GemvElem<MT>::CPL; }   // columns of one wave load
template <typename MT>
__device__ __forceinline__ typename GemvElem<MT>::Vec gemv_ld(const MT *p) { return *reinterpret_cast<const typename GemvElem<MT>::Vec *>(p); }
template <int RPW, typename MT>
__device__ __forceinline__ void gemv_load_group(typename GemvElem<MT>::Vec (&mv)[RPW][GemvElem<MT>::G], const MT *const (&rowp)[RPW], int col0,
                                                int cb, int pw, int lane) {
#pragma unroll
  for (int u = 0; u < GemvElem<MT>::G; ++u) {
    const int c = cb + u * gemv_wave_cols<MT>() + lane * GemvElem<MT>::CPL;
#pragma unroll
    for (int k = 0; k < RPW; ++k)
      mv[k][u] = (c < pw) ? gemv_ld<MT>(rowp[k] + col0 + c) : GemvElem<MT>::zero();
  }
}
template <int RPW>
__device__ __forceinline__ void gemv_fma_group(double (&acc)[RPW], const double2 (&mv)[RPW][GU], const double *xs, int cb,
                                               int pw, int lane) {
#pragma unroll
  for (int u = 0; u < GU; ++u) {
    const int c = cb + u * 128 + lane * 2;
    const double2 xv = (c < pw) ? *reinterpret_cast<const double2 *>(&xs[c]) : make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      acc[k] += mv[k][u].x * xv.x;
      acc[k] += mv[k][u].y * xv.y;
    }
  }
}
template <int RPW>
__device__ __forceinline__ void gemv_fma_group(double (&acc)[RPW], const float4 (&mv)[RPW][GemvElem<float>::G], const double *xs, int cb,
                                               int pw, int lane) {
#pragma unroll
  for (int u = 0; u < GemvElem<float>::G; ++u) {
    const int c = cb + u * 256 + lane * 4;   // (pw is a multiple of 32: c < pw covers c + 3)
    const double2 xa = (c < pw) ? *reinterpret_cast<const double2 *>(&xs[c]) : make_double2(0.0, 0.0);
    const double2 xb = (c < pw) ? *reinterpret_cast<const double2 *>(&xs[c + 2]) : make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      acc[k] += (double)mv[k][u].x * xa.x;
      acc[k] += (double)mv[k][u].y * xa.y;
      acc[k] += (double)mv[k][u].z * xb.x;
      acc[k] += (double)mv[k][u].w * xb.y;
    }
  }
}
// Row streamer of one tile: RPW rows per wave, 16 B per lane and row per load, groups of 4 loads.
// `begin` issues the first group of matrix loads (so the stream is in flight while the caller
// stages the column values into LDS), `panel` consumes one staged panel, `finish` reduces.
template <int RPW, typename MT = double>
struct GemvRows {
  using Vec = typename GemvElem<MT>::Vec;
  static constexpr int GROUP_COLS = gemv_wave_cols<MT>() * GemvElem<MT>::G;
  const MT *rowp[RPW];
  double acc[RPW];
  Vec buf[RPW][GemvElem<MT>::G];
  int lane, ld;
  __device__ __forceinline__ void begin(const DenseMeta &m, const GemvTile &t) { begin(m.M, t); }
  __device__ __forceinline__ void begin(const void *M, const GemvTile &t) {   // M = DenseMeta::M
    lane = threadIdx.x & 63;
    ld = t.ld;
    const int row_base = t.row0 + (threadIdx.x >> 6) * RPW;
    const MT *Md = static_cast<const MT *>(M) + t.mat_off;   // (mat_off and ld count elements of the storage type)
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      const int r = min(row_base + k, t.n - 1);  // clamp: tail rows re-read a valid row, result dropped
      rowp[k] = Md + (long long)r * ld;
      acc[k] = 0.0;
    }
    gemv_load_group<RPW, MT>(buf, rowp, 0, 0, min(GEMV_PANEL, ld), lane);
  }
  // xs holds columns [c0, c0 + pw) of the operand; for c0 > 0 the first group is loaded here
  __device__ __forceinline__ void panel(const double *xs, int c0, int pw) {
    if (c0) gemv_load_group<RPW, MT>(buf, rowp, c0, 0, pw, lane);
    for (int cb = 0; cb < pw; cb += GROUP_COLS) {
      if (cb) gemv_load_group<RPW, MT>(buf, rowp, c0, cb, pw, lane);
      gemv_fma_group<RPW>(acc, buf, xs, cb, pw, lane);
    }
  }
  __device__ __forceinline__ void finish(double (&sum)[RPW]) {
#pragma unroll
    for (int k = 0; k < RPW; ++k) sum[k] = wave_sum(acc[k]);  // valid in lane 0
  }
};

// Arguments: the fields of DenseMeta as plain pointers, the seven the head of the launch dereferences first (14 dwords:
// what kernel-argument preload delivers in SGPRs at wave start; a struct passed by value is never preloaded).
template <int RPW, bool SCALE, int WAVES, typename MT = double>
__global__ __launch_bounds__(64 * WAVES) void k_gemv_batched(const GemvTile *tiles, const int *done, const int *zero_x,
                                                             const int *__restrict__ gidx, const double *__restrict__ x,
                                                             const double *__restrict__ cnt, const void *M,
                                                             double *__restrict__ yslots, const int *__restrict__ out_pos) {
  constexpr int NTH = 64 * WAVES;
  // tile record and both flags in ONE memory round trip (tested one after the other they cost three, 1.2-2 us each)
  const GemvTile t = tiles[blockIdx.x];
  const int done0 = done ? *done : 0, zero0 = zero_x ? *zero_x : 0;
  asm volatile("" ::"s"(t.mat_off), "s"(t.n), "s"(t.ld), "s"(t.loc_off), "s"(t.row0), "s"(t.active), "s"(done0), "s"(zero0),
               "s"(yslots), "s"(out_pos));   // (the two arguments behind the preloaded ones: requested in the same batch)
  if (done0) return;
  __shared__ __attribute__((aligned(16))) double xs[GEMV_PANEL];
  if (!t.active) return;
  const int off = t.loc_off, n = t.n;
  if (zero0) {  // x is identically zero (set-up of a solve from x0 = 0): the products are +0, nothing to stream
    const int row_base = t.row0 + (threadIdx.x >> 6) * RPW;
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < RPW; ++k)
        if (row_base + k < n) yslots[out_pos[off + row_base + k]] = 0.0;
    return;
  }
  GemvRows<RPW, MT> rows;
#if !MI355_OPERAND_FIRST
  rows.begin(M, t);
#endif
  for (int c0 = 0; c0 < t.ld; c0 += GEMV_PANEL) {
    const int pw = min(GEMV_PANEL, t.ld - c0);  // multiple of 16
    if (c0) __syncthreads();
#if MI355_OPERAND_FIRST
    // Vector-memory results return in issue order: the operand gather (index -> value, two dependent loads) is issued
    // BEFORE the first group of the matrix stream, so staging waits for its own loads only, not for 128 KB of matrix.
    constexpr int XPT = (GEMV_PANEL + NTH - 1) / NTH;
    int gi[XPT];
#pragma unroll
    for (int q = 0; q < XPT; ++q) {
      const int j = c0 + q * NTH + (int)threadIdx.x;
      gi[q] = (q * NTH + (int)threadIdx.x < pw && j < n) ? gidx[off + j] : -1;
    }
    double xv[XPT];
#pragma unroll
    for (int q = 0; q < XPT; ++q) {
      const int j = c0 + q * NTH + (int)threadIdx.x;
      xv[q] = 0.0;
      if (gi[q] >= 0) {
        xv[q] = x[gi[q]];
        if (SCALE) xv[q] = xv[q] / cnt[off + j];
      }
    }
    if (c0 == 0) rows.begin(M, t);
#pragma unroll
    for (int q = 0; q < XPT; ++q) {
      const int l = q * NTH + (int)threadIdx.x;
      if (l < pw) xs[l] = xv[q];
    }
#else
    for (int l = threadIdx.x; l < pw; l += NTH) {
      const int j = c0 + l;
      double v = 0.0;
      if (j < n) {
        v = x[gidx[off + j]];
        if (SCALE) v = v / cnt[off + j];
      }
      xs[l] = v;
    }
#endif
    __syncthreads();
    rows.panel(xs, c0, pw);
  }
  double sum[RPW];
  rows.finish(sum);
  const int row_base = t.row0 + (threadIdx.x >> 6) * RPW;
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int r = row_base + k;
    if (rows.lane == 0 && r < n) yslots[out_pos[off + r]] = SCALE ? sum[k] / cnt[off + r] : sum[k];
  }
}

// The same GEMV for KV operand vectors at once: S_d is streamed ONCE for up to KV columns of X (`WtA[i,:] = A*W[:,i]`
// of the deflated solvers, defcg.jl:41-44 / 261-264; `AV[:, j] = A*V[:, j]` of eigpcg's restart, eigcg.jl:233-240) instead of once
// per column. Per (row, vector) the products are accumulated in the order of k_gemv_batched: results are bit-identical
// to KV single applies. X is column-major with leading dimension ldx; vector v writes its slot table at v*slot_stride.
template <int RPW, int KV, bool SCALE, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_gemv_multi(const GemvTile *tiles, const int *__restrict__ gidx,
                                                           const double *__restrict__ X, const double *__restrict__ cnt,
                                                           const double *__restrict__ M, long long ldx, int kv,
                                                           double *__restrict__ yslots, long long slot_stride,
                                                           const int *__restrict__ out_pos) {   // (DenseMeta's fields; 13 dwords preloaded)
  constexpr int NTH = 64 * WAVES;
  __shared__ __attribute__((aligned(16))) double xs[KV][GEMV_PANEL];
  const GemvTile t = tiles[blockIdx.x];
  if (!t.active) return;
  const int off = t.loc_off, n = t.n, lane = threadIdx.x & 63;
  const int row_base = t.row0 + (threadIdx.x >> 6) * RPW;
  const double *rowp[RPW];
  double acc[RPW][KV];
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    rowp[k] = M + t.mat_off + (long long)min(row_base + k, n - 1) * t.ld;   // (fp64 storage only)
#pragma unroll
    for (int v = 0; v < KV; ++v) acc[k][v] = 0.0;
  }
  for (int c0 = 0; c0 < t.ld; c0 += GEMV_PANEL) {
    const int pw = min(GEMV_PANEL, t.ld - c0);
    if (c0) __syncthreads();
    for (int l = threadIdx.x; l < pw; l += NTH) {
      const int j = c0 + l;
      const int gi = j < n ? gidx[off + j] : -1;
      const double cn = (SCALE && j < n) ? cnt[off + j] : 1.0;
#pragma unroll
      for (int v = 0; v < KV; ++v) {
        double xv = 0.0;
        if (gi >= 0 && v < kv) {
          xv = X[(long long)v * ldx + gi];
          if (SCALE) xv = xv / cn;
        }
        xs[v][l] = xv;
      }
    }
    __syncthreads();
    double2 buf[RPW][GU];
    for (int cb = 0; cb < pw; cb += 128 * GU) {
      gemv_load_group<RPW, double>(buf, rowp, c0, cb, pw, lane);
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int c = cb + u * 128 + lane * 2;
        if (c < pw) {
#pragma unroll
          for (int v = 0; v < KV; ++v) {
            const double2 xv = *reinterpret_cast<const double2 *>(&xs[v][c]);
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
              acc[k][v] += buf[k][u].x * xv.x;
              acc[k][v] += buf[k][u].y * xv.y;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int r = row_base + k;
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      const double sum = wave_sum(acc[k][v]);
      if (lane == 0 && r < n && v < kv)
        yslots[(long long)v * slot_stride + out_pos[off + r]] = SCALE ? sum / cnt[off + r] : sum;
    }
  }
}
// Γ-sum of the slot tables of k_gemv_multi: grid (x, kv); vector v -> Y[:, v] (leading dimension ldy)
__global__ __launch_bounds__(NT) void k_assemble_slots_multi(int n, int width, const double *__restrict__ yslots,
                                                             long long slot_stride, double *__restrict__ Y, long long ldy) {
  const double *ys = yslots + (long long)blockIdx.y * slot_stride;
  double *y = Y + (long long)blockIdx.y * ldy;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    double s = 0.0;
    for (int j = 0; j < width; ++j) s += ys[(long long)i * width + j];
    y[i] = s;
  }
}

// ------------------------------------------------------------------ PCG folded into the two GEMVs (2 launches / iteration)
// For pcg(S, b, x, ΠSnn) with both operators dense and built on the same subdomain maps, the vector
// work of an iteration is folded into the prologue/epilogue of the two GEMV launches:
//
//   PHASE 1 (ΠS GEMV): d = Σ partial(p'Ap); alpha = r'z / d (cg.jl:94-95); r_new = r - alpha Ap for this
//            workgroup's columns (Ap = Γ-sum of the S contributions) -> LDS, scaled by 1/cnt; the workgroup that
//            owns a Γ node (first contributing subdomain) stores r_new, x += alpha p (cg.jl:97-98); GEMV;
//            epilogue: z contributions, partial r'z and partial r'r (cg.jl:99-101).
//   PHASE 0 (S GEMV):  r'r, r'z from the partials; it += 1; res_norm[it] = sqrt(r'r); stop rule (cg.jl:91,
//            104-105) — evaluated identically by every workgroup; beta = (1/old)*new; p_new = beta p + z for this
//            workgroup's columns (z = Γ-sum of the ΠS contributions) -> LDS (cg.jl:102-103); owners store p_new;
//            GEMV; epilogue: S contributions, partial p'Ap (cg.jl:93-94).
//
// A dot product is therefore summed per GEMV row and then over tiles (Σ_d Σ_rows p_g y_row = Σ_g p_g Σ_d y),
// a re-association of the same terms.
// Everything the prologue reads is kept in LOCAL order (one entry per (subdomain, Γ_d slot)), so the
// loads of a workgroup are contiguous and need no index chain: a producer writes its row result
// into the contribution row of every subdomain that shares the Γ node (`tgt`, <= W tiny stores), and
// the owner of a node writes the updated vector entry into every sharing subdomain's copy (`peer`).
// r and p have a "current" copy (read by everyone) and a "next" copy (written by owners); the owners
// of the following launch copy next -> current, so no launch reads a buffer it writes. Scalars follow
// the same rule (it/it_nxt, rTz/rTz_prev).
// Start-up: it_nxt = 0 marks the first PHASE 1 launch (alpha = 0, so r_new = r_0 and x is untouched;
// p = 0 and rTz_prev = 1 make the first PHASE 0 produce p = z_0, it = 1, res_norm[1] = ||r_0||).
struct PcgFold {
  // ---- what the head of a launch needs, contiguous at the front: with DenseMeta ahead of it in the kernel-argument segment
  // these are fetched by ONE batch of scalar loads, issued together with the tile record and the state block (k_gemv_pcg)
  int n_in;
  int W;
  // deflation (defcg.jl:291-305; nvec == 0: plain pcg). PHASE 1 also leaves per-tile partials of WtA*z; k_defl_mu turns
  // them into mu = WtAW \ (WtA*z) and (W*mu) in local order; PHASE 0 subtracts that from beta*p + z.
  int nvec;
  int dbg_wg;               // MI355_FOLD_DEBUG: the workgroup that writes stamps (tested at the first stamp, right behind the exit)
  // inputs that come out of a peer exchange (exchange.hpp) are double-buffered by the parity of the exchange number:
  // con_in / part_in0 / part_in1 point at copy 0, copy (*in_epoch & 1) is in_stride doubles further
  long long in_stride;
  long long *dbg;           // MI355_FOLD_DEBUG: wall-clock stamps of workgroup dbg_wg, 8 per launch (tools/fold_stamps.py)
  const double *r_gamma;    // [n_Γ] r_0 in Γ order: the first PHASE 1 launch gathers it (no separate scatter pass)
  const int *jrank;         // [nloc] rank of this subdomain among the contributors of the node (0 = owner)
  const int *peer;          // [nloc*W] local positions of the same Γ node in the sharing subdomains (-1 pad)
  const int *tgt;           // [nloc*W] where this row's result goes in each sharing subdomain's contribution row (-1 pad)
  double *r_cur, *r_nxt, *p_cur, *p_nxt;  // [nloc] local-order copies
  double *x;                // [n_Γ]
  const double *wm_loc;     // [nloc] (W*mu)[gidx[loc]]
  // ---- used after the operand is staged
  double *con_out;          // [nloc*W]
  double *part_out0;        // PHASE 1: partial r'r          PHASE 0: partial p'Ap
  double *part_out1;        // PHASE 1: partial r'z
  double *res_norm;
  long long n_gamma;
  const double *AW;         // [nvec * n_Γ] WtA[v, :] = A*W[:, v], Γ order
  double *part_mu;          // [nvec * ntiles(ΠS)] layout v * ntiles + tile
  // ---- passed to the kernel as leading plain parameters (preloaded into SGPRs at wave start); the kernel does not read
  // these copies, the launch (operators.hpp: gemv_pcg) takes them from here
  SolverState *st;
  const double *con_in;     // [nloc*W] contributions to sum: S (PHASE 1) / ΠS (PHASE 0), local order
  const double *part_in0;   // PHASE 1: partial p'Ap         PHASE 0: partial r'r
  const double *part_in1;   //                               PHASE 0: partial r'z
  const unsigned long long *in_epoch;
  // ---- peer exchange
  // outputs of a launch that is sharded over ranks and exchanged by peer stores (exchange.hpp): con_out / part_out0 /
  // part_out1 then point at copy 0 of the table in the OWN arena; every streamed tile stores its results into copy
  // ((epoch + 1) & 1) of the table in EVERY arena, publishes them and counts itself in; the last of the n_arrive tiles
  // stores exchange number epoch + 1 into this rank's flag of every arena. The wait (and the advance of `epoch`) is a
  // one-wave kernel behind the launch — a streaming launch never spins.
  const XchgPeers *xp;      // device copy (null: outputs stay local)
  XchgState *xst;
  long long out_stride;
  unsigned int n_arrive;
  // x_inwait (every rank on a GPU of its own — a waiting launch keeps its compute units): no kernel between the launches.
  // A launch whose inputs come out of an exchange (in_stride != 0) waits for the flags itself, with its first matrix loads
  // already in flight. The exchange number is then carried like it / it_nxt: a PHASE p launch reads xst->xep[p] and its
  // lead thread writes xst->xep[1 - p] (the launches alternate), so no workgroup reads a word its own launch writes.
  int x_inwait;
  const XchgPeers *xpw;     // peers to wait for (device copy)
  // launch of an operator that is sharded over ranks (XCHG kernels only): the partials are summed by PART_LANES threads,
  // so that ranks that chose different tilings for their slices associate the sum alike
  int canon;
  // ---- exit
  // whole-solve graphs: the PHASE 0 launch that meets the stop rule hands the results to the host itself (block 0),
  // so that the host is released before this launch and the graph's tail have drained
  const SolveArgs *exit_args;
  PinnedFlags *exit_flags;
};
constexpr int PART_LANES = 256;   // the smallest workgroup of the folded launches (4 waves)
#define MI_FSTAMP(i) \
  do { if (dbg && (int)blockIdx.x == dbg_wg && threadIdx.x == 0) dbg[dbg_row * 8 + (i)] = wall_clock64(); } while (0)
__device__ __forceinline__ double slot_sum(const double *slots, int g, int W) {
  double s = 0.0;
  if (W == 4) {
    const double4 q = *reinterpret_cast<const double4 *>(slots + 4ll * g);
    s += q.x; s += q.y; s += q.z; s += q.w;
  } else if (W == 2) {
    const double2 q = *reinterpret_cast<const double2 *>(slots + 2ll * g);
    s += q.x; s += q.y;
  } else {
    for (int j = 0; j < W; ++j) s += slots[(long long)g * W + j];
  }
  return s;
}

// FOLD_CPT = columns per thread staged in registers: the launch needs max n_Γd <= FOLD_CPT * 64 * WAVES (<= GEMV_PANEL)
// XCHG = false compiles every peer-exchange branch out: the single-GPU launches are the kernel they were before.
// MT = float: the blocks of this launch are stored as fp32 (PHASE 1, XCHG = false only: the Neumann-Neumann launch).
// Arguments: the seven pointers in front of the structs are the 14 dwords gfx950 delivers in SGPRs when a wave starts
// (kernel-argument preload, csrc/Makefile PRELOAD; a struct passed by value is never preloaded): what the first loads
// of a launch dereference — tile record, state block, the partials and contributions to sum, the current copy of the
// phase's vector (`vec_cur`: r_cur for PHASE 1, p_cur for PHASE 0), the exchange parity. The body reads these, not the
// copies in `m` / `f`. (n_in and W would be dwords 15 and 16: they come with the one batch below instead — `in_epoch` has
// to be dereferenced before the first vector load and would otherwise cost a sharded solve a round trip of its own.)
template <int RPW, int PHASE, int FOLD_CPT, int WAVES, bool XCHG, typename MT = double>
__global__ __launch_bounds__(64 * WAVES) void k_gemv_pcg(const GemvTile *tiles, SolverState *st, const double *part_in0_,
                                                         const double *part_in1_, const double *con_in_, const double *vec_cur,
                                                         const unsigned long long *in_epoch, DenseMeta m, PcgFold f) {
  constexpr int NTH = 64 * WAVES, NR = WAVES * RPW;  // threads and rows per workgroup
  const bool x_push = XCHG && f.xp != nullptr, x_inwait = XCHG && f.x_inwait != 0;
  // The tile record and the state block are requested together, before the stop flag is looked at (one memory round trip
  // instead of two at the top of every launch; the empty asm takes them all as inputs — without it the compiler sinks
  // every load but `done` below the early exit). Their addresses are in registers when the wave starts, and every other
  // kernel argument the prologue needs is requested in the same batch: one scalar wait ahead of the first vector load.
  const GemvTile t = tiles[blockIdx.x];
  const int done0 = st->done;
  const long long it0 = st->it, it_nxt0 = st->it_nxt, maxit = st->maxit, cap = st->res_cap;
  const double tol = st->tol, rTz0 = st->rTz, old = st->rTz_prev;
  const unsigned long long xo = XCHG && f.xst ? (x_inwait ? f.xst->xep[PHASE] : f.xst->epoch) : 0ull;   // (same round trip as the state block)
  const unsigned long long xe = x_inwait ? xo : (in_epoch ? *in_epoch : 0ull);
  const int n_in = f.n_in, W = f.W, nvec = f.nvec;
  const long long in_stride = f.in_stride;
  const void *const Mp = m.M;
  const int *const gidx = m.gidx, *const jrank = f.jrank, *const peer = f.peer, *const tgt = f.tgt;
  const double *const cntp = m.cnt, *const r_gamma = f.r_gamma, *const vec_nxt = PHASE == 1 ? f.p_nxt : f.r_nxt;
  double *const xg = f.x;
  // (two statements: an asm takes 30 operands at most. The first holds the kernel arguments of the prologue, the debug
  // stamps' included — MI_FSTAMP(0) tests them right behind the exit — and, for PHASE 1, of the epilogue's stores.)
  double *const con_out = f.con_out, *const part_out0 = f.part_out0, *const part_out1 = PHASE == 1 ? f.part_out1 : nullptr;
  long long *const dbg = f.dbg;
  const int dbg_wg = f.dbg_wg;
  const double *const AW = PHASE == 1 ? f.AW : nullptr;
  double *const part_mu = PHASE == 1 ? f.part_mu : nullptr;
  const long long n_gamma = f.n_gamma;
  if constexpr (!XCHG)   // (the launches with peer exchange keep the compiler's placement: some of them sit at a VGPR step of the occupancy)
    asm volatile("" ::"s"(n_in), "s"(W), "s"(nvec), "s"(in_stride), "s"(Mp), "s"(gidx), "s"(cntp), "s"(jrank), "s"(peer), "s"(tgt),
                 "s"(r_gamma), "s"(vec_nxt), "s"(xg), "s"(dbg), "s"(dbg_wg), "s"(con_out), "s"(part_out0), "s"(part_out1), "s"(AW),
                 "s"(part_mu), "s"(n_gamma));
  asm volatile("" ::"s"(t.mat_off), "s"(t.n), "s"(t.ld), "s"(t.loc_off), "s"(t.row0), "s"(t.active), "s"(t.nrows), "s"(it0),
               "s"(it_nxt0), "s"(maxit), "s"(cap), "s"(tol), "s"(rTz0), "s"(old), "s"(done0), "s"(xe), "s"(xo));
  if (done0) return;
  GemvRows<RPW, MT> rows;
  if (x_inwait && in_stride) {
    // the tables this launch reads are complete when every rank's flag in the own arena has reached the exchange number
    if (t.active) rows.begin(Mp, t);      // (the matrix does not depend on them: its first loads travel while the flags are polled)
    if (threadIdx.x < 64) xchg_wait(f.xst, *f.xpw, xo);
    __syncthreads();
    // (the tables sit in fine-grained memory — no level of cache keeps their lines across the peers' stores; the vector
    // caches were emptied when this launch began and have not seen the tables since)
    if (__hip_atomic_load(&f.xst->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // expired: the solve fails with MI_ERR_COMM
  }
  const bool streaming = x_inwait && in_stride;
  const long long xoff = (long long)(xe & 1ull) * in_stride;
  const double *con_in = con_in_ + xoff, *part_in0 = part_in0_ + xoff, *part_in1 = PHASE == 0 ? part_in1_ + xoff : nullptr;
  __shared__ __attribute__((aligned(16))) double xs[GEMV_PANEL];
  __shared__ double sm[2 * (NTH / 64)];
  __shared__ double rowv[NR], rowc0[NR], rowc1[NR];
  __shared__ double rowy[NR];   // deflation: the rows' z-contributions
  __shared__ int rowg[NR];      //            and their Γ indices
  const int off = t.loc_off, n = t.n;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (threadIdx.x < NR) { rowc0[threadIdx.x] = 0.0; rowv[threadIdx.x] = 0.0; rowy[threadIdx.x] = 0.0; rowg[threadIdx.x] = 0; }  // visible after the barrier of the sums
#if !MI355_OPERAND_FIRST
  if (t.active && !streaming) rows.begin(Mp, t);  // matrix stream in flight from here on
#endif

  // ---- every load of the prologue is issued before the first barrier (one memory round trip), all contiguous
  const bool first1 = PHASE == 1 && it_nxt0 == 0;  // very first launch of a solve: r_0 comes from the Γ-ordered vector, p = 0
  const int dbg_row = (int)((PHASE == 1 ? 2 * it_nxt0 : 2 * it0 + 1) & 63);
  MI_FSTAMP(0);
  double pa = 0.0, pb = 0.0;
  // Threads that sum the partials. A launch whose tiling is this rank's own (sharded operator) must not let its thread count
  // decide how the sum is associated — alpha, beta and the stop rule would then differ between the ranks in the last bits:
  // its first PART_LANES threads sum, whatever WAVES is (the other waves add zeros to the tree below: exact).
  const int SL = XCHG && f.canon ? PART_LANES : NTH;
  for (int i0 = XCHG && f.canon && threadIdx.x >= PART_LANES ? n_in : (int)threadIdx.x; i0 < n_in; i0 += 8 * SL) {  // up to eight partials in flight per thread, added in order
    double ta[8], tb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k * SL;
      ta[k] = i < n_in ? part_in0[i] : 0.0;
      tb[k] = PHASE == 0 && i < n_in ? part_in1[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { pa += ta[k]; if (PHASE == 0) pb += tb[k]; }
  }
  double cv[FOLD_CPT], cs[FOLD_CPT], cc[FOLD_CPT];  // vector value, Γ-sum of the contributions, cnt (PHASE 0: W*mu) — per column
#pragma unroll
  for (int q = 0; q < FOLD_CPT; ++q) {
    const int j = q * NTH + threadIdx.x;
    cv[q] = cs[q] = 0.0; cc[q] = PHASE == 1 ? 1.0 : 0.0;
    if (j < n) {
      const int loc = off + j;
      cs[q] = slot_sum(con_in, loc, W);
      if (PHASE == 1) { cv[q] = first1 ? r_gamma[gidx[loc]] : vec_cur[loc]; cc[q] = cntp[loc]; }
      else { cv[q] = vec_cur[loc]; if (nvec > 0) cc[q] = f.wm_loc[loc]; }
    }
  }
  // The thread whose column j is also a row of this tile serves that row (at most one column per thread:
  // the rows of a tile are consecutive and fewer than the threads). Its owner duties need p/r of the node, x[g] and the peer list: load now.
  int o_q = -1, o_g = 0;
  bool o_own = false;
  double o_a = 0.0, o_x = 0.0;  // PHASE 1: p (next copy), x[g]    PHASE 0: r (next copy)
  int o_peer[4] = {-1, -1, -1, -1};
#pragma unroll
  for (int q = 0; q < FOLD_CPT; ++q) {
    const int j = q * NTH + threadIdx.x, ri = j - t.row0;
    if (j < n && ri >= 0 && ri < t.nrows) {
      const int loc = off + j;
      o_q = q;
      // everything an owner needs is requested unconditionally (a load behind `if (owner)` would wait for jrank first:
      // a second memory round trip on the way to the operand barrier); x[g] — a dependent load — is consumed only in the
      // epilogue, after the matrix stream
      o_own = jrank[loc] == 0;
      if (PHASE == 1) { o_a = first1 ? 0.0 : vec_nxt[loc]; o_g = gidx[loc]; }
      else o_a = vec_nxt[loc];
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < W) o_peer[k] = peer[loc * W + k];
    }
  }
  if (PHASE == 1 && o_q >= 0 && o_own) o_x = xg[o_g];
  // lane 0 of every wave stores the results of its RPW rows into the contribution rows of all sharing subdomains
  int e_tgt[RPW][4];
  double e_cnt[RPW];
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int r = t.row0 + (int)(threadIdx.x >> 6) * RPW + k;
    e_cnt[k] = 1.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) e_tgt[k][q] = -1;
    if ((threadIdx.x & 63) == 0 && r < n) {
      const int loc = off + r;
      if (PHASE == 1) e_cnt[k] = cntp[loc];
#pragma unroll
      for (int q = 0; q < 4; ++q) if (q < W) e_tgt[k][q] = tgt[loc * W + q];
    }
  }

  // peer stores of the results: thread i < 4*NR serves slot (i & 3) of row (i >> 2) of this tile, in every arena
  int x_tgt = -1;
  if (x_push && t.active && threadIdx.x < 4 * NR) {
    const int r = t.row0 + (int)(threadIdx.x >> 2), k = threadIdx.x & 3;
    if (r < n && k < W) x_tgt = tgt[(off + r) * W + k];
  }
#if MI355_OPERAND_FIRST
  if (t.active && !streaming) rows.begin(Mp, t);  // matrix stream in flight from here on: issued AFTER the prologue's loads (results return in issue order)
#endif
  MI_FSTAMP(1);   // all prologue loads and the first matrix group issued
  // ---- scalars
  double coef;  // alpha (PHASE 1) or beta (PHASE 0)
  if (PHASE == 1) {
    const bool first = first1;
    block_sum2_t<NTH>(pa, pb, sm);
    const double d = pa;
    coef = first ? 0.0 : rTz0 / d;
    if (lead) {
      st->d = d; st->alpha = coef;
      st->rTz_prev = first ? 1.0 : rTz0;
      st->it = it_nxt0;
      if (x_inwait) { f.xst->xep[0] = xo + (x_push ? 1 : 0); f.xst->epoch = xo; }
    }
  } else {
    const long long it_new = it0 + 1;
    block_sum2_t<NTH>(pa, pb, sm);
    const double rr = pa, rz = pb;
    const double res = sqrt(rr);
    const bool stop = !((it_new < maxit) && (res > tol));
    coef = 1. / old;
    coef *= rz;
    if (lead) {
      st->rTr = rr; st->rTz = rz; st->beta = coef;
      st->it_nxt = it_new;
      if (it_new <= cap) f.res_norm[it_new - 1] = res; else st->overflow = 1;
      if (stop || it_new > cap) st->done = 1;
      if (x_inwait) { f.xst->xep[1] = xo + (x_push && !(stop || it_new > cap) ? 1 : 0); f.xst->epoch = xo; }
    }
    if (stop || it_new > cap) {        // same decision in every workgroup (it_new > cap: the reference's BoundsError)
      if (f.exit_args && blockIdx.x == 0) {
        // x is final (the ΠS launch before this one stored it): results to the caller, then ONE store of the solve number
        const SolveArgs q = *f.exit_args;
        for (long long i = threadIdx.x; i < n_gamma; i += NTH) q.x_out[i] = xg[i];
        if (q.res_stage) {
          const long long mres = it_new < q.ncap ? it_new : q.ncap;
          for (long long i = threadIdx.x; i < mres; i += NTH) q.res_stage[i] = i == it_new - 1 ? res : f.res_norm[i];
        }
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
          PinnedFlags *fl = f.exit_flags;
          fl->it = it_new; fl->done = 1; fl->overflow = it_new > cap; fl->respec = 0; fl->x0z = st->x0_zero;
          fl->t_exit = wall_clock64();
          __threadfence_system();
          __hip_atomic_store(&fl->seq, q.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
      return;
    }
  }

  MI_FSTAMP(2);   // partial sums reduced: alpha / beta known
  // ---- operand of this GEMV into LDS; rows of this tile: value for the epilogue dot, owners' stores
#pragma unroll
  for (int q = 0; q < FOLD_CPT; ++q) {
    const int j = q * NTH + threadIdx.x;
    if (j < t.ld) {
      double v = 0.0, vs = 0.0;
      if (j < n) {
        // (the first launch of a solve takes r_0 as it is: the contribution rows still hold the previous solve's
        // values, and 0 * NaN left there by a solve that ended non-finite would poison every later solve)
        v = PHASE == 1 ? (first1 ? cv[q] : cv[q] + (-coef) * cs[q])   // r - alpha*Ap
                       : coef * cv[q] + cs[q];                        // beta*p + z
        if (PHASE == 0 && nvec > 0) v = v - cc[q];                  // ... - W*mu (defcg.jl:303)
        vs = PHASE == 1 ? v / cc[q] : v;
      }
      xs[j] = vs;
      if (q == o_q) {
        const int ri = j - t.row0;
        if (t.active) rowv[ri] = v;
        if (PHASE == 1 && nvec > 0) rowg[ri] = o_g;
        if (o_own) {                                      // owner of this Γ node
          if (PHASE == 1) {
            if (t.active) rowc0[ri] = v * v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int pl = o_peer[k];
              if (pl >= 0) { f.r_nxt[pl] = v; f.p_cur[pl] = o_a; }
            }
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int pl = o_peer[k];
              if (pl >= 0) { f.p_nxt[pl] = v; f.r_cur[pl] = o_a; }
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // Multi-GPU, sharded operator: a tile whose block lives on another rank has done its share of the vector work (scalars,
  // owner stores of p / r, x) and stops here; its contribution rows and partial dots come from the owning rank through the
  // exchange that follows the launch (its own entries stay zero).
  if (!t.active) {
    if (PHASE == 1 && o_q >= 0 && o_own) xg[o_g] = o_x + coef * o_a;  // x + alpha*p (cg.jl:97)
    return;
  }
  MI_FSTAMP(3);   // operand staged
  rows.panel(xs, 0, t.ld);
  MI_FSTAMP(4);   // stream consumed
  double sum[RPW];
  rows.finish(sum);
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int ri = w * RPW + k, r = t.row0 + ri;
    if (rows.lane == 0) {
      double y = 0.0;
      if (r < n) {
        y = PHASE == 1 ? sum[k] / e_cnt[k] : sum[k];
        if (!x_push) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int tg = e_tgt[k][q];
            if (tg >= 0) con_out[tg] = y;
          }
        }
      }
      rowc1[ri] = (r < n ? rowv[ri] : 0.0) * y;    // r_g * z-contribution  /  p_g * Ap-contribution
      if (PHASE == 1 || x_push) rowy[ri] = y;
    }
  }
  if (PHASE == 1 && o_q >= 0 && o_own) xg[o_g] = o_x + coef * o_a;  // x + alpha*p (cg.jl:97), off the critical path
  __syncthreads();
  MI_FSTAMP(5);   // results scattered
  const long long xpo = (long long)((xo + 1) & 1ull) * f.out_stride;
  if (x_push && x_tgt >= 0) {
    const XchgPeers &P = *f.xp;
    const double y = rowy[threadIdx.x >> 2];
    const char *own = P.arena[P.rank];
    for (int q = 0; q < P.n; ++q)
      xchg_store(reinterpret_cast<double *>(reinterpret_cast<char *>(f.con_out) + (P.arena[q] - own)) + xpo + x_tgt, y);
  }
  if (PHASE == 1 && nvec > 0 && (int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + nvec) {
    // per-tile partial of WtA*z (defcg.jl:301): sum over this tile's rows of WtA[v, g(row)] * (z-contribution of the row);
    // the second wave does it while the first one reduces the dot products (nvec <= 64)
    const int v = (int)threadIdx.x - 64;
    const double *aw = AW + (long long)v * n_gamma;
    double s = 0.0;
    for (int i0 = 0; i0 < NR; i0 += 8) {
      double a[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = i0 + k < NR ? aw[rowg[i0 + k]] : 0.0;   // rows beyond the tile: rowy = 0, rowg = 0
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (i0 + k < NR) s += a[k] * rowy[i0 + k];
    }
    part_mu[(long long)v * gridDim.x + blockIdx.x] = s;
  }
  if (threadIdx.x < 64) {  // per-tile partials of the next dot products: one shuffle tree over the NR row terms
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < NR; i += 64) { a += rowc1[i]; b += rowc0[i]; }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0) {
      const int ps = t.active - 1;   // the tile number on one GPU; a tiling-independent slot when the launch is sharded over ranks
      if (!x_push) {
        if (PHASE == 1) { part_out1[ps] = a; part_out0[ps] = b; }
        else part_out0[ps] = a;
      } else {
        const XchgPeers &P = *f.xp;
        const char *own = P.arena[P.rank];
        for (int q = 0; q < P.n; ++q) {
          const long long d = P.arena[q] - own;
          xchg_store(reinterpret_cast<double *>(reinterpret_cast<char *>(f.part_out0) + d) + xpo + ps, PHASE == 1 ? b : a);
          if (PHASE == 1) xchg_store(reinterpret_cast<double *>(reinterpret_cast<char *>(f.part_out1) + d) + xpo + ps, a);
        }
      }
    }
  }
  if (x_push) {
    // publish. The results went out as system-scope write-through stores (xchg_store): nothing of them stays in an L2, so
    // no cache write-back is needed — a system-scope fence per tile walks the L2 and cost 8 us per launch with ~290 tiles
    // (profiles/NOTES.md). Every thread waits for the acknowledgement of its own stores, the barrier collects the
    // workgroup, and the last tile to count itself in stores the flags: all stores of the launch are complete by then.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned int prev = __hip_atomic_fetch_add(&f.xst->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == f.n_arrive - 1) {
        __hip_atomic_store(&f.xst->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const XchgPeers &P = *f.xp;
        for (int q = 0; q < P.n; ++q) __hip_atomic_store(xchg_flag(P, q, P.rank), xo + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
  MI_FSTAMP(6);
}

// y[i] = sum of the local contributions to Γ node i, in ascending subdomain order
// (`Sx[lΓ] += Sdxd[lΓd]` for idom = 1..ndom, EPDD.jl:779-781 / 1379-1381); indexed form, used by the
// matrix-free operator whose local results are produced in local order by the SpMV kernel.
__global__ __launch_bounds__(NT) void k_assemble(int n, const int *__restrict__ aptr, const int *__restrict__ apos,
                                                 const double *__restrict__ yloc, double *__restrict__ y,
                                                 const int *done) {
  if (done && *done) return;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    double s = 0.0;
    for (int k = aptr[i]; k < aptr[i + 1]; ++k) s += yloc[apos[k]];
    y[i] = s;
  }
}
// The same sum over the contiguous contribution slots written by k_gemv_batched.
__global__ __launch_bounds__(NT) void k_assemble_slots(int n, int width, const double *__restrict__ yslots,
                                                       double *__restrict__ y, const int *done) {
  if (done && *done) return;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    double s = 0.0;
    for (int j = 0; j < width; ++j) s += yslots[(long long)i * width + j];
    y[i] = s;
  }
}
// xcat[slot] = x[gidx[slot]] for every local slot (matrix-free path: xd[lΓd] = x[lΓ], EPDD.jl:728-730)
__global__ __launch_bounds__(NT) void k_gather(int nloc, const int *__restrict__ gidx, const double *__restrict__ x,
                                               double *__restrict__ xcat) {
  for (int i = blockIdx.x * NT + threadIdx.x; i < nloc; i += gridDim.x * NT) xcat[i] = x[gidx[i]];
}

// ------------------------------------------------------------------ Krylov loop kernels
// Set-up:  r = b - Ap; partial r'r and b'b.
__global__ __launch_bounds__(NT) void k_residual(int n, const double *__restrict__ b, const double *__restrict__ Ap,
                                                 double *__restrict__ r, double *__restrict__ part_rr,
                                                 double *__restrict__ part_bb) {
  __shared__ double sm[NT / 64 + 1];
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
    part_rr[blockIdx.x] = srr;
    if (part_bb) part_bb[blockIdx.x] = sbb;
  }
}
// Start-up of the folded Schur loop when n_Γ exceeds the single-workgroup kernels (k_fused_residual<., true>): after
// k_residual, one workgroup sums its partials and leaves the scalars exactly as that kernel does.
__global__ __launch_bounds__(NT) void k_fold_start(SolverState *st, const double *part_rr, const double *part_bb, int g) {
  __shared__ double sm[NT / 64 + 1];
  const double eps = st->eps;
  const double rr = sum_partials(part_rr, g, sm);
  const double bb = sum_partials(part_bb, g, sm);
  if (threadIdx.x == 0) krylov_start_zero(st, rr, bb, eps, 0.0, rr);
}
// Set-up: it = 1; res_norm[1] = sqrt(r'r); tol = eps*norm2(b) (cg.jl:26-32 / 81-89). eps, maxit and
// res_cap were written into the state block by the host.
__global__ __launch_bounds__(NT) void k_init_state(SolverState *st, const double *part_rr, const double *part_bb,
                                                   const double *part_rz, int g, double *res_norm) {
  __shared__ double sm[NT / 64 + 1];
  const double eps = st->eps;
  const long long maxit = st->maxit, res_cap = st->res_cap;
  const double rr = sum_partials(part_rr, g, sm);
  const double bb = sum_partials(part_bb, g, sm);
  const double rz = part_rz ? sum_partials(part_rz, g, sm) : rr;
  if (threadIdx.x == 0) {
    st->rTr = rr; st->bnorm = sqrt(bb);
    krylov_start_one(st, res_norm, rr, rz, eps * st->bnorm, maxit, res_cap);
  }
}
// Loop step 1:  d = p'Ap (from partials); alpha = num/d; x += alpha p; r -= alpha Ap; partial r'r.
// num = r'z (pcg, cg.jl:95) or r'r (cg, cg.jl:38). With a diagonal preconditioner (diag 1: identity,
// 2: Jacobi) `z .= M \ r` and the partial r'z (cg.jl:100-101) are produced in the same pass.
__global__ __launch_bounds__(NT) void k_update_xr(int n, SolverState *st, const double *part_pAp, int g_in,
                                                  const double *__restrict__ p, const double *__restrict__ Ap,
                                                  double *__restrict__ x, double *__restrict__ r,
                                                  double *__restrict__ part_rr, int precond, int diag,
                                                  const double *__restrict__ dinv, double *__restrict__ z,
                                                  double *__restrict__ part_rz) {
  if (st->done) return;
  __shared__ double sm[NT / 64 + 1];
  // The element loads do not depend on alpha: the first four elements of every thread (all of them unless the grid is
  // capped) are requested BEFORE the partial sums are reduced, so the kernel pays one memory round trip, not two.
  const int stride = gridDim.x * NT;
  int i0 = blockIdx.x * NT + threadIdx.x;
  double pv[4], xv[4], rv[4], av[4], dv[4];
  auto load = [&](int base) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + k * stride;
      const bool ok = i < n;
      pv[k] = ok ? p[i] : 0.0; xv[k] = ok ? x[i] : 0.0; rv[k] = ok ? r[i] : 0.0; av[k] = ok ? Ap[i] : 0.0;
      dv[k] = ok && diag == 2 ? dinv[i] : 1.0;
    }
  };
  load(i0);
  const double d = sum_partials(part_pAp, g_in, sm);
  const double num = precond ? st->rTz : st->rTr;
  const double alpha = num / d;
  double srr = 0.0, srz = 0.0;
  for (;;) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k * stride;
      if (i < n) {
        x[i] = xv[k] + alpha * pv[k];              // axpy!(alpha, p, x)
        const double ri = rv[k] + (-alpha) * av[k];  // axpy!(-alpha, Ap, r)
        r[i] = ri;
        srr += ri * ri;
        if (diag) {
          const double zi = diag == 2 ? dv[k] * ri : ri;
          z[i] = zi;
          srz += ri * zi;
        }
      }
    }
    i0 += 4 * stride;
    if (i0 >= n) break;
    load(i0);
  }
  srr = block_sum(srr, sm);
  if (diag) srz = block_sum(srz, sm);
  if (threadIdx.x == 0) {
    part_rr[blockIdx.x] = srr;
    if (diag) part_rz[blockIdx.x] = srz;
    if (blockIdx.x == 0) {
      st->d = d; st->alpha = alpha;
      st->rTr_prev = st->rTr; st->rTz_prev = st->rTz;
    }
  }
}
// Loop step 2:  r'r, r'z from partials; beta = (1/old)*new (cg.jl:39,44 / 96,102);
// p = beta p + z [- W mu] (cg.jl:45 / 103; defcg.jl:78 / 303); it += 1; res_norm[it] = sqrt(r'r); stop rule.
__global__ __launch_bounds__(NT) void k_update_p(int n, SolverState *st, const double *part_rr,
                                                 const double *part_rz, int g_in, const double *__restrict__ z,
                                                 double *__restrict__ p, const double *__restrict__ W,
                                                 const double *__restrict__ mu, int nvec, double *res_norm,
                                                 int precond) {
  __shared__ double sm[NT / 64 + 1];
  __shared__ int was_done;  // thread 0 of workgroup 0 sets st->done below: take one uniform snapshot
  if (threadIdx.x == 0) was_done = st->done;
  __syncthreads();
  if (was_done) return;
  const int stride = gridDim.x * NT;
  int i0 = blockIdx.x * NT + threadIdx.x;
  double pv[4], zv[4];
  auto load = [&](int base) {  // independent of beta: requested before the reductions (see k_update_xr)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + k * stride;
      pv[k] = i < n ? p[i] : 0.0;
      zv[k] = i < n ? z[i] : 0.0;
    }
  };
  load(i0);
  const double rr = sum_partials(part_rr, g_in, sm);
  const double rz = precond ? sum_partials(part_rz, g_in, sm) : rr;
  const double old = precond ? st->rTz_prev : st->rTr_prev;
  const double beta = krylov_beta(old, rz);
  for (;;) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k * stride;
      if (i < n) {
        double v = beta * pv[k] + zv[k];     // axpby!(1, z, beta, p)
        if (nvec > 0) v = v - w_times_mu(W, n, i, mu, nvec);   // (W*mu)[i], column-axpy order
        p[i] = v;
      }
    }
    i0 += 4 * stride;
    if (i0 >= n) break;
    load(i0);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->rTr = rr; st->rTz = rz; st->beta = beta;
    const long long it = st->it + 1;
    const double res = sqrt(rr);
    krylov_count(st, res_norm, it, res, krylov_stop(it, st->maxit, st->res_cap, res, st->tol));
  }
}
// Entry and exit of a solve, one launch each instead of a handful of small copies (each a separate blit on the stream):
// in:  b, x0 -> workspace; eps / maxit / res_cap -> state block.
__global__ __launch_bounds__(NT) void k_solve_begin(int n, const double *__restrict__ b_in, const double *__restrict__ x_in,
                                                    double *__restrict__ b, double *__restrict__ x, SolverState *st, double eps,
                                                    long long maxit, long long res_cap) {
  int nz = 0;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    const double xi = x_in[i];
    b[i] = b_in[i]; x[i] = xi;
    nz |= xi != 0.0;   // NaN counts as non-zero
  }
  // x0_zero was left at 1 by the previous solve's k_solve_end (0 after allocation): it survives only if every entry is 0
  if (__syncthreads_or(nz) && threadIdx.x == 0) st->x0_zero = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) { st->eps = eps; st->maxit = maxit; st->res_cap = res_cap; st->done = 0; }
}
// The same entry / exit pair as graph nodes: arguments through the pinned block instead of kernel parameters, and the
// exit kernel ends with a release of everything it wrote followed by ONE store of the solve number, which is what the
// host waits for (no stream synchronisation on the critical path of a solve).
__global__ __launch_bounds__(NT) void k_solve_begin_g(int n, const SolveArgs *pin, double *__restrict__ b, double *__restrict__ x,
                                                      SolverState *st, SolveArgs *dev, PinnedFlags *flags) {
  __shared__ unsigned long long a[SOLVE_ARGS_WORDS];
  if (blockIdx.x == 0 && threadIdx.x == 0) flags->t_entry = wall_clock64();
  const SolveArgs &q = load_solve_args(pin, a);
  const double *b_in = q.b_in, *x_in = q.x_in;
  int nz = 0;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    const double xi = x_in[i];
    b[i] = b_in[i]; x[i] = xi;
    nz |= xi != 0.0;
  }
  if (__syncthreads_or(nz) && threadIdx.x == 0) st->x0_zero = 0;
  if (blockIdx.x == 0) {
    if (threadIdx.x < SOLVE_ARGS_WORDS) ((unsigned long long *)dev)[threadIdx.x] = a[threadIdx.x];
    if (threadIdx.x == 0) { st->eps = q.eps; st->maxit = q.maxit; st->res_cap = q.res_cap; st->done = 0; }
  }
}
__global__ __launch_bounds__(NT) void k_solve_end_g(int n, SolverState *st, const SolveArgs *dev, int fold, const double *__restrict__ x,
                                                    const double *__restrict__ res_norm, PinnedFlags *flags, int *x0_zero,
                                                    unsigned *end_count) {
  __shared__ int last;
  const long long it = fold ? st->it_nxt : st->it;
  const SolveArgs q = *dev;
  // a loop launch may have handed the results over already (k_gemv_pcg's stop branch): same answer in every workgroup,
  // since that launch precedes this one on the stream and this kernel stores the number only after all of them counted in
  if (sys_load_u64(&flags->seq) == q.seq) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *x0_zero = 1;   // "assume zero" for the next solve's entry kernel to refute
    return;
  }
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) q.x_out[i] = x[i];
  if (q.res_stage) {
    const long long m = it < q.ncap ? it : q.ncap;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < m; i += (long long)gridDim.x * NT) q.res_stage[i] = res_norm[i];
  }
  __threadfence_system();   // this thread's stores are out (device memory written back, pinned memory delivered) ...
  __syncthreads();          // ... for the whole workgroup before it counts itself as finished
  if (threadIdx.x == 0) last = atomicAdd(end_count, 1u) == gridDim.x - 1;
  __syncthreads();
  if (last && threadIdx.x == 0) {
    *end_count = 0;
    const int x0z = *x0_zero;
    *x0_zero = 1;
    publish_flags(flags, it, st->done, st->overflow, 0, x0z, true, q.seq);
  }
}
// out: x -> caller's vector (device), `it` / done / overflow and the first min(it, ncap) residual norms -> pinned host memory.
__global__ __launch_bounds__(NT) void k_solve_end(int n, const SolverState *st, int fold, const double *__restrict__ x,
                                                  double *__restrict__ x_out, const double *__restrict__ res_norm,
                                                  double *__restrict__ res_stage, long long ncap, PinnedFlags *flags,
                                                  int *x0_zero) {
  const long long it = fold ? st->it_nxt : st->it;
  if (blockIdx.x == 0 && threadIdx.x == 0) *x0_zero = 1;  // "assume zero" for the next solve's k_solve_begin to refute
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) x_out[i] = x[i];
  if (res_stage) {
    const long long m = it < ncap ? it : ncap;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < m; i += (long long)gridDim.x * NT) res_stage[i] = res_norm[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { flags->it = it; flags->done = st->done; flags->overflow = st->overflow; }
}

// ------------------------------------------------------------------ fused single-workgroup kernels (n <= 8192)
// On the Schur system the Γ-vectors are tiny (n_Γ ≈ 4 k): one 1024-thread workgroup keeps its
// share of every vector in registers and does Γ-sum + dot + update in one launch, so a PCG
// iteration is 4 launches (S GEMV, this, NN GEMV, this) instead of 8 latency-bound ones.
// A vector operand is a "view": width == 0: plain vector src[i]; width == W: the Γ-sum
// y[i] = Σ_{j<W} src[i*W + j] over the contribution slots of k_gemv_batched (deferred scatter-add).
// All loads of a kernel are issued up front (one memory round trip), scalars included.
constexpr int NTF = 1024;
constexpr int FUSED_MAX_N = NTF * 8;

struct AsmView {
  const double *src;
  int width;
};
__device__ __forceinline__ double view_load(const AsmView &v, int e) {
  if (v.width == 0) return v.src[e];
  double s = 0.0;
  if (v.width == 4) {
    const double4 q = *reinterpret_cast<const double4 *>(v.src + 4ll * e);
    s += q.x; s += q.y; s += q.z; s += q.w;
  } else if (v.width == 2) {
    const double2 q = *reinterpret_cast<const double2 *>(v.src + 2ll * e);
    s += q.x; s += q.y;
  } else {
    for (int j = 0; j < v.width; ++j) s += v.src[(long long)e * v.width + j];
  }
  return s;
}
// Deterministic sum over the 1024-thread workgroup, broadcast. `sm` has NTF/64 + 1 doubles.
__device__ __forceinline__ double block_sum_f(double v, double *sm) { return block_sum_t<NTF>(v, sm); }
// Ap = view; d = p'Ap; alpha = num/d; x += alpha p; r -= alpha Ap; r'r   (cg.jl:36-43 / 93-99)
template <int EPT>
__global__ __launch_bounds__(NTF) void k_fused_xr(int n, SolverState *st, AsmView vAp, const double *__restrict__ p,
                                                  double *__restrict__ x, double *__restrict__ r, int precond) {
  __shared__ double sm[NTF / 64 + 1];
  const int done0 = st->done;   // tested after the operands have been requested: one memory round trip, not two
  const double rTr0 = st->rTr, rTz0 = st->rTz;
  double pe[EPT], ae[EPT], xe[EPT], re[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    pe[k] = ae[k] = xe[k] = re[k] = 0.0;
    if (e < n) { ae[k] = view_load(vAp, e); pe[k] = p[e]; xe[k] = x[e]; re[k] = r[e]; }
  }
  asm volatile("" ::"s"(done0), "v"(pe[0]), "v"(ae[0]), "v"(xe[0]), "v"(re[0]));
  if (done0) return;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) s += pe[k] * ae[k];
  const double d = block_sum_f(s, sm);
  const double alpha = (precond ? rTz0 : rTr0) / d;
  double srr = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) {
      x[e] = xe[k] + alpha * pe[k];
      const double ri = re[k] + (-alpha) * ae[k];
      r[e] = ri;
      srr += ri * ri;
    }
  }
  srr = block_sum_f(srr, sm);
  if (threadIdx.x == 0) {
    st->d = d; st->alpha = alpha;
    st->rTr_prev = rTr0; st->rTz_prev = rTz0;
    st->rTr = srr;
  }
}
// mu = WtAW \ rhs by ONE wave, in registers: lane i holds b[i]; row swaps, unit-lower forward and upper backward
// substitution in the order of LAPACK getrs (and of k_lu_solve), values exchanged with wave shuffles. nvec <= 64.
__device__ __forceinline__ double wave_lu_solve(int nvec, const double *__restrict__ LU, const int *__restrict__ piv,
                                                double b) {
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < nvec; ++k) {
    const int pk = piv[k];
    const double vk = __shfl(b, k, 64), vp = __shfl(b, pk, 64);
    if (pk != k) { if (lane == k) b = vp; else if (lane == pk) b = vk; }
  }
  for (int k = 0; k < nvec; ++k) {
    const double bk = __shfl(b, k, 64);
    if (lane > k && lane < nvec) b -= bk * LU[lane + (long long)k * nvec];
  }
  for (int k = nvec - 1; k >= 0; --k) {
    if (lane == k) b /= LU[k + (long long)k * nvec];
    const double bk = __shfl(b, k, 64);
    if (lane < k) b -= bk * LU[lane + (long long)k * nvec];
  }
  return b;
}
// The same solve with this lane's row of the factors in registers and the exchanged values read with v_readlane
// (uniform lane index): a step of the 3*nvec-long dependency chain costs a few cycles instead of an LDS round trip.
__device__ __forceinline__ double lane_read(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
template <int NV>
__device__ __forceinline__ double wave_lu_solve_reg(int nvec, const double *lu_s, const int *piv_s, double b) {
  const int lane = threadIdx.x & 63;
  double row[NV];                                    // LU[lane, 0:nvec]
#pragma unroll
  for (int k = 0; k < NV; ++k) row[k] = (k < nvec && lane < nvec) ? lu_s[lane + k * nvec] : 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (k < nvec) {
      const int pk = __builtin_amdgcn_readfirstlane(piv_s[k]);
      const double vk = lane_read(b, k), vp = lane_read(b, pk);
      if (pk != k) { if (lane == k) b = vp; else if (lane == pk) b = vk; }
    }
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (k < nvec) {
      const double bk = lane_read(b, k);
      if (lane > k && lane < nvec) b -= bk * row[k];
    }
#pragma unroll
  for (int k = NV - 1; k >= 0; --k)
    if (k < nvec) {
      if (lane == k) b /= row[k];
      const double bk = lane_read(b, k);
      if (lane < k) b -= bk * row[k];
    }
  return b;
}

// W_loc[v * nloc + loc] = W[v * n + gidx[loc]]: the deflation vectors in the local order of the dense blocks, once per solve
// (k_defl_mu then needs no Γ index before it can request its W entries: one memory round trip less per iteration)
__global__ __launch_bounds__(NT) void k_gather_w_loc(int nvec, long long n_gamma, int nloc, const int *__restrict__ gidx,
                                                     const double *__restrict__ W, double *__restrict__ W_loc) {
  const int loc = blockIdx.x * NT + threadIdx.x;
  if (loc >= nloc) return;
  const long long g = gidx[loc];
  const int v = blockIdx.y;
  W_loc[(long long)v * nloc + loc] = W[(long long)v * n_gamma + g];
}

// Folded Def-PCG, between the ΠS and the S launch: mu = WtAW \ (WtA*z) from the per-tile partials (every workgroup
// solves the same nvec x nvec system with the LU factors staged in LDS, nvec <= 64), then
// wm_loc[loc] = (W*mu)[gidx[loc]] in column-axpy order (`W * mu`, defcg.jl:303) for this workgroup's slice of the
// local positions, where the S launch reads it contiguously. 1024 threads: 16 per deflation vector for the sums.
__global__ __launch_bounds__(1024) void k_defl_mu(const SolverState *st, int nvec, int ntiles, const double *__restrict__ part_mu,
                                                  const double *__restrict__ LU, const int *__restrict__ piv, int nloc,
                                                  const int *__restrict__ gidx,   // (up to here: preloaded into SGPRs at wave start)
                                                  const double *__restrict__ W, long long n_gamma, double *__restrict__ wm_loc,
                                                  double *__restrict__ mu_out, const double *__restrict__ W_loc) {
  // One memory round trip for everything whose address is known at launch (stop flag, LU factors, pivots, Γ index, the
  // first batch of partials), a second one for the W entries behind the Γ index: the kernel is nothing but latency.
  __shared__ double lu_s[64 * 64];
  __shared__ int piv_s[64];
  __shared__ double mu_s[64];
  const int done0 = st->done;
  double lu_r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int i = (int)threadIdx.x + 1024 * k; lu_r[k] = i < nvec * nvec ? LU[i] : 0.0; }
  const int piv_r = (int)threadIdx.x < nvec ? piv[threadIdx.x] : 0;
  const int loc = blockIdx.x * 1024 + threadIdx.x;
  const long long g = (loc < nloc && !W_loc) ? gidx[loc] : 0;
  // rhs[v] = sum over tiles: TPV = 1024 / (nvec rounded up to a power of two) threads per vector, every thread's
  // partials requested in one batch, then a TPV-lane shuffle tree (fixed order: deterministic)
  int vpad = 1;
  while (vpad < nvec) vpad <<= 1;
  const int tpv = 1024 / vpad;                          // 16 .. 1024, a power of two
  const int v = threadIdx.x / tpv, l16 = threadIdx.x % tpv;
  double a0[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) a0[k] = (v < nvec && l16 + tpv * k < ntiles) ? part_mu[(long long)v * ntiles + l16 + tpv * k] : 0.0;
  // W entries of this thread's local position: independent of mu, in flight during the sums and the solve (from the
  // pre-gathered W_loc they need no Γ index: requested with everything else, ahead of the exit test)
  double w0[20];                                        // the first 20 columns of W at g
#pragma unroll
  for (int u = 0; u < 20; ++u)
    w0[u] = (u < nvec && loc < nloc) ? (W_loc ? W_loc[(long long)u * nloc + loc] : W[(long long)u * n_gamma + g]) : 0.0;
  asm volatile("" ::"s"(done0));
  if (done0) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int i = (int)threadIdx.x + 1024 * k; if (i < nvec * nvec) lu_s[i] = lu_r[k]; }
  if ((int)threadIdx.x < nvec) piv_s[threadIdx.x] = piv_r;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += a0[k];
  if (v < nvec)
    for (int i0 = l16 + tpv * 16; i0 < ntiles; i0 += tpv * 16) {
      double a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = i0 + tpv * k < ntiles ? part_mu[(long long)v * ntiles + i0 + tpv * k] : 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += a[k];
    }
  if (tpv > 64) {                                       // few vectors: finish across waves through LDS
    s = wave_sum(s);
    __shared__ double wsum[16];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (l16 == 0 && v < nvec) { s = 0.0; for (int k = 0; k < tpv / 64; ++k) s += wsum[v * (tpv / 64) + k]; }
  } else {
    for (int o = tpv / 2; o > 0; o >>= 1) s += __shfl_down(s, o, tpv);
  }
  if (l16 == 0 && v < nvec) mu_s[v] = s;
  __syncthreads();
  if (threadIdx.x < 64) {
    const double rv = (int)threadIdx.x < nvec ? mu_s[threadIdx.x] : 0.0;
    const double m = nvec <= 12 ? wave_lu_solve_reg<12>(nvec, lu_s, piv_s, rv)
                   : nvec <= 20 ? wave_lu_solve_reg<20>(nvec, lu_s, piv_s, rv) : wave_lu_solve(nvec, lu_s, piv_s, rv);
    mu_s[threadIdx.x] = m;
    if (blockIdx.x == 0 && (int)threadIdx.x < nvec) mu_out[threadIdx.x] = m;
  }
  __syncthreads();
  if (loc < nloc) {
    double wm = 0.0;
#pragma unroll
    for (int u = 0; u < 20; ++u)
      if (u < nvec) wm += w0[u] * mu_s[u];
    for (int q0 = 20; q0 < nvec; q0 += 16) {      // beyond the preloaded columns: sixteen in flight per thread
      double w[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        w[u] = q0 + u < nvec ? (W_loc ? W_loc[(long long)(q0 + u) * nloc + loc] : W[(long long)(q0 + u) * n_gamma + g]) : 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (q0 + u < nvec) wm += w[u] * mu_s[q0 + u];
    }
    wm_loc[loc] = wm;
  }
}

// z = view; r'z; beta = (1/old)*new; p = beta p + z [- W mu]; it += 1; res_norm[it]; stop rule
// (cg.jl:44-47 / 100-106; defcg.jl:76-80 / 299-305). r'r was stored by k_fused_xr. Deflation: mu is either
// given, or (LU != nullptr, nvec <= 64) solved here from rhs[v] = WtA[v,:].z by the first wave.
template <int EPT>
__global__ __launch_bounds__(NTF) void k_fused_p(int n, SolverState *st, AsmView vz, const double *__restrict__ r,
                                                 double *__restrict__ p, const double *__restrict__ W,
                                                 const double *__restrict__ mu, int nvec, double *res_norm,
                                                 int precond, const double *__restrict__ LU,
                                                 const int *__restrict__ piv, const double *__restrict__ rhs) {
  if (st->done) return;  // written only by thread 0 at the very end, behind the barriers below
  __shared__ double sm[NTF / 64 + 1];
  __shared__ double mu_s[64];
  __shared__ double lu_s[64 * 64];  // the factors in LDS: the substitution is a chain of 3*nvec dependent steps, and a
  __shared__ int piv_s[64];         // global load inside every step costs a memory round trip each
  const bool wave_lu = nvec > 0 && LU;
  if (wave_lu) {
    for (int i = threadIdx.x; i < nvec * nvec; i += NTF) lu_s[i] = LU[i];
    if ((int)threadIdx.x < nvec) piv_s[threadIdx.x] = piv[threadIdx.x];
  }
  const double rr = st->rTr;
  const double old = precond ? st->rTz_prev : st->rTr_prev;
  const double tol = st->tol;
  const long long it0 = st->it, maxit = st->maxit, cap = st->res_cap;
  double ze[EPT], pe[EPT];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    ze[k] = pe[k] = 0.0;
    if (e < n) {
      ze[k] = view_load(vz, e);
      pe[k] = p[e];
      if (precond) s += r[e] * ze[k];
    }
  }
  if (wave_lu) {
    const double rv = threadIdx.x < (unsigned)nvec ? rhs[threadIdx.x] : 0.0;
    __syncthreads();  // lu_s, piv_s
    if (threadIdx.x < 64) mu_s[threadIdx.x] = wave_lu_solve(nvec, lu_s, piv_s, rv);
  }
  const double rz = precond ? block_sum_f(s, sm) : rr;
  if (!precond) __syncthreads();  // mu_s visible (block_sum_f has barriers of its own)
  const double beta = krylov_beta(old, rz);
  double wm[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) wm[k] = 0.0;
  if (nvec > 0) {  // (W*mu)[e] in column order; the loads of 8 columns x EPT elements go out together (one round trip per 8 columns)
    const double *mup = LU ? mu_s : mu;
    constexpr int QB = EPT >= 8 ? 4 : 8;  // EPT*QB doubles in flight per thread (<= 64 VGPRs)
    for (int q0 = 0; q0 < nvec; q0 += QB) {
      double w[EPT][QB];
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        const int e = k * NTF + threadIdx.x;
#pragma unroll
        for (int u = 0; u < QB; ++u) w[k][u] = (e < n && q0 + u < nvec) ? W[(long long)(q0 + u) * n + e] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < QB; ++u)
        if (q0 + u < nvec) {
          const double m = mup[q0 + u];
#pragma unroll
          for (int k = 0; k < EPT; ++k) wm[k] += w[k][u] * m;
        }
    }
  }
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) {
      double v = beta * pe[k] + ze[k];
      if (nvec > 0) v = v - wm[k];
      p[e] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    st->rTz = rz; st->beta = beta;
    const double res = sqrt(rr);
    krylov_count(st, res_norm, it0 + 1, res, krylov_stop(it0 + 1, maxit, cap, res, tol));
  }
}
// Unpreconditioned cg (cg.jl:35-47): both halves of the iteration in ONE single-workgroup launch — z is r,
// so nothing but two workgroup reductions separates alpha from beta:
//   d = p'Ap; alpha = r'r/d; x += alpha p; r -= alpha Ap; r'r; beta = (1/old)*new; p = beta p + r; it; stop rule.
template <int EPT>
__global__ __launch_bounds__(NTF) void k_fused_cg(int n, SolverState *st, AsmView vAp, double *__restrict__ p,
                                                  double *__restrict__ x, double *__restrict__ r, double *res_norm) {
  __shared__ double sm[NTF / 64 + 1];
  const int done0 = st->done;   // tested after the operands have been requested: one memory round trip, not two
  const double rTr0 = st->rTr, tol = st->tol;
  const long long it0 = st->it, maxit = st->maxit, cap = st->res_cap;
  double pe[EPT], ae[EPT], xe[EPT], re[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    pe[k] = ae[k] = xe[k] = re[k] = 0.0;
    if (e < n) { ae[k] = view_load(vAp, e); pe[k] = p[e]; xe[k] = x[e]; re[k] = r[e]; }
  }
  asm volatile("" ::"s"(done0), "v"(pe[0]), "v"(ae[0]), "v"(xe[0]), "v"(re[0]));
  if (done0) return;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) s += pe[k] * ae[k];
  const double d = block_sum_f(s, sm);
  const double alpha = rTr0 / d;
  double srr = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) {
      x[e] = xe[k] + alpha * pe[k];
      re[k] = re[k] + (-alpha) * ae[k];
      r[e] = re[k];
      srr += re[k] * re[k];
    }
  }
  const double rr = block_sum_f(srr, sm);
  const double beta = krylov_beta(rTr0, rr);
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) p[e] = beta * pe[k] + re[k];
  }
  if (threadIdx.x == 0) {
    st->d = d; st->alpha = alpha; st->beta = beta;
    st->rTr_prev = rTr0; st->rTz_prev = rTr0;
    st->rTr = rr; st->rTz = rr;
    const double res = sqrt(rr);
    krylov_count(st, res_norm, it0 + 1, res, krylov_stop(it0 + 1, maxit, cap, res, tol));
  }
}

// Set-up, first half: r = b - A*x (Ap as a view); r'r and b'b   (cg.jl:28-29,32 / 83-84,88).
// FOLD: also the scalars the folded PCG launches (k_gemv_pcg) expect at start-up: tol, it_nxt = 0,
// rTz_prev = 1, flags cleared (the first PHASE 1 launch gathers r_0 and treats p as 0 by itself).
template <int EPT, bool FOLD>
__global__ __launch_bounds__(NTF) void k_fused_residual(int n, SolverState *st, AsmView vAp,
                                                        const double *__restrict__ b, double *__restrict__ r) {
  __shared__ double sm[NTF / 64 + 1];
  const double eps = st->eps;
  double srr = 0.0, sbb = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) {
      const double bi = b[e];
      const double ri = bi - view_load(vAp, e);
      r[e] = ri;
      srr += ri * ri;
      sbb += bi * bi;
    }
  }
  srr = block_sum_f(srr, sm);
  sbb = block_sum_f(sbb, sm);
  if (threadIdx.x == 0) {
    if (FOLD) krylov_start_zero(st, srr, sbb, eps, 0.0, srr);
    else { st->rTr = srr; st->bnorm = sqrt(sbb); }
  }
}
// Entry of a whole-solve graph of the folded loop that was built for x0 == 0 (the usual call, `pcg(S, b, zeros, M)`): the
// three launches of the general entry (k_solve_begin_g, the skipped `S*x0`, k_fused_residual<., true>) in one — b and x0
// in, r_0 = b, the scalars exactly as k_fused_residual<., true> leaves them (b - 0 = b bit for bit, same sum order).
// A non-zero x0 is reported instead (respec): nothing else of the graph runs (done = 1) and the host replays the
// general form.
template <int EPT>
__global__ __launch_bounds__(NTF) void k_entry_zero(int n, const SolveArgs *pin, double *__restrict__ b, double *__restrict__ x,
                                                    double *__restrict__ r, SolverState *st, SolveArgs *dev, PinnedFlags *flags) {
  __shared__ unsigned long long a[SOLVE_ARGS_WORDS];
  __shared__ double sm[NTF / 64 + 1];
  if (threadIdx.x == 0) flags->t_entry = wall_clock64();
  const SolveArgs &q = load_solve_args(pin, a);
  const double *b_in = q.b_in, *x_in = q.x_in;
  double bv[EPT], xv[EPT];
  int nz = 0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    bv[k] = 0.0; xv[k] = 0.0;
    if (e < n) { bv[k] = b_in[e]; xv[k] = x_in[e]; nz |= xv[k] != 0.0; }
  }
  nz = __syncthreads_or(nz);
  if (threadIdx.x < SOLVE_ARGS_WORDS) ((unsigned long long *)dev)[threadIdx.x] = a[threadIdx.x];
  if (nz) {
    if (threadIdx.x == 0) {
      st->done = 1; st->x0_zero = 0;
      publish_flags(flags, 0, 0, 0, 1, 0, false, q.seq);
    }
    return;
  }
  double srr = 0.0, sbb = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) {
      const double bi = bv[k];
      const double ri = bi - 0.0;
      b[e] = bi; x[e] = xv[k]; r[e] = ri;
      srr += ri * ri;
      sbb += bi * bi;
    }
  }
  srr = block_sum_f(srr, sm);
  sbb = block_sum_f(sbb, sm);
  if (threadIdx.x == 0) {
    st->eps = q.eps; st->maxit = q.maxit; st->res_cap = q.res_cap; st->x0_zero = 1;
    krylov_start_zero(st, srr, sbb, q.eps, 0.0, srr);
  }
}
// Set-up, second half: z = view; r'z; p = z; it = 1; res_norm[1]; tol; stop rule (cg.jl:26-33 / 81-89).
// eps, maxit, res_cap arrive through st->tol / st->maxit / st->res_cap (written by the host before the
// launch), so that the launch can live in a replayable graph.
template <int EPT>
__global__ __launch_bounds__(NTF) void k_fused_start(int n, SolverState *st, AsmView vz, const double *__restrict__ r,
                                                     double *__restrict__ p, double *res_norm, int precond) {
  __shared__ double sm[NTF / 64 + 1];
  const double rr = st->rTr, bnorm = st->bnorm, eps = st->eps;
  const long long maxit = st->maxit, cap = st->res_cap;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    if (e < n) {
      const double ze = view_load(vz, e);
      p[e] = ze;
      if (precond) s += r[e] * ze;
    }
  }
  const double rz = precond ? block_sum_f(s, sm) : rr;
  if (threadIdx.x == 0) krylov_start_one(st, res_norm, rr, rz, eps * bnorm, maxit, cap);
}

// Set-up of the deflated solvers: p = z - W mu (defcg.jl:61 / 285); plain copy when nvec == 0.
__global__ __launch_bounds__(NT) void k_init_p(int n, const double *__restrict__ z, double *__restrict__ p,
                                               const double *__restrict__ W, const double *__restrict__ mu, int nvec) {
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    double v = z[i];
    if (nvec > 0) v = v - w_times_mu(W, n, i, mu, nvec);
    p[i] = v;
  }
}
// x += W mu (defcg.jl:54 / 275)
__global__ __launch_bounds__(NT) void k_add_Wmu(int n, double *__restrict__ x, const double *__restrict__ W,
                                                const double *__restrict__ mu, int nvec) {
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    x[i] = x[i] + w_times_mu(W, n, i, mu, nvec);
  }
}
// part[v*gx + g] = partial of V[:,v] . z   (V = AW for `WtA*z`, V = W for `W'r`); grid (gx, nvec)
__global__ __launch_bounds__(NT) void k_multi_dot_partial(int n, const double *__restrict__ V,
                                                          const double *__restrict__ z, double *__restrict__ part,
                                                          const int *done) {
  if (done && *done) return;
  __shared__ double sm[NT / 64 + 1];
  const double *v = V + (long long)blockIdx.y * n;
  double s = 0.0;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) s += v[i] * z[i];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = s;
}
// part[v] = V[:,v] . z with z given as a view (small systems: one 1024-thread workgroup per vector, all loads of a
// thread issued together); grid (nvec)
template <int EPT>
__global__ __launch_bounds__(NTF) void k_multi_dot_view(int n, const double *__restrict__ V, AsmView vz,
                                                        double *__restrict__ part, const int *done) {
  if (done && *done) return;
  __shared__ double sm[NTF / 64 + 1];
  const double *v = V + (long long)blockIdx.x * n;
  double a[EPT], b[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = k * NTF + threadIdx.x;
    a[k] = b[k] = 0.0;
    if (e < n) { a[k] = v[e]; b[k] = view_load(vz, e); }
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) s += a[k] * b[k];
  s = block_sum_f(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// C[i + j*nvec] = partial-free small gemm entry AW[:,i] . W[:,j]; grid (nvec, nvec), one workgroup each.
__global__ __launch_bounds__(NT) void k_small_gram(int n, const double *__restrict__ AW, const double *__restrict__ W,
                                                   double *__restrict__ C, int nvec) {
  __shared__ double sm[NT / 64 + 1];
  const double *a = AW + (long long)blockIdx.x * n;
  const double *b = W + (long long)blockIdx.y * n;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += NT) s += a[i] * b[i];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) C[blockIdx.x + (long long)blockIdx.y * nvec] = s;
}
// mu = WtAW \ rhs with rhs[v] = sum of partials; LU (unit lower L, U) and pivots from the host
// factorisation (LAPACK getrf/getrs order: all row swaps, forward, backward). One wave.
__global__ __launch_bounds__(64) void k_lu_solve(int nvec, const double *__restrict__ LU, const int *__restrict__ piv,
                                                 const double *__restrict__ part, int gx, double *__restrict__ mu,
                                                 const int *done) {
  if (done && *done) return;
  extern __shared__ double bsh[];
  if (nvec <= 64) {  // one wave, factors staged in LDS (launched with nvec + nvec*nvec + nvec/2 + 1 doubles of LDS)
    double *lu_s = bsh + nvec;
    int *piv_s = reinterpret_cast<int *>(lu_s + nvec * nvec);
    for (int i = threadIdx.x; i < nvec * nvec; i += 64) lu_s[i] = LU[i];
    if ((int)threadIdx.x < nvec) piv_s[threadIdx.x] = piv[threadIdx.x];
    double s = 0.0;
    if ((int)threadIdx.x < nvec)
      for (int g = 0; g < gx; ++g) s += part[threadIdx.x * gx + g];
    __syncthreads();
    s = wave_lu_solve(nvec, lu_s, piv_s, s);
    if ((int)threadIdx.x < nvec) mu[threadIdx.x] = s;
    return;
  }
  for (int v = threadIdx.x; v < nvec; v += 64) {
    double s = 0.0;
    for (int g = 0; g < gx; ++g) s += part[v * gx + g];
    bsh[v] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < nvec; ++k) {
      const int pk = piv[k];
      if (pk != k) { const double t = bsh[k]; bsh[k] = bsh[pk]; bsh[pk] = t; }
    }
  __syncthreads();
  for (int k = 0; k < nvec; ++k) {
    const double bk = bsh[k];
    for (int i = k + 1 + threadIdx.x; i < nvec; i += 64) bsh[i] -= bk * LU[i + (long long)k * nvec];
    __syncthreads();
  }
  for (int k = nvec - 1; k >= 0; --k) {
    if (threadIdx.x == 0) bsh[k] /= LU[k + (long long)k * nvec];
    __syncthreads();
    const double bk = bsh[k];
    for (int i = threadIdx.x; i < k; i += 64) bsh[i] -= bk * LU[i + (long long)k * nvec];
    __syncthreads();
  }
  for (int v = threadIdx.x; v < nvec; v += 64) mu[v] = bsh[v];
}
// y = a - b (matrix-free: Sdxd .-= A_IΓdd' * v, EPDD.jl:652)
__global__ __launch_bounds__(NT) void k_sub(int n, const double *__restrict__ a, const double *__restrict__ b,
                                            double *__restrict__ y) {
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) y[i] = a[i] - b[i];
}

}  // namespace mi
