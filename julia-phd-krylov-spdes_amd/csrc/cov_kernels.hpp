// Matrix-free covariance kernel: Y[0:nt, 0:m] = Σ_j c(p_i, q_j) X[j, 0:m] — the nodal covariance K[i, j] = cov(p_i, q_j) that
// the reference evaluates inside the element loops of do_mass_covariance_assembly (Fem/KarhunenLoeve.jl:40-105) and of its
// rectangular forms (Fem/KarhunenLoeveDomainDecomposition.jl:135-176, 508-547), applied to a vector or a narrow panel without
// ever being stored. Models (Fem/Covariances.jl:27; the names of get_root_filename, KarhunenLoeveDomainDecompositionHelper.jl:54):
//   MI_COV_SEXP  c = σ² exp(-((x1 - x2)² + (y1 - y2)²) / L²)
//   MI_COV_EXP   c = σ² exp(-sqrt((x1 - x2)² + (y1 - y2)²) / L)
// The exponent is computed as the reference writes it (true division by L * L resp. L, no contraction: the Makefile builds with
// -ffp-contract=off), so it carries the bits of the host expression; exp is the device library's (1 ulp).
//
// Tiling. One thread owns one target row and COV_CB column accumulators in registers; a workgroup of COV_ROW_TILE threads owns
// COV_ROW_TILE rows x one block of up to COV_CB columns. The sources go through LDS in chunks of COV_SRC_CHUNK: their
// coordinates and their COV_CB values of X, laid out source-major, so that in the inner loop every lane of a wave reads the same
// LDS address (a broadcast: no bank conflicts) and one exp per (i, j) feeds COV_CB FMAs. fp64 exp and the division are tens of
// VALU instructions per pair; the FMAs of a panel ride along almost free. No MFMA: the exp evaluations are the cost.
// Budget (kernel-resource-usage, gfx950): 60 VGPRs with one accumulator (8 waves per SIMD), 108 with COV_CB = 8 (4 waves per
// SIMD), no scratch; the inner loop is VALU bound and its only memory traffic is LDS broadcasts, so 4 waves suffice. LDS is
// COV_SRC_CHUNK x (2 + COV_CB) x 8 B = 20 KiB per workgroup at most.
//
// Filling the machine. A local KL problem has nt ~ 10³ rows: four row tiles on 256 CUs. The source range is then split over
// blockIdx.z (cov_tiling below; whole chunks per split, a function of (nt, ns, m) only), every split writes its partial sums to a
// workspace, and k_cov_reduce adds the partials in ascending split order. No float atomics, fixed summation orders: two
// calls give the same bits.
//
// Bounds. Every global load is guarded by nt / ns / m; rows past nt and columns past m are never stored; only rows [0, ns) of
// a column of X and rows [0, nt) of a column of Y are touched (the padding up to ldx / ldy is neither read nor written).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/mi355schur.h"

namespace mi {

constexpr int COV_ROW_TILE = 256;    // target rows per workgroup = threads per workgroup
constexpr int COV_SRC_CHUNK = 256;   // sources staged in LDS at a time
constexpr int COV_CB = 8;            // column accumulators per thread
constexpr int COV_FILL = 256;        // workgroups that fill the grid (one per CU): at or above it the sources are not split
constexpr int COV_MAX_SPLITS = 64;

struct CovTiling {
  int row_tiles, col_blocks, splits, chunks_per_split;
};
// Pure host function of the sizes: row tiles x column blocks workgroups when they fill the grid, else the source chunks are
// dealt to as many splits as bring the launch to about 2 COV_FILL workgroups (at most COV_MAX_SPLITS, at most one per chunk).
inline CovTiling cov_tiling(int64_t nt, int64_t ns, int64_t m) {
  CovTiling t;
  t.row_tiles = (int)((nt + COV_ROW_TILE - 1) / COV_ROW_TILE);
  t.col_blocks = (int)((m + COV_CB - 1) / COV_CB);
  const int64_t chunks = (ns + COV_SRC_CHUNK - 1) / COV_SRC_CHUNK;
  const int64_t base = (int64_t)t.row_tiles * t.col_blocks;
  int64_t want = base >= COV_FILL ? 1 : (2 * COV_FILL + base - 1) / base;
  want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, chunks), COV_MAX_SPLITS));
  t.chunks_per_split = (int)((chunks + want - 1) / want);
  t.splits = (int)((chunks + t.chunks_per_split - 1) / t.chunks_per_split);
  return t;
}

template <int MODEL>
__device__ __forceinline__ double cov_value(double px, double py, double qx, double qy, double sig2, double L) {
  const double dx = px - qx, dy = py - qy;
  const double r2 = dx * dx + dy * dy;
  if (MODEL == MI_COV_SEXP) return sig2 * exp(-r2 / (L * L));
  return sig2 * exp(-sqrt(r2) / L);
}

// grid (row_tiles, col_blocks, splits). Split z covers the sources [z * per_split, min(ns, (z + 1) * per_split)) and writes
// out + z * out_split (out_split = 0 with one split: straight into Y). CBT: accumulators in use (1, 2, 4 or COV_CB).
template <int MODEL, int CBT>
__global__ __launch_bounds__(COV_ROW_TILE) void k_cov_apply(int nt, int ns, int m, const double *__restrict__ pt,
                                                            const double *__restrict__ ps, double sig2, double L,
                                                            const double *__restrict__ X, long long ldx, double *__restrict__ out,
                                                            long long ldo, long long out_split, int per_split, const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double sq[2 * COV_SRC_CHUNK];
  __shared__ __attribute__((aligned(16))) double sx[COV_SRC_CHUNK * CBT];
  const int i = (int)blockIdx.x * COV_ROW_TILE + (int)threadIdx.x;
  const int c0 = (int)blockIdx.y * COV_CB;
  const int ncol = min(CBT, m - c0);
  const long long j_begin = (long long)blockIdx.z * per_split;
  const int j_end = (int)min((long long)ns, j_begin + per_split);
  double px = 0.0, py = 0.0;
  if (i < nt) { px = pt[2 * (size_t)i]; py = pt[2 * (size_t)i + 1]; }
  double acc[CBT];
#pragma unroll
  for (int c = 0; c < CBT; ++c) acc[c] = 0.0;
  for (int j0 = (int)j_begin; j0 < j_end; j0 += COV_SRC_CHUNK) {
    const int len = min(COV_SRC_CHUNK, j_end - j0);
    __syncthreads();   // the previous chunk has been consumed
    for (int t = threadIdx.x; t < 2 * len; t += COV_ROW_TILE) sq[t] = ps[2 * (size_t)j0 + t];
    for (int t = threadIdx.x; t < len * CBT; t += COV_ROW_TILE) {
      const int c = t / len, j = t - c * len;   // consecutive threads read consecutive rows of one column
      sx[j * CBT + c] = c < ncol ? X[(size_t)(c0 + c) * ldx + j0 + j] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < len; ++j) {
      const double k = cov_value<MODEL>(px, py, sq[2 * j], sq[2 * j + 1], sig2, L);
#pragma unroll
      for (int c = 0; c < CBT; ++c) acc[c] = fma(k, sx[j * CBT + c], acc[c]);
    }
  }
  if (i < nt) {
    double *o = out + (size_t)blockIdx.z * out_split;
#pragma unroll
    for (int c = 0; c < CBT; ++c)
      if (c < ncol) o[(size_t)(c0 + c) * ldo + i] = acc[c];
  }
}

// Y[i, c] = Σ_s part[s][i, c], s ascending; part is splits x (nt x m, compact)
__global__ __launch_bounds__(COV_ROW_TILE) void k_cov_reduce(int nt, int m, int splits, const double *__restrict__ part,
                                                             double *__restrict__ Y, long long ldy, const int *done) {
  if (done && *done) return;
  const long long total = (long long)nt * m;
  for (long long e = (long long)blockIdx.x * COV_ROW_TILE + threadIdx.x; e < total; e += (long long)gridDim.x * COV_ROW_TILE) {
    const int c = (int)(e / nt), i = (int)(e - (long long)c * nt);
    double s = part[e];
    for (int z = 1; z < splits; ++z) s += part[(size_t)z * total + e];
    Y[(size_t)c * ldy + i] = s;
  }
}

// doubles of workspace a launch of these sizes needs (0 with one split)
inline size_t cov_workspace(int64_t nt, int64_t ns, int64_t m) {
  const CovTiling t = cov_tiling(nt, ns, m);
  return t.splits > 1 ? (size_t)t.splits * (size_t)nt * (size_t)m : 0;
}

// Enqueue Y = K(pt, ps) X on `s`. All pointers are device pointers; `work` holds cov_workspace(nt, ns, m) doubles.
inline void cov_launch(hipStream_t s, int model, double sig2, double L, int nt, const double *pt, int ns, const double *ps, int m,
                       const double *X, long long ldx, double *Y, long long ldy, double *work, const int *done) {
  const CovTiling t = cov_tiling(nt, ns, m);
  const dim3 grid(t.row_tiles, t.col_blocks, t.splits);
  const bool split = t.splits > 1;
  double *out = split ? work : Y;
  const long long ldo = split ? nt : ldy, out_split = split ? (long long)nt * m : 0;
  const int per_split = t.chunks_per_split * COV_SRC_CHUNK;
  const int cbt = m > 4 ? COV_CB : m > 2 ? 4 : m;   // 1, 2, 4 or 8 accumulators in use (m <= COV_CB is one column block)
#define MI_COV_GO(MODEL, CBT) \
  hipLaunchKernelGGL((k_cov_apply<MODEL, CBT>), grid, dim3(COV_ROW_TILE), 0, s, nt, ns, m, pt, ps, sig2, L, X, ldx, out, ldo, out_split, per_split, done)
#define MI_COV_MODEL(MODEL)                                \
  switch (cbt) {                                           \
    case 1: MI_COV_GO(MODEL, 1); break;                    \
    case 2: MI_COV_GO(MODEL, 2); break;                    \
    case 4: MI_COV_GO(MODEL, 4); break;                    \
    default: MI_COV_GO(MODEL, COV_CB); break;              \
  }
  if (model == MI_COV_SEXP) { MI_COV_MODEL(MI_COV_SEXP) } else { MI_COV_MODEL(MI_COV_EXP) }
#undef MI_COV_MODEL
#undef MI_COV_GO
  if (split) {
    const long long total = (long long)nt * m;
    const int g = (int)std::min<long long>((total + COV_ROW_TILE - 1) / COV_ROW_TILE, 1024);
    hipLaunchKernelGGL(k_cov_reduce, dim3(g), dim3(COV_ROW_TILE), 0, s, nt, m, t.splits, (const double *)work, Y, ldy, done);
  }
}

}  // namespace mi
