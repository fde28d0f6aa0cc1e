// Vector quantization of the latent vector ξ: nearest centroid, Lloyd's centre update, k-means++ seeding and the ordered sums
// they share — `kmeans(X, P, tol=1e-8, maxiter=1_000)` of Example20_QuantizedPreconditioner_Functions.jl:56-73 (also
// Example12_Quantization_Functions.jl:29-59, Example13_CLVQ_Functions.jl:129-159, Example18), the scan of `find_precond`
// (Example20_…_Functions.jl:39-54) and of `get_distortion` (Example13_CLVQ_Functions.jl:53-69) — and k_lincomb, the last kernel
// of the combined operator z = Σ_i c_i (Π_i \ r) (`apply_local_interpolation`, Example14_…_Functions.jl:85-97).
//
// All matrices are column-major as Julia passes them: X is d x ns (a sample per column), C is d x P (a centroid per column).
//
// k_vq_assign. The distance is the reference's own expression (x .- c)' * (x .- c): t = x_k - c_k, acc = acc + t * t, k ascending
// from +0 (the Makefile builds with -ffp-contract=off), and ONE accumulator sees all d terms of its pair in order, so every
// dist2 carries the bits of the host loop whatever the tiling. A thread owns a register tile of VQ_PR points x VQ_CR centroids;
// a wave covers the 64 * VQ_PR = VQ_POINT_TILE points of the workgroup's point tile, and the VQ_WAVES waves of a workgroup take
// VQ_CR centroids each of a VQ_CENT_TILE = VQ_WAVES * VQ_CR centroid tile: X goes through LDS in chunks of VQ_K_CHUNK coordinates
// (point-minor: a lane reads its own points, no conflicts), the centroids too (centroid-minor: every lane of a wave reads the
// same 64 bytes, a broadcast). One staged X element feeds VQ_CENT_TILE pairs, one staged pair of LDS reads 3 * VQ_PR * VQ_CR = 96
// fp64 VALU operations: the inner loop is VALU bound. No MFMA and no ‖x‖² - 2 x·c + ‖c‖² expansion.
// The winner is the smallest dist2, among equals the lowest p — the reference's strict `<` scan, including its start from
// dist(x, c_0): a NaN there stays (the scan never replaces it), a NaN elsewhere never wins. A thread scans its centroids in
// ascending p; waves, and the centroid splits over blockIdx.y that fill the machine when the point tiles alone do not (the
// ns = 1 shape of find_precond), are combined by a lexicographic (dist2, p) minimum in k_vq_finish.
// Budget (kernel-resource-usage, gfx950): see the table at the end of this comment.
//
// Ordered sums over samples: VQ_SUM_CHUNK consecutive values are added in ascending order from +0 into a chunk total
// (k_vq_chunk_sums, a thread per chunk), the chunk totals in ascending order (k_vq_scan_totals, which also leaves the sum of
// the earlier chunks for every chunk). The objective Σ_s dist2[s] and the seeding prefix use this order.
//
// Centre update: counts by integer atomics (their result does not depend on the order), an exclusive scan, then the member
// lists: the owner thread of a cluster walks the assignments in ascending s (LDS broadcasts) and appends its members, so every
// list is ascending without a sort and without float atomics. k_vq_centres sums a cluster's members in that order from +0,
// one thread per (cluster, coordinate), and divides by the count (a true division); an empty cluster is not written.
//
// Seeding (k-means++): the uniforms come from the caller. mind[s] = min(mind[s], dist2(x_s, c_{j-1})) through the assign kernel
// (the same bits), prefix(s) = (sum of the earlier chunk totals) + (ascending sum within the chunk of s up to s), the pick is
// the smallest s with prefix(s) > u_j * total, or, where rounding of u_j * total leaves none, the smallest s with
// prefix(s) >= total. Either way mind[pick] > 0: a sample already chosen is never chosen again.
//
// Bounds. Every global load is guarded by d / ns / P; rows past d of a column (the padding up to ldx / ldc) are neither read
// nor written; assignments outside [0, P) raise the error word instead of indexing with them.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   k_vq_assign       160 VGPRs, no scratch, 49 280 B of LDS: 3 workgroups per CU = 3 waves per SIMD by either limit. The loop
//                     is VALU bound with 32 independent accumulators per thread, so three waves cover the LDS latency.
//   every other kernel here: under 32 VGPRs, no scratch, at most 8 KiB of LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "operators.hpp"

namespace mi {

constexpr int VQ_NT = 256;                         // threads per workgroup
constexpr int VQ_WAVES = VQ_NT / 64;
constexpr int VQ_PR = 4;                           // points per thread
constexpr int VQ_CR = 8;                           // centroids per thread
constexpr int VQ_POINT_TILE = 64 * VQ_PR;          // points per workgroup (every wave covers all of them)
constexpr int VQ_CENT_TILE = VQ_WAVES * VQ_CR;     // centroids staged at a time
constexpr int VQ_K_CHUNK = 16;                     // coordinates staged at a time
constexpr int VQ_XS = VQ_POINT_TILE + 1;           // row stride of the staged X chunk (the staging writes run along k)
constexpr int VQ_FILL = 256;                       // workgroups that fill the grid: at or above it the centroids are not split
constexpr int VQ_MAX_SPLITS = 64;
constexpr int VQ_SUM_CHUNK = 256;                  // samples per chunk of the ordered sums
constexpr int VQ_SCAN_CHUNK = 1024;                // assignments staged at a time by the member scan
constexpr int64_t VQ_MAX_N = (int64_t)1 << 31;     // ns and P stay below it
constexpr int VQ_NONE = 0x7fffffff;                // "no centroid yet" in a partial result
constexpr int VQ_STUCK = -1;                       // "dist(x, c_0) is NaN": the reference's scan keeps it

struct VqTiling {
  int64_t point_tiles, cent_tiles;
  int splits, tiles_per_split;
};
// Pure host function of the sizes: one workgroup per point tile when they fill the grid, else the centroid tiles are dealt to as
// many splits as bring the launch to about 2 VQ_FILL workgroups (at most VQ_MAX_SPLITS, at most one per centroid tile).
inline VqTiling vq_tiling(int64_t d, int64_t ns, int64_t P) {
  (void)d;
  VqTiling t;
  t.point_tiles = (ns + VQ_POINT_TILE - 1) / VQ_POINT_TILE;
  t.cent_tiles = (P + VQ_CENT_TILE - 1) / VQ_CENT_TILE;
  int64_t want = t.point_tiles >= VQ_FILL ? 1 : (2 * VQ_FILL + t.point_tiles - 1) / t.point_tiles;
  want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, t.cent_tiles), VQ_MAX_SPLITS));
  const int64_t per = (t.cent_tiles + want - 1) / want;
  t.tiles_per_split = (int)std::min<int64_t>(per, INT32_MAX);
  t.splits = (int)((t.cent_tiles + per - 1) / per);
  return t;
}

// (d, p) replaces (bd, bp) in a lexicographic minimum of partial results; VQ_STUCK wins over everything, VQ_NONE over nothing
__device__ __forceinline__ bool vq_takes(double d, int p, double bd, int bp) {
  if (bp == VQ_STUCK || p == VQ_NONE) return false;
  if (p == VQ_STUCK || bp == VQ_NONE) return true;
  return d < bd || (d == bd && p < bp);
}

// grid (point tiles, splits). Split y covers the centroid tiles [y * tiles_per_split, (y + 1) * tiles_per_split) and writes
// its winner for every sample to part_d / part_p [y * ns + s].
__global__ __launch_bounds__(VQ_NT) void k_vq_assign(int d, int ns, int P, const double *__restrict__ X, long long ldx,
                                                     const double *__restrict__ C, long long ldc, int tiles_per_split,
                                                     double *__restrict__ part_d, int *__restrict__ part_p, const int *skip) {
  if (skip && *skip) return;
  __shared__ __attribute__((aligned(16))) double sX[VQ_K_CHUNK * VQ_XS];
  __shared__ __attribute__((aligned(16))) double sC[VQ_K_CHUNK * VQ_CENT_TILE];
  __shared__ double red_d[VQ_WAVES * VQ_POINT_TILE];
  __shared__ int red_p[VQ_WAVES * VQ_POINT_TILE];
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long s0 = (long long)blockIdx.x * VQ_POINT_TILE;
  const int npts = (int)min((long long)VQ_POINT_TILE, (long long)ns - s0);
  const long long p_begin = (long long)blockIdx.y * tiles_per_split * VQ_CENT_TILE;
  double best_d[VQ_PR];
  int best_p[VQ_PR];
#pragma unroll
  for (int i = 0; i < VQ_PR; ++i) { best_d[i] = HUGE_VAL; best_p[i] = VQ_NONE; }

  for (int t = 0; t < tiles_per_split; ++t) {
    const long long pt0 = p_begin + (long long)t * VQ_CENT_TILE;
    if (pt0 >= P) break;   // the same for the whole workgroup
    const int ncent = (int)min((long long)VQ_CENT_TILE, (long long)P - pt0);
    const bool wave_live = w * VQ_CR < ncent;   // a wave whose centroids are all padding only helps staging
    double acc[VQ_PR][VQ_CR];
#pragma unroll
    for (int i = 0; i < VQ_PR; ++i)
#pragma unroll
      for (int j = 0; j < VQ_CR; ++j) acc[i][j] = 0.0;
    for (int k0 = 0; k0 < d; k0 += VQ_K_CHUNK) {
      const int klen = min(VQ_K_CHUNK, d - k0);
      __syncthreads();   // the previous chunk has been consumed
      for (int e = tid; e < VQ_K_CHUNK * VQ_POINT_TILE; e += VQ_NT) {
        const int k = e % VQ_K_CHUNK, s = e / VQ_K_CHUNK;   // consecutive threads read consecutive coordinates of one sample
        sX[k * VQ_XS + s] = (k < klen && s < npts) ? X[(size_t)(s0 + s) * ldx + k0 + k] : 0.0;
      }
      for (int e = tid; e < VQ_K_CHUNK * VQ_CENT_TILE; e += VQ_NT) {
        const int k = e % VQ_K_CHUNK, c = e / VQ_K_CHUNK;
        sC[k * VQ_CENT_TILE + c] = (k < klen && c < ncent) ? C[(size_t)(pt0 + c) * ldc + k0 + k] : 0.0;
      }
      __syncthreads();
      if (wave_live) {
#pragma unroll 4
        for (int k = 0; k < klen; ++k) {
          double x[VQ_PR], c[VQ_CR];
#pragma unroll
          for (int i = 0; i < VQ_PR; ++i) x[i] = sX[k * VQ_XS + i * 64 + lane];
#pragma unroll
          for (int j = 0; j < VQ_CR; ++j) c[j] = sC[k * VQ_CENT_TILE + w * VQ_CR + j];
#pragma unroll
          for (int i = 0; i < VQ_PR; ++i)
#pragma unroll
            for (int j = 0; j < VQ_CR; ++j) {
              const double df = x[i] - c[j];
              acc[i][j] = acc[i][j] + df * df;
            }
        }
      }
    }
    if (wave_live) {
#pragma unroll
      for (int j = 0; j < VQ_CR; ++j) {
        if (w * VQ_CR + j >= ncent) break;
        const long long p = pt0 + w * VQ_CR + j;   // ascending over j and over t for this thread: the strict `<` keeps the lowest p
#pragma unroll
        for (int i = 0; i < VQ_PR; ++i) {
          const double v = acc[i][j];
          if (p == 0 && v != v) { best_d[i] = v; best_p[i] = VQ_STUCK; }
          else if (best_p[i] != VQ_STUCK && v < best_d[i]) { best_d[i] = v; best_p[i] = (int)p; }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VQ_PR; ++i) {
    red_d[w * VQ_POINT_TILE + i * 64 + lane] = best_d[i];
    red_p[w * VQ_POINT_TILE + i * 64 + lane] = best_p[i];
  }
  __syncthreads();
  if (tid < npts) {
    double bd = red_d[tid];
    int bp = red_p[tid];
    for (int v = 1; v < VQ_WAVES; ++v) {
      const double dv = red_d[v * VQ_POINT_TILE + tid];
      const int pv = red_p[v * VQ_POINT_TILE + tid];
      if (vq_takes(dv, pv, bd, bp)) { bd = dv; bp = pv; }
    }
    const size_t o = (size_t)blockIdx.y * (size_t)ns + (size_t)(s0 + tid);
    part_d[o] = bd;
    part_p[o] = bp;
  }
}

// The splits' winners in ascending split order -> assign (0-based) and dist2; either may be NULL. No centroid below +Inf:
// the reference's scan is still at its start, (dist(x, c_0), 0), which is then +Inf, or the NaN that VQ_STUCK stands for.
__global__ __launch_bounds__(VQ_NT) void k_vq_finish(int ns, int splits, const double *__restrict__ part_d, const int *__restrict__ part_p,
                                                     long long *__restrict__ assign, double *__restrict__ dist2, const int *skip) {
  if (skip && *skip) return;
  for (long long s = (long long)blockIdx.x * VQ_NT + threadIdx.x; s < ns; s += (long long)gridDim.x * VQ_NT) {
    double bd = part_d[s];
    int bp = part_p[s];
    for (int z = 1; z < splits; ++z) {
      const double dv = part_d[(size_t)z * ns + s];
      const int pv = part_p[(size_t)z * ns + s];
      if (vq_takes(dv, pv, bd, bp)) { bd = dv; bp = pv; }
    }
    if (bp == VQ_NONE) { bd = HUGE_VAL; bp = 0; }
    if (bp == VQ_STUCK) bp = 0;   // bd is the NaN itself
    if (assign) assign[s] = bp;
    if (dist2) dist2[s] = bd;
  }
}

// tot[c] = Σ v[s] over the chunk c, s ascending from +0. With `mind` (seeding): first v[s] = min(mind[s], v[s]) is stored to mind.
__global__ __launch_bounds__(64) void k_vq_chunk_sums(int ns, const double *__restrict__ v, double *mind, double *__restrict__ tot, const int *skip) {
  if (skip && *skip) return;
  const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
  const long long b = c * VQ_SUM_CHUNK;
  if (b >= ns) return;
  const int len = (int)min((long long)VQ_SUM_CHUNK, (long long)ns - b);
  double acc = 0.0;
  for (int j = 0; j < len; ++j) {
    double x = v[b + j];
    if (mind) {
      const double m = mind[b + j];
      x = x < m ? x : m;
      mind[b + j] = x;
    }
    acc = acc + x;
  }
  tot[c] = acc;
}

// excl[c] = Σ tot[0 .. c) ascending from +0, *total = Σ of all. One workgroup; thread 0 adds, the others stage.
__global__ __launch_bounds__(VQ_NT) void k_vq_scan_totals(int nchunks, const double *__restrict__ tot, double *__restrict__ excl,
                                                          double *__restrict__ total, const int *skip) {
  if (skip && *skip) return;
  __shared__ double st[VQ_NT];
  double acc = 0.0;
  for (int c0 = 0; c0 < nchunks; c0 += VQ_NT) {
    const int len = min(VQ_NT, nchunks - c0);
    __syncthreads();
    if ((int)threadIdx.x < len) st[threadIdx.x] = tot[c0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < len; ++j) {
        excl[c0 + j] = acc;
        acc = acc + st[j];
      }
  }
  if (threadIdx.x == 0) *total = acc;
}

// ---- centre update
__global__ __launch_bounds__(VQ_NT) void k_vq_count(int ns, int P, const long long *__restrict__ assign, unsigned long long *counts, int *err) {
  for (long long s = (long long)blockIdx.x * VQ_NT + threadIdx.x; s < ns; s += (long long)gridDim.x * VQ_NT) {
    const long long a = assign[s];
    if (a < 0 || a >= P) { *err = 1; continue; }
    atomicAdd(&counts[a], 1ULL);
  }
}

// off[p] = Σ counts[0 .. p), off[P] = the number of samples counted. One workgroup.
__global__ __launch_bounds__(VQ_NT) void k_vq_offsets(int P, const unsigned long long *__restrict__ counts, int *__restrict__ off) {
  __shared__ int sc[VQ_NT];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  for (int p0 = 0; p0 < P; p0 += VQ_NT) {
    const int p = p0 + (int)threadIdx.x;
    const int v = p < P ? (int)counts[p] : 0;
    __syncthreads();   // carry is set; the previous tile has been read
    sc[threadIdx.x] = v;
    __syncthreads();
    for (int h = 1; h < VQ_NT; h <<= 1) {
      const int add = (int)threadIdx.x >= h ? sc[threadIdx.x - h] : 0;
      __syncthreads();
      sc[threadIdx.x] += add;
      __syncthreads();
    }
    const int base = carry;
    if (p < P) off[p] = base + sc[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == VQ_NT - 1) carry = base + sc[VQ_NT - 1];
  }
  __syncthreads();
  if (threadIdx.x == 0) off[P] = carry;
}

// members[off[p] ..] = the samples of cluster p in ascending s. The thread that owns p walks all assignments.
__global__ __launch_bounds__(VQ_NT) void k_vq_members(int ns, int P, const long long *__restrict__ assign, const int *__restrict__ off,
                                                      int *__restrict__ members) {
  __shared__ __attribute__((aligned(16))) int sa[VQ_SCAN_CHUNK];
  const long long p = (long long)blockIdx.x * VQ_NT + threadIdx.x;
  const bool live = p < P;
  int cur = live ? off[p] : 0;
  const int end = live ? off[p + 1] : 0;   // a list never grows past its own range, whatever the assignments hold
  for (long long b = 0; b < ns; b += VQ_SCAN_CHUNK) {
    const int len = (int)min((long long)VQ_SCAN_CHUNK, (long long)ns - b);
    __syncthreads();
    for (int j = threadIdx.x; j < len; j += VQ_NT) {
      const long long a = assign[b + j];
      sa[j] = (a >= 0 && a < P) ? (int)a : -1;
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < len; ++j)
        if (sa[j] == (int)p && cur < end) members[cur++] = (int)(b + j);
  }
}

// C[k, p] = (Σ_m X[k, members[m]]) / count_p, m ascending from +0; thread (cluster, coordinate). An empty cluster is skipped.
__global__ __launch_bounds__(VQ_NT) void k_vq_centres(int d, int P, int dd, int cpw, const double *__restrict__ X, long long ldx,
                                                      const int *__restrict__ members, const int *__restrict__ off, double *__restrict__ C,
                                                      long long ldc) {
  const int local = (int)threadIdx.x / dd;
  const long long p = (long long)blockIdx.x * cpw + local;
  if (local >= cpw || p >= P) return;
  const int m0 = off[p], m1 = off[p + 1];
  if (m1 == m0) return;
  const double cnt = (double)(m1 - m0);
  for (int k = (int)threadIdx.x % dd; k < d; k += dd) {
    double acc = 0.0;
    for (int m = m0; m < m1; ++m) acc = acc + X[(size_t)members[m] * ldx + k];
    C[(size_t)p * ldc + k] = acc / cnt;
  }
}

// ---- seeding
// mind[:] = +Inf on the whole grid; workgroup 0 also takes centre 0 = sample floor(u[0] * ns)
__global__ __launch_bounds__(VQ_NT) void k_vq_seed_first(int d, int ns, const double *__restrict__ X, long long ldx, const double *__restrict__ u,
                                                         double *__restrict__ mind, double *__restrict__ C, long long *__restrict__ picked) {
  for (long long s = (long long)blockIdx.x * VQ_NT + threadIdx.x; s < ns; s += (long long)gridDim.x * VQ_NT) mind[s] = HUGE_VAL;
  if (blockIdx.x != 0) return;
  const double f = floor(u[0] * (double)ns);
  long long s = f >= 0.0 ? (f < (double)ns ? (long long)f : (long long)ns - 1) : 0;   // NaN and negatives: sample 0
  for (int k = threadIdx.x; k < d; k += VQ_NT) C[k] = X[(size_t)s * ldx + k];
  if (threadIdx.x == 0) picked[0] = s;
}

// Centre j: the smallest s with prefix(s) > u[j] * total (else the smallest with prefix(s) >= total); C[:, j] = X[:, s].
// total == 0 (or not finite) raises *err and every later kernel of the seeding returns at once. One workgroup.
__global__ __launch_bounds__(VQ_NT) void k_vq_seed_pick(int j, int d, int ns, int nchunks, const double *__restrict__ X, long long ldx,
                                                        const double *__restrict__ u, const double *__restrict__ mind,
                                                        const double *__restrict__ tot, const double *__restrict__ excl,
                                                        const double *__restrict__ total, double *__restrict__ C, long long ldc,
                                                        long long *__restrict__ picked, int *err) {
  if (*err) return;
  __shared__ double sm[VQ_SUM_CHUNK];
  __shared__ int sfirst[VQ_NT];
  __shared__ int spick;
  const double T = *total;
  if (!(T > 0.0) || !(T < HUGE_VAL)) {
    __syncthreads();   // every thread has read *err
    if (threadIdx.x == 0) *err = 1;
    return;
  }
  const double thresh = u[j] * T;
  int chunk = nchunks;
  for (int mode = 0; mode < 2 && chunk == nchunks; ++mode) {   // mode 1: the fallback `>= total`
    int first = nchunks;
    for (int c = threadIdx.x; c < nchunks; c += VQ_NT) {
      const double e = excl[c] + tot[c];
      if (mode == 0 ? e > thresh : e >= T) { first = c; break; }
    }
    __syncthreads();
    sfirst[threadIdx.x] = first;
    __syncthreads();
    for (int h = VQ_NT / 2; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) sfirst[threadIdx.x] = min(sfirst[threadIdx.x], sfirst[threadIdx.x + h]);
      __syncthreads();
    }
    chunk = sfirst[0];
    if (chunk != nchunks) {
      const long long b = (long long)chunk * VQ_SUM_CHUNK;
      const int len = (int)min((long long)VQ_SUM_CHUNK, (long long)ns - b);
      if ((int)threadIdx.x < len) sm[threadIdx.x] = mind[b + threadIdx.x];
      __syncthreads();
      if (threadIdx.x == 0) {
        const double E = excl[chunk];
        double W = 0.0;
        int pick = len - 1;
        for (int q = 0; q < len; ++q) {
          W = W + sm[q];
          const double e = E + W;
          if (mode == 0 ? e > thresh : e >= T) { pick = q; break; }
        }
        spick = (int)(b + pick);
      }
    }
  }
  __syncthreads();
  if (chunk == nchunks) {   // unreachable for a finite positive total: prefix(ns - 1) == total
    if (threadIdx.x == 0) *err = 1;
    return;
  }
  const long long s = spick;
  for (int k = threadIdx.x; k < d; k += VQ_NT) C[(size_t)j * ldc + k] = X[(size_t)s * ldx + k];
  if (threadIdx.x == 0) picked[j] = s;
}

// ---- combined operator: z = Σ_i c[i] * t_i, i ascending from +0 (product, then sum); t_i = T + i * n
__global__ __launch_bounds__(NT) void k_lincomb(int n, int k, const double *__restrict__ coef, const double *__restrict__ T,
                                                double *__restrict__ z, const int *done) {
  if (done && *done) return;
  for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
    double acc = 0.0;
    for (int i = 0; i < k; ++i) acc = acc + coef[i] * T[(size_t)i * n + e];
    z[e] = acc;
  }
}

// ------------------------------------------------------------------ host side: workspace and launch sequences
// Everything below only enqueues on `s`; all pointers are device pointers. The workspace belongs to one call.
struct VqWork {
  int64_t d, ns, P;
  VqTiling t;
  int nchunks;
  DevBuf<double> part_d, tot, excl, total, tmp;   // splits x ns; chunks; chunks; 1; ns (seeding: the new distances)
  DevBuf<int> part_p, off, members, err;          // splits x ns; P + 1; ns; 1
  DevBuf<unsigned long long> cnt;                 // P
  VqWork(int64_t d_, int64_t ns_, int64_t P_) : d(d_), ns(ns_), P(P_), t(vq_tiling(d_, ns_, P_)) {
    nchunks = (int)((ns + VQ_SUM_CHUNK - 1) / VQ_SUM_CHUNK);
    part_d.alloc((size_t)t.splits * (size_t)ns);
    part_p.alloc((size_t)t.splits * (size_t)ns);
    tot.alloc((size_t)nchunks);
    excl.alloc((size_t)nchunks);
    total.alloc(1);
    err.alloc(1);
  }
  static int grid_1d(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + VQ_NT - 1) / VQ_NT, 4096)); }

  // the centroids C (d x Pc, Pc <= P) -> assign / dist2 (either may be NULL)
  void assign(hipStream_t s, const double *X, long long ldx, int64_t Pc, const double *C, long long ldc, long long *a, double *dist2,
              const int *skip) {
    const VqTiling tc = vq_tiling(d, ns, Pc);   // never more splits than the workspace holds: splits grow with P
    hipLaunchKernelGGL(k_vq_assign, dim3((unsigned)tc.point_tiles, (unsigned)tc.splits), dim3(VQ_NT), 0, s, (int)d, (int)ns, (int)Pc, X, ldx, C,
                       ldc, tc.tiles_per_split, part_d.p, part_p.p, skip);
    hipLaunchKernelGGL(k_vq_finish, dim3(grid_1d(ns)), dim3(VQ_NT), 0, s, (int)ns, tc.splits, (const double *)part_d.p, (const int *)part_p.p, a,
                       dist2, skip);
    MI_HIP(hipGetLastError());
  }
  // *total.p = Σ v in the chunked order (with `mind`: of min(mind, v), stored to mind)
  void ordered_sum(hipStream_t s, const double *v, double *mind, const int *skip) {
    hipLaunchKernelGGL(k_vq_chunk_sums, dim3((unsigned)((nchunks + 63) / 64)), dim3(64), 0, s, (int)ns, v, mind, tot.p, skip);
    hipLaunchKernelGGL(k_vq_scan_totals, dim3(1), dim3(VQ_NT), 0, s, nchunks, (const double *)tot.p, excl.p, total.p, skip);
    MI_HIP(hipGetLastError());
  }
  double read_total(hipStream_t s) {
    double out = 0.0;
    MI_HIP(hipMemcpyAsync(&out, total.p, sizeof(double), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    return out;
  }
  int read_err(hipStream_t s) {
    int out = 0;
    MI_HIP(hipMemcpyAsync(&out, err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    return out;
  }
  // counts (P) and the new centres. With `check` the call waits for the counts and returns false, with no centre
  // written, when an assignment lies outside [0, P); without it such an assignment is merely left out.
  bool update(hipStream_t s, const double *X, long long ldx, const long long *a, double *C, long long ldc, long long *counts, bool check) {
    off.ensure((size_t)P + 1);
    members.ensure((size_t)ns);
    cnt.ensure((size_t)P);
    MI_HIP(hipMemsetAsync(cnt.p, 0, (size_t)P * sizeof(long long), s));
    MI_HIP(hipMemsetAsync(err.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_vq_count, dim3(grid_1d(ns)), dim3(VQ_NT), 0, s, (int)ns, (int)P, a, cnt.p, err.p);
    if (check && read_err(s)) return false;
    MI_HIP(hipMemcpyAsync(counts, cnt.p, (size_t)P * sizeof(long long), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_vq_offsets, dim3(1), dim3(VQ_NT), 0, s, (int)P, (const unsigned long long *)cnt.p, off.p);
    hipLaunchKernelGGL(k_vq_members, dim3((unsigned)((P + VQ_NT - 1) / VQ_NT)), dim3(VQ_NT), 0, s, (int)ns, (int)P, a, (const int *)off.p, members.p);
    const int dd = (int)std::min<int64_t>(d, VQ_NT), cpw = VQ_NT / dd;
    hipLaunchKernelGGL(k_vq_centres, dim3((unsigned)((P + cpw - 1) / cpw)), dim3(VQ_NT), 0, s, (int)d, (int)P, dd, cpw, X, ldx, (const int *)members.p,
                       (const int *)off.p, C, ldc);
    MI_HIP(hipGetLastError());
    return true;
  }
  // k-means++: P uniforms u -> picked (P) and C (d x P); *err.p is raised when the distances to the chosen centres sum to 0
  void seed(hipStream_t s, const double *X, long long ldx, const double *u, long long *picked, double *C, long long ldc) {
    tmp.ensure((size_t)ns);
    DevBuf<double> mind((size_t)ns);
    MI_HIP(hipMemsetAsync(err.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_vq_seed_first, dim3(grid_1d(ns)), dim3(VQ_NT), 0, s, (int)d, (int)ns, X, ldx, u, mind.p, C, picked);
    for (int64_t j = 1; j < P; ++j) {
      assign(s, X, ldx, 1, C + (size_t)(j - 1) * ldc, ldc, nullptr, tmp.p, err.p);
      ordered_sum(s, tmp.p, mind.p, err.p);
      hipLaunchKernelGGL(k_vq_seed_pick, dim3(1), dim3(VQ_NT), 0, s, (int)j, (int)d, (int)ns, nchunks, X, ldx, u, (const double *)mind.p,
                         (const double *)tot.p, (const double *)excl.p, (const double *)total.p, C, ldc, picked, err.p);
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));   // mind goes back to the pool
  }
};

// A column-major matrix (rows x cols, leading dimension ld) or a vector (cols = 1) in the caller's pointer mode: the device
// pointer the kernels use, staged compactly for host pointers; finish() copies an output back.
template <class T>
struct VqArg {
  mi_ctx_s *c; T *user; T *dev = nullptr; long long ld; size_t rows, cols, uld; bool staged;
  DevBuf<typename std::remove_const<T>::type> buf;
  VqArg(mi_ctx_s *c_, T *p, size_t rows_, size_t cols_, long long ld_, bool read) : c(c_), user(p), ld(ld_), rows(rows_), cols(cols_), uld((size_t)ld_) {
    staged = c->ptr_mode != MI_PTR_DEVICE && p != nullptr;
    if (!staged) { dev = p; return; }
    buf.alloc(rows * cols);
    dev = buf.p; ld = (long long)rows;
    if (read) MI_HIP(hipMemcpy2DAsync((void *)dev, sizeof(T) * rows, p, sizeof(T) * uld, sizeof(T) * rows, cols, hipMemcpyHostToDevice, c->stream));
  }
  void finish() {   // the caller synchronises
    if (staged) MI_HIP(hipMemcpy2DAsync((void *)user, sizeof(T) * uld, dev, sizeof(T) * rows, sizeof(T) * rows, cols, hipMemcpyDeviceToHost, c->stream));
  }
};

// ------------------------------------------------------------------ z = Σ_i c_i (Π_i \ r)
// `InterpolatingPreconditioner` (Example14_QuantizationAndShepardLocalInterpolation_Functions.jl:73-113). The children stay the
// caller's; apply runs child i into the i-th temporary, then one k_lincomb. Nothing is allocated or synchronised in apply.
// The children are borrowed through their handles: every place a handle holds among `kid_h` is counted in its
// `bound_combine`, which refuses mi_op_destroy of a child while this operator lives (a child in two combinations, or twice
// in one, is released when the last place is gone).
struct CombineOp : Operator {
  std::vector<mi_op_s *> kid_h;
  std::vector<Operator *> kids;   // kid_h[i]->impl
  DevBuf<double> coef, tmp;   // k; k x n
  CombineOp(mi_ctx_s *c, int64_t n_, std::vector<mi_op_s *> kid_h_, const double *cf) : Operator(c, n_), kid_h(std::move(kid_h_)) {
    for (mi_op_s *h : kid_h) kids.push_back(h->impl.get());
    coef.alloc(kids.size());
    tmp.alloc(kids.size() * (size_t)n_);
    set_coefficients(cf);
    for (mi_op_s *h : kid_h) ++h->bound_combine;   // last: nothing above may leave a count behind
  }
  ~CombineOp() override {
    for (mi_op_s *h : kid_h) --h->bound_combine;
  }
  bool uses(const Operator *o) const override {
    if (o == this) return true;
    for (const Operator *k : kids)
      if (k->uses(o)) return true;
    return false;
  }
  bool usable(std::string &why) const override {
    for (const Operator *k : kids)
      if (!k->usable(why)) return false;
    return true;
  }
  // a blocking copy on the context's stream: it is ordered after the solves already enqueued, and a captured graph reads the
  // same device array afterwards
  void set_coefficients(const double *cf) {
    MI_HIP(hipMemcpyAsync(coef.p, cf, kids.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
  }
  void apply(const double *r, double *z, const int *done) override {
    for (size_t i = 0; i < kids.size(); ++i) kids[i]->apply(r, tmp.p + i * (size_t)n, done);
    hipLaunchKernelGGL(k_lincomb, dim3(grid_for(n)), dim3(NT), 0, ctx->stream, (int)n, (int)kids.size(), (const double *)coef.p,
                       (const double *)tmp.p, z, done);
    MI_HIP(hipGetLastError());
  }
  bool graph_safe() const override {
    for (const Operator *k : kids)
      if (!k->graph_safe()) return false;
    return true;
  }
  void bytes(int64_t *a, int64_t *dm) const override {
    int64_t sa = 0, sd = 0;
    for (const Operator *k : kids) {
      int64_t ka = 0, kd = 0;
      k->bytes(&ka, &kd);
      sa += ka;
      sd = std::max(sd, kd);
    }
    *a = sa + 8 * n * ((int64_t)kids.size() + 1);
    *dm = sd;
  }
  void apply_dominant(const double *x) override { kids[0]->apply_dominant(x); }
};

}  // namespace mi
