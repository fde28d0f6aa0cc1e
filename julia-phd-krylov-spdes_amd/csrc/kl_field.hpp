// Realization sampler: from a latent vector ξ to the field g = Σ_α sqrt(Λ_α) ξ_α Ψ[:, α] and the coefficient a = exp(g), for up
// to KLF_RB realizations per pass over the modes — the field half of `draw!` / `set!` (Fem/KarhunenLoeveDomainDecomposition.jl
// = "KLDD.jl" :1026-1044, :1150-1164; Fem/Samplers.jl:62-87), the factored `draw` that never forms Ψ (KLDD.jl:850-883) and
// `get_kl_coordinates` (KLDD.jl:1109-1124). Tiling and the index plan of the factored form: kl_field_plan.hpp.
//
// These are bandwidth kernels: the n x m matrix is read once per launch, column-major, one thread per row, so a wave reads
// 512 contiguous bytes of a column; KLF_UNROLL columns are requested before the first of them is used. The coefficients
// c[α, r] = sqrt(Λ_α) Ξ[α, r] are computed once per launch (k_klf_coef), staged through LDS in chunks of KLF_MODE_CHUNK modes
// (realization-minor, so every lane of a wave reads the same address: a broadcast) and shared by the whole workgroup.
//
// Bits. α runs ascending and is never split over workgroups; each term is acc = acc + c * Ψ, product then sum (the Makefile
// builds with -ffp-contract=off), starting from +0: every column of G carries the bits of the host loop
// `g += (sqrt(Λ[α]) * ξ[α]) * Ψ[:, α]`. exp is the device library's (1 ulp). The factored form sums in its own fixed order
// (y = Φ c with γ ascending; t_d = Φd[d] y_d with α ascending; the owners of a node in ascending d; a true division by
// cnt), the coordinates in a fixed order of rows per thread, threads per workgroup (a tree in LDS) and splits (ascending, as
// k_cov_reduce). No float atomics: equal calls give equal bits.
//
// Bounds. Every global load is guarded by n / m / nreal / the tile's own row count; rows past n and realizations past nreal
// are never stored; the padding up to a leading dimension is neither read nor written.
#pragma once
#include <hip/hip_runtime.h>

#include "kl_field_plan.hpp"
#include "operators.hpp"

namespace mi {

// c[α * RB + r] = sqrt_lam[α] * Xi[r * ldxi + α] for r < nreal, 0 for the accumulators beyond
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_coef(int m, int nreal, int rb, const double *__restrict__ sqrt_lam,
                                                           const double *__restrict__ Xi, long long ldxi, double *__restrict__ c) {
  const long long total = (long long)m * rb;
  for (long long e = (long long)blockIdx.x * KLF_ROW_TILE + threadIdx.x; e < total; e += (long long)gridDim.x * KLF_ROW_TILE) {
    const int a = (int)(e / rb), r = (int)(e - (long long)a * rb);
    c[e] = r < nreal ? sqrt_lam[a] * Xi[(size_t)r * ldxi + a] : 0.0;
  }
}

// acc[r] += Σ_α c[α, r] P[row, α], α = 0 .. m - 1 ascending; P column-major with leading dimension ldp, c (m x RB) in global
// memory, staged through `sc` (KLF_MODE_CHUNK * RB doubles of LDS). Every thread of the workgroup calls it (barriers);
// `live` threads load, the others only help staging.
template <int RB>
__device__ __forceinline__ void klf_mode_sum(bool live, const double *__restrict__ P, long long ldp, size_t row, int m,
                                             const double *__restrict__ c, double *sc, double (&acc)[RB]) {
  for (int a0 = 0; a0 < m; a0 += KLF_MODE_CHUNK) {
    const int len = min(KLF_MODE_CHUNK, m - a0);
    __syncthreads();   // the previous chunk has been consumed
    for (int t = threadIdx.x; t < len * RB; t += KLF_ROW_TILE) sc[t] = c[(size_t)a0 * RB + t];
    __syncthreads();
    const double *col = P + (size_t)a0 * ldp + row;
    int j = 0;
    for (; j + KLF_UNROLL <= len; j += KLF_UNROLL) {
      double v[KLF_UNROLL];
#pragma unroll
      for (int u = 0; u < KLF_UNROLL; ++u) v[u] = live ? col[(size_t)(j + u) * ldp] : 0.0;
#pragma unroll
      for (int u = 0; u < KLF_UNROLL; ++u)
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = acc[r] + sc[(j + u) * RB + r] * v[u];
    }
    for (; j < len; ++j) {
      const double v = live ? col[(size_t)j * ldp] : 0.0;
#pragma unroll
      for (int r = 0; r < RB; ++r) acc[r] = acc[r] + sc[j * RB + r] * v;
    }
  }
}

// G[i, r] = Σ_α c[α, r] Ψ[i, α], A[i, r] = exp(G[i, r]); either output may be NULL. grid: row tiles.
template <int RB>
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_dense(int n, int m, int nreal, const double *__restrict__ Psi, long long ldpsi,
                                                            const double *__restrict__ c, double *__restrict__ G, long long ldg,
                                                            double *__restrict__ A, long long lda) {
  __shared__ __attribute__((aligned(16))) double sc[KLF_MODE_CHUNK * RB];
  const long long i = (long long)blockIdx.x * KLF_ROW_TILE + threadIdx.x;
  const bool live = i < n;
  double acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = 0.0;
  klf_mode_sum<RB>(live, Psi, ldpsi, (size_t)i, m, c, sc, acc);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < RB; ++r)
    if (r < nreal) {
      if (G) G[(size_t)r * ldg + i] = acc[r];
      if (A) A[(size_t)r * lda + i] = exp(acc[r]);
    }
}

// Stage 1 of the factored form: y[row, r] = Σ_γ Φ[row, γ] c[γ, r] on the nred = Σ md rows of the reduced eigenvector block;
// y is nred x RB, compact
template <int RB>
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_reduced(int nred, int m, const double *__restrict__ Phi, const double *__restrict__ c,
                                                              double *__restrict__ y) {
  __shared__ __attribute__((aligned(16))) double sc[KLF_MODE_CHUNK * RB];
  const long long row = (long long)blockIdx.x * KLF_ROW_TILE + threadIdx.x;
  const bool live = row < nred;
  double acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = 0.0;
  klf_mode_sum<RB>(live, Phi, nred, (size_t)row, m, c, sc, acc);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < RB; ++r) y[(size_t)row * RB + r] = acc[r];   // realization-minor: stage 2 stages it as it stages c
}

// Stage 2: t[t_off[d] + l, r] = Σ_α Φd[d][l, α] y[y_off[d] + α, r] for the tile (d, row0) of blockIdx.x; t is nloc x RB with
// leading dimension nloc (a column per realization, so that the gather reads one column per realization)
template <int RB>
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_local(const klfp::Tile *__restrict__ tiles, const int *__restrict__ n_d,
                                                            const int *__restrict__ md, const int *__restrict__ y_off,
                                                            const int *__restrict__ t_off, const long long *__restrict__ phid_off,
                                                            const double *__restrict__ Phid, const double *__restrict__ y,
                                                            double *__restrict__ t, int nloc) {
  __shared__ __attribute__((aligned(16))) double sc[KLF_MODE_CHUNK * RB];
  const klfp::Tile tile = tiles[blockIdx.x];
  const int nd = n_d[tile.d];
  const int l = tile.row0 + (int)threadIdx.x;
  const bool live = l < nd;
  double acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = 0.0;
  klf_mode_sum<RB>(live, Phid + phid_off[tile.d], nd, (size_t)l, md[tile.d], y + (size_t)y_off[tile.d] * RB, sc, acc);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < RB; ++r) t[(size_t)r * nloc + t_off[tile.d] + l] = acc[r];
}

// Stage 3: G[i, r] = (Σ_{k in own_ptr[i] .. own_ptr[i + 1]} t[own_pos[k], r]) / cnt_i, the owners in ascending d
template <int RB>
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_gather(int n, int nreal, const int *__restrict__ own_ptr, const int *__restrict__ own_pos,
                                                             const double *__restrict__ t, int nloc, double *__restrict__ G, long long ldg,
                                                             double *__restrict__ A, long long lda) {
  const long long i = (long long)blockIdx.x * KLF_ROW_TILE + threadIdx.x;
  if (i >= n) return;
  const int k0 = own_ptr[i], k1 = own_ptr[i + 1];
  double acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int p = own_pos[k];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = acc[r] + t[(size_t)r * nloc + p];
  }
  const double cnt = (double)(k1 - k0);
#pragma unroll
  for (int r = 0; r < RB; ++r)
    if (r < nreal) {
      const double g = acc[r] / cnt;
      if (G) G[(size_t)r * ldg + i] = g;
      if (A) A[(size_t)r * lda + i] = exp(g);
    }
}

// Coordinates: part[z][α] = Σ_{i in split z} Ψ[i, α] w[i] with w = M g. grid (splits, column blocks of KLF_RB). A thread sums
// its rows (row tile by row tile, ascending), then the threads are added by a tree in LDS: a fixed order.
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_coords(int n, int m, const double *__restrict__ Psi, long long ldpsi,
                                                             const double *__restrict__ w, int rows_per_split, double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double red[KLF_ROW_TILE * KLF_RB];
  const int a0 = (int)blockIdx.y * KLF_RB;
  const int ncol = min(KLF_RB, m - a0);
  const long long r_begin = (long long)blockIdx.x * rows_per_split;
  const long long r_end = min((long long)n, r_begin + rows_per_split);
  double acc[KLF_RB];
#pragma unroll
  for (int c = 0; c < KLF_RB; ++c) acc[c] = 0.0;
  for (long long i = r_begin + threadIdx.x; i < r_end; i += KLF_ROW_TILE) {
    const double wi = w[i];
    double v[KLF_RB];
#pragma unroll
    for (int c = 0; c < KLF_RB; ++c) v[c] = c < ncol ? Psi[(size_t)(a0 + c) * ldpsi + i] : 0.0;
#pragma unroll
    for (int c = 0; c < KLF_RB; ++c) acc[c] = acc[c] + v[c] * wi;
  }
#pragma unroll
  for (int c = 0; c < KLF_RB; ++c) red[c * KLF_ROW_TILE + threadIdx.x] = acc[c];
  __syncthreads();
  for (int half = KLF_ROW_TILE / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
#pragma unroll
      for (int c = 0; c < KLF_RB; ++c) red[c * KLF_ROW_TILE + threadIdx.x] = red[c * KLF_ROW_TILE + threadIdx.x] + red[c * KLF_ROW_TILE + threadIdx.x + half];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < ncol) part[(size_t)blockIdx.x * m + a0 + threadIdx.x] = red[threadIdx.x * KLF_ROW_TILE];
}

// ξ[α] = (Σ_z part[z][α]) / sqrt_lam[α], z ascending
__global__ __launch_bounds__(KLF_ROW_TILE) void k_klf_coords_reduce(int m, int splits, const double *__restrict__ part,
                                                                    const double *__restrict__ sqrt_lam, double *__restrict__ xi) {
  const int a = (int)blockIdx.x * KLF_ROW_TILE + (int)threadIdx.x;
  if (a >= m) return;
  double s = part[a];
  for (int z = 1; z < splits; ++z) s = s + part[(size_t)z * m + a];
  xi[a] = s / sqrt_lam[a];
}

}  // namespace mi

// ------------------------------------------------------------------ the handle
// Everything a set or a coordinates call needs is allocated at creation: in device-pointer mode they only enqueue kernels on the
// context's stream (no allocation, no synchronisation; legal inside a capture).
struct mi_kl_field_s {
  mi_ctx_s *ctx = nullptr;
  int n = 0, m = 0;
  bool dd = false;
  std::vector<double> lam;                  // host copy: Λ_α == 0 is refused by the coordinates only
  mi::DevBuf<double> sqrt_lam, c;           // m; m x KLF_RB
  // dense form
  mi::DevBuf<double> Psi;                   // n x m, compact
  mi::DevBuf<double> w, part;               // coordinates: M g; coord_splits x m partial sums (coord_splits <= KLF_MAX_SPLITS)
  // factored form
  mi::klfp::Plan plan;
  mi::DevBuf<double> Phi, Phid, y, t;       // nred x m; Σ n_d md_d; nred x KLF_RB; nloc x KLF_RB
  mi::DevBuf<mi::klfp::Tile> tiles;
  mi::DevBuf<int> n_d, md, y_off, t_off, own_ptr, own_pos;
  mi::DevBuf<long long> phid_off;
  int64_t bytes_kept = 0, bytes_per_set = 0;

  // up to KLF_RB realizations: Xi (m x nreal, leading dimension ldxi), G and A (n x nreal) are device pointers
  void launch_set(int nreal, const double *Xi, long long ldxi, double *G, long long ldg, double *A, long long lda) {
    using namespace mi;
    hipStream_t s = ctx->stream;
    const int rb = klf_rb_in_use(nreal);
    const int gc = (int)std::min<long long>(((long long)m * rb + KLF_ROW_TILE - 1) / KLF_ROW_TILE, 1024);
    hipLaunchKernelGGL(k_klf_coef, dim3(gc), dim3(KLF_ROW_TILE), 0, s, m, nreal, rb, (const double *)sqrt_lam.p, Xi, ldxi, c.p);
    const dim3 rows((unsigned)((n + KLF_ROW_TILE - 1) / KLF_ROW_TILE)), wg(KLF_ROW_TILE);
#define MI_KLF_RB(GO) \
  switch (rb) {       \
    case 1: GO(1); break; \
    case 2: GO(2); break; \
    case 4: GO(4); break; \
    default: GO(KLF_RB); break; \
  }
    if (!dd) {
#define MI_KLF_DENSE(RB) hipLaunchKernelGGL((k_klf_dense<RB>), rows, wg, 0, s, n, m, nreal, (const double *)Psi.p, (long long)n, (const double *)c.p, G, ldg, A, lda)
      MI_KLF_RB(MI_KLF_DENSE)
#undef MI_KLF_DENSE
    } else {
      const dim3 red((unsigned)((plan.nred + KLF_ROW_TILE - 1) / KLF_ROW_TILE)), loc((unsigned)plan.tiles.size());
#define MI_KLF_DD(RB)                                                                                                                         \
  hipLaunchKernelGGL((k_klf_reduced<RB>), red, wg, 0, s, plan.nred, m, (const double *)Phi.p, (const double *)c.p, y.p);                       \
  hipLaunchKernelGGL((k_klf_local<RB>), loc, wg, 0, s, (const klfp::Tile *)tiles.p, (const int *)n_d.p, (const int *)md.p, (const int *)y_off.p, \
                     (const int *)t_off.p, (const long long *)phid_off.p, (const double *)Phid.p, (const double *)y.p, t.p, plan.nloc);        \
  hipLaunchKernelGGL((k_klf_gather<RB>), rows, wg, 0, s, n, nreal, (const int *)own_ptr.p, (const int *)own_pos.p, (const double *)t.p,        \
                     plan.nloc, G, ldg, A, lda)
      MI_KLF_RB(MI_KLF_DD)
#undef MI_KLF_DD
    }
#undef MI_KLF_RB
    MI_HIP(hipGetLastError());
  }

  // ξ = Ψ' (M g) ./ sqrt(Λ): g and xi are device pointers (dense form)
  void launch_coords(const mi::CsrDev &M, const double *g, double *xi) {
    using namespace mi;
    hipStream_t s = ctx->stream;
    M.launch(0, g, nullptr, w.p, nullptr, s);
    const KlfTiling tl = klf_tiling(n, m, 1);
    hipLaunchKernelGGL(k_klf_coords, dim3(tl.coord_splits, tl.coord_col_blocks), dim3(KLF_ROW_TILE), 0, s, n, m, (const double *)Psi.p,
                       (long long)n, (const double *)w.p, tl.coord_tiles_per_split * KLF_ROW_TILE, part.p);
    hipLaunchKernelGGL(k_klf_coords_reduce, dim3((m + KLF_ROW_TILE - 1) / KLF_ROW_TILE), dim3(KLF_ROW_TILE), 0, s, m, tl.coord_splits,
                       (const double *)part.p, (const double *)sqrt_lam.p, xi);
    MI_HIP(hipGetLastError());
  }
};
