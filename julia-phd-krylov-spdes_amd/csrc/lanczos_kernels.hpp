// Device side of the thick-restart Lanczos eigensolver (lanczos.hpp; mi_eigsolve): the full re-orthogonalisation of the new
// Krylov vector against the basis panel V (n x (m+1), column-major, HBM resident), classical Gram-Schmidt applied twice.
// Per step, after the operator apply(s):
//   k_lz_project         part1[c, wg] = partial of V[:, c] . x           (x = w; generalized: x = u = A v_j = B w)
//   k_lz_update_project  h = Σ part1;  w -= V h;  part2[c, wg] = partial of V[:, c] . w_new   (standard problem: same launch)
//   k_lz_update_norm     h2 = Σ part2; w -= V h2 (u -= Q h2);  partn[wg] = partial of w'w (w'u);  T[:, j] = h + h2
//   k_lz_commit          beta = sqrt(Σ partn);  v_{j+1} = w / beta (q_{j+1} = u / beta);  break-down / non-finite flags
//
// Layout. The panels have an EVEN leading dimension ld >= n (rows n .. ld-1 are zero), so that every column starts on a
// 16-byte boundary and a thread's rows come as double2 loads. A workgroup walks tiles of LZ_TILE = 4 NT rows (two double2 per
// thread): it holds its slice of the vector in registers and streams the slice of every active column, LZ_CT columns at a
// time — 2 LZ_CT independent 16-byte loads in flight per thread. Per tile and column group the four waves' sums meet in LDS
// (double-buffered: one barrier per group) and are added to the workgroup's accumulator of that column, tiles ascending:
// fixed orders everywhere, no atomics, so a call is bitwise reproducible.
//
// Stop flags. Step j reads status[j] (written by the commit of step j-1) and its commit writes status[j+1]: no kernel reads a
// word another workgroup of the same launch writes. 0: go on; LZ_BREAKDOWN: beta <= 64 eps max|T| (V[:, :j+1] is invariant);
// LZ_NONFINITE: beta or T[:, j] is not finite. A step behind a raised flag does nothing but pass the flag on, so all steps
// up to the end of the window replay as one graph whatever happens inside it.
#pragma once
#include "kernels.hpp"

namespace mi {

constexpr int LZ_TILE = 4 * NT;  // rows per workgroup and tile = rows per workgroup of vec_grid(n) below MAX_PARTS workgroups
constexpr int LZ_CT = 4;         // columns whose loads are issued together
constexpr int LZ_NW = NT / 64;

enum { LZ_RUN = 0, LZ_BREAKDOWN = 1, LZ_NONFINITE = 2 };
enum { LZ_STEP = 0, LZ_LAST_OF_FULL_SPACE = 1, LZ_NEW_VECTOR = 2 };  // k_lz_commit modes

// rows r, r+1 of a vector with zero padding up to an even length (r even); rows >= n read as zero
__device__ __forceinline__ double2 lz_load2(const double *__restrict__ p, long long r, int n) {
  double2 v = make_double2(0.0, 0.0);
  if (r < n) {
    v = *reinterpret_cast<const double2 *>(p + r);
    if (r + 1 >= n) v.y = 0.0;
  }
  return v;
}
__device__ __forceinline__ void lz_store2(double *__restrict__ p, long long r, int n, double2 v) {
  if (r < n) {
    if (r + 1 >= n) v.y = 0.0;
    *reinterpret_cast<double2 *>(p + r) = v;
  }
}

// h[c] = Σ_b part[c * g + b], b ascending within a lane, then the shuffle tree: the same bits in every workgroup.
__device__ __forceinline__ void lz_reduce_h(const double *__restrict__ part, int g, int ncols, double *h) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < ncols; c += LZ_NW) {
    double s = 0.0;
    for (int b = lane; b < g; b += 64) s += part[(long long)c * g + b];
    s = wave_sum(s);
    if (lane == 0) h[c] = s;
  }
  __syncthreads();
}

// acc[c] += V[rows of this thread's tile, c] . (x0, x1) summed over the workgroup, for every c < ncols.
// wv: 2 * LZ_NW * LZ_CT doubles; `flip` alternates its halves from group to group and is carried across calls.
__device__ __forceinline__ void lz_tile_dots(const double *__restrict__ V, long long ld, int n, int ncols, long long r0, long long r1,
                                             double2 x0, double2 x1, double *acc, double *wv, int &flip) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c0 = 0; c0 < ncols; c0 += LZ_CT) {
    double2 a[LZ_CT], b[LZ_CT];
#pragma unroll
    for (int k = 0; k < LZ_CT; ++k) {
      const double *col = V + (long long)min(c0 + k, ncols - 1) * ld;   // past the last column: a valid load, discarded below
      a[k] = lz_load2(col, r0, n);
      b[k] = lz_load2(col, r1, n);
    }
    double *buf = wv + flip * (LZ_NW * LZ_CT);
#pragma unroll
    for (int k = 0; k < LZ_CT; ++k) {
      double s = a[k].x * x0.x + a[k].y * x0.y + b[k].x * x1.x + b[k].y * x1.y;
      s = wave_sum(s);
      if (lane == 0) buf[wave * LZ_CT + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < LZ_CT && c0 + (int)threadIdx.x < ncols) {
      double s = buf[threadIdx.x];
#pragma unroll
      for (int w = 1; w < LZ_NW; ++w) s += buf[w * LZ_CT + threadIdx.x];
      acc[c0 + threadIdx.x] += s;
    }
    flip ^= 1;
  }
}

// (x0, x1) -= Σ_c V[rows, c] * h[c], c ascending; with Q also (y0, y1) -= Σ_c Q[rows, c] * h[c].
__device__ __forceinline__ void lz_tile_axpys(const double *__restrict__ V, const double *__restrict__ Q, long long ld, int n,
                                              int ncols, long long r0, long long r1, const double *h, double2 &x0, double2 &x1,
                                              double2 &y0, double2 &y1) {
  for (int c0 = 0; c0 < ncols; c0 += LZ_CT) {
    double2 a[LZ_CT], b[LZ_CT], qa[LZ_CT], qb[LZ_CT];
#pragma unroll
    for (int k = 0; k < LZ_CT; ++k) {
      const long long off = (long long)min(c0 + k, ncols - 1) * ld;
      a[k] = lz_load2(V + off, r0, n);
      b[k] = lz_load2(V + off, r1, n);
      if (Q) {
        qa[k] = lz_load2(Q + off, r0, n);
        qb[k] = lz_load2(Q + off, r1, n);
      }
    }
#pragma unroll
    for (int k = 0; k < LZ_CT; ++k) {
      if (c0 + k < ncols) {
        const double hc = h[c0 + k];
        x0.x -= a[k].x * hc; x0.y -= a[k].y * hc;
        x1.x -= b[k].x * hc; x1.y -= b[k].y * hc;
        if (Q) {
          y0.x -= qa[k].x * hc; y0.y -= qa[k].y * hc;
          y1.x -= qb[k].x * hc; y1.y -= qb[k].y * hc;
        }
      }
    }
  }
}

// Dynamic LDS of the three sweeps: ncols coefficients + ncols accumulators + the waves' hand-over buffer.
inline size_t lz_lds_bytes(int ncols) { return sizeof(double) * (2 * (size_t)ncols + 2 * LZ_NW * LZ_CT); }

// part[c * gridDim.x + wg] = partial of V[:, c] . x, c < ncols. grid vec_grid(n).
__global__ __launch_bounds__(NT) void k_lz_project(int n, long long ld, int ncols, const double *__restrict__ V,
                                                   const double *__restrict__ x, double *__restrict__ part, const int *stop) {
  if (stop && *stop) return;
  extern __shared__ double lz_lds[];
  double *acc = lz_lds + ncols, *wv = lz_lds + 2 * ncols;
  for (int c = threadIdx.x; c < ncols; c += NT) acc[c] = 0.0;
  __syncthreads();
  int flip = 0;
  for (long long t0 = (long long)blockIdx.x * LZ_TILE; t0 < n; t0 += (long long)gridDim.x * LZ_TILE) {
    const long long r0 = t0 + 2 * threadIdx.x, r1 = r0 + 2 * NT;
    const double2 x0 = lz_load2(x, r0, n), x1 = lz_load2(x, r1, n);
    lz_tile_dots(V, ld, n, ncols, r0, r1, x0, x1, acc, wv, flip);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ncols; c += NT) part[(long long)c * gridDim.x + blockIdx.x] = acc[c];
}

// h = Σ part_in (every workgroup, redundantly); w -= V h; workgroup 0 keeps h in hsave. With part_out also the partials of
// V' w_new for the workgroup's rows: w_new[i] depends on h and row i only, so the second projection rides in this launch on
// the registers that hold w_new — no further launch and no further sweep of w (the V slice of the tile is read a second
// time, from cache where it fits).
__global__ __launch_bounds__(NT) void k_lz_update_project(int n, long long ld, int ncols, const double *__restrict__ V,
                                                          double *__restrict__ w, const double *__restrict__ part_in,
                                                          double *__restrict__ hsave, double *__restrict__ part_out,
                                                          const int *stop) {
  if (stop && *stop) return;
  extern __shared__ double lz_lds[];
  double *h = lz_lds, *acc = lz_lds + ncols, *wv = lz_lds + 2 * ncols;
  for (int c = threadIdx.x; c < ncols; c += NT) acc[c] = 0.0;
  lz_reduce_h(part_in, gridDim.x, ncols, h);
  if (blockIdx.x == 0 && hsave)
    for (int c = threadIdx.x; c < ncols; c += NT) hsave[c] = h[c];
  int flip = 0;
  for (long long t0 = (long long)blockIdx.x * LZ_TILE; t0 < n; t0 += (long long)gridDim.x * LZ_TILE) {
    const long long r0 = t0 + 2 * threadIdx.x, r1 = r0 + 2 * NT;
    double2 x0 = lz_load2(w, r0, n), x1 = lz_load2(w, r1, n), y0 = x0, y1 = x1;
    lz_tile_axpys(V, nullptr, ld, n, ncols, r0, r1, h, x0, x1, y0, y1);
    lz_store2(w, r0, n, x0);
    lz_store2(w, r1, n, x1);
    if (part_out) lz_tile_dots(V, ld, n, ncols, r0, r1, x0, x1, acc, wv, flip);
  }
  if (!part_out) return;
  __syncthreads();
  for (int c = threadIdx.x; c < ncols; c += NT) part_out[(long long)c * gridDim.x + blockIdx.x] = acc[c];
}

// h2 = Σ part_in; w -= V h2 (generalized: also u -= Q h2); partn[wg] = partial of w'w (w'u). Workgroup 0 writes the upper
// part of column jcol of the projected matrix, T[c, jcol] = h1[c] + h2[c] (Tcol == nullptr: a new start vector, no column).
// ncols == 0: only the norm (the start vector).
__global__ __launch_bounds__(NT) void k_lz_update_norm(int n, long long ld, int ncols, const double *__restrict__ V,
                                                       const double *__restrict__ Q, double *__restrict__ w,
                                                       double *__restrict__ u, const double *__restrict__ part_in,
                                                       const double *__restrict__ h1, double *__restrict__ Tcol,
                                                       double *__restrict__ partn, const int *stop) {
  if (stop && *stop) return;
  extern __shared__ double lz_lds[];
  __shared__ double sm[NT / 64 + 1];
  double *h = lz_lds;
  if (ncols > 0) lz_reduce_h(part_in, gridDim.x, ncols, h);
  if (blockIdx.x == 0 && Tcol)
    for (int c = threadIdx.x; c < ncols; c += NT) Tcol[c] = (h1 ? h1[c] : 0.0) + h[c];
  double s = 0.0;
  for (long long t0 = (long long)blockIdx.x * LZ_TILE; t0 < n; t0 += (long long)gridDim.x * LZ_TILE) {
    const long long r0 = t0 + 2 * threadIdx.x, r1 = r0 + 2 * NT;
    double2 x0 = lz_load2(w, r0, n), x1 = lz_load2(w, r1, n);
    double2 y0 = x0, y1 = x1;
    if (u) { y0 = lz_load2(u, r0, n); y1 = lz_load2(u, r1, n); }
    if (ncols > 0) {
      lz_tile_axpys(V, u ? Q : nullptr, ld, n, ncols, r0, r1, h, x0, x1, y0, y1);
      lz_store2(w, r0, n, x0);
      lz_store2(w, r1, n, x1);
      if (u) { lz_store2(u, r0, n, y0); lz_store2(u, r1, n, y1); }
    }
    if (!u) { y0 = x0; y1 = x1; }
    s += x0.x * y0.x + x0.y * y0.y + x1.x * y1.x + x1.y * y1.y;
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) partn[blockIdx.x] = s;
}

// beta = sqrt(Σ partn) (every workgroup, the same bits); unless a flag is raised, vdst = w / beta (qdst = u / beta).
// Workgroup 0 writes status_out, beta_out and the running max|T| (tmax_out = max(tmax_prev, max_c |Tcol[c]|)).
//   LZ_STEP                  : LZ_NONFINITE if beta or a Tcol entry is not finite, LZ_BREAKDOWN if beta <= 64 eps max|T|
//   LZ_LAST_OF_FULL_SPACE    : the basis spans the whole space (m == n, j == n - 1): beta is rounding noise, nothing is scaled
//   LZ_NEW_VECTOR            : start vector / fresh vector after a break-down: LZ_NONFINITE if beta is not finite or zero
__global__ __launch_bounds__(NT) void k_lz_commit(int n, int g, int ncols, const double *__restrict__ partn,
                                                  const double *__restrict__ w, const double *__restrict__ u,
                                                  double *__restrict__ vdst, double *__restrict__ qdst,
                                                  const double *__restrict__ Tcol, const int *status_in, int *status_out,
                                                  double *beta_out, const double *tmax_prev, double *tmax_out, int mode) {
  const int in = status_in ? *status_in : LZ_RUN;
  if (in != LZ_RUN) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *status_out = in;
    return;
  }
  __shared__ double sm[NT / 64 + 1];
  const double beta = sqrt(sum_partials(partn, g, sm));
  double mx = tmax_prev ? *tmax_prev : 0.0, bad = 0.0;
  if (Tcol)
    for (int c = threadIdx.x; c < ncols; c += NT) {
      const double t = fabs(Tcol[c]);
      if (isfinite(t)) mx = fmax(mx, t);
      else bad = 1.0;
    }
  bad = block_sum(bad, sm);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = sm[0];
#pragma unroll
  for (int k = 1; k < NT / 64; ++k) mx = fmax(mx, sm[k]);
  int st = LZ_RUN;
  if (bad != 0.0 || !isfinite(beta)) st = LZ_NONFINITE;
  else if (mode == LZ_NEW_VECTOR) st = beta > 0.0 ? LZ_RUN : LZ_NONFINITE;
  else if (mode == LZ_STEP && beta <= 64.0 * 2.220446049250313e-16 * mx) st = LZ_BREAKDOWN;
  if (st == LZ_RUN && mode != LZ_LAST_OF_FULL_SPACE)
    for (long long t0 = (long long)blockIdx.x * LZ_TILE; t0 < n; t0 += (long long)gridDim.x * LZ_TILE) {
      const long long r0 = t0 + 2 * threadIdx.x, r1 = r0 + 2 * NT;
      double2 x0 = lz_load2(w, r0, n), x1 = lz_load2(w, r1, n);
      x0.x /= beta; x0.y /= beta; x1.x /= beta; x1.y /= beta;
      lz_store2(vdst, r0, n, x0);
      lz_store2(vdst, r1, n, x1);
      if (u) {
        double2 y0 = lz_load2(u, r0, n), y1 = lz_load2(u, r1, n);
        y0.x /= beta; y0.y /= beta; y1.x /= beta; y1.y /= beta;
        lz_store2(qdst, r0, n, y0);
        lz_store2(qdst, r1, n, y1);
      }
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *status_out = st;
    *beta_out = beta;
    if (tmax_out) *tmax_out = mx;
  }
}

}  // namespace mi
