// Sparse direct `M \ r` for a sparse SPD matrix with an interface-like graph: the `A_ΓΓ` that RecyclingKrylovSolvers'
// pcg applies as `z .= M \ r` (cg.jl:85, 100) in Example07:412/416, `pcg(S, b_schur, zeros(S.N), A_ΓΓ)`.
//
// One level of nested dissection (spd_direct_plan.hpp, host, once per pattern): pieces of <= P nodes, separator Σ.
//   numeric (device, per set of values; no atomics, fixed summation orders — bitwise reproducible):
//     k_sd_scatter   the stored values into dense D_i, B_i' and A_ΣΣ
//     k_sd_factor    one workgroup per piece, in LDS: D_i^-1 (Gauss-Jordan, no pivoting: every pivot of an SPD block is
//                    positive), G_i = D_i^-1 B_i' (n_i x |Σ_i|) and the patch B_i G_i (|Σ_i| x |Σ_i|)
//     k_sd_schur     s = A_ΣΣ - Σ_i patch_i, the patches of an entry summed in ascending piece order
//     s^-1           the same LDS kernel when |Σ| <= P_MAX, else one Gauss-Jordan step per launch; then the probe certificate
//                    of mi_nn_pinv (setup_gj.hpp): ||v - Z s v||_inf <= 4 |Σ| eps ||Z||_inf ||s||_inf, v = ±1
//   A pivot that is not positive (relative to its original diagonal entry) or a failed certificate is MI_ERR_SINGULAR, and
//   the operator keeps its previous factor: a later solve never sees NaNs.
//   apply (2 launches):
//     k_sd_apply1    one workgroup per piece: y_i = D_i^-1 r_i, and G_i' r_i into the slots (Σ node, piece)
//     k_sd_apply2    one workgroup per piece (+ one for Σ nodes adjacent to no piece): t = r_Σ - Σ slots (ascending piece),
//                    z_Σ rows of Σ_i = s^-1[Σ_i, :] t, z_i = y_i - G_i z_Σi. A Σ node is written by its first piece.
#pragma once
#include "setup_gj.hpp"
#include "spd_direct_plan.hpp"

namespace mi {

struct SdPlanDev {   // device arrays of the plan, by value into the kernels
  int n_pieces, ns, n_orphan;
  const int *piece_ptr, *piece_node, *sigma, *sig_ptr, *sig_idx, *slot_ptr, *slot, *slot_piece, *orphan;
  const int64_t *d_off, *b_off, *s_off;
};

__global__ __launch_bounds__(256) void k_sd_scatter(int64_t nnz, const int64_t *__restrict__ dst, const double *__restrict__ val,
                                                    double *__restrict__ work) {
  for (int64_t k = blockIdx.x * 256ll + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) {
    const int64_t d = dst[k];
    if (d >= 0) work[d] = val[k];
  }
}

// In-place inverse of the SPD n x n matrix M (LDS, column-major, leading dimension ld) by scalar Gauss-Jordan without
// pivoting, all 256 threads; `row`, `col`, `dg`: n doubles of LDS each. Returns (uniformly) false when a pivot is not
// positive and finite or not above n eps times its original diagonal entry (a singular or indefinite block).
__device__ bool sd_gj_lds(double *M, int n, int ld, double *row, double *col, double *dg) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) dg[i] = M[i + i * ld];
  __syncthreads();
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    const double p = M[k + k * ld];
    ok = ok && isfinite(p) && p > (double)n * 2.220446049250313e-16 * dg[k];
    const double ip = 1.0 / p;
    for (int i = tid; i < n; i += 256) { row[i] = M[k + i * ld]; col[i] = M[i + k * ld]; }
    __syncthreads();
    for (int e = tid; e < n * n; e += 256) {
      const int i = e % n, j = e / n;
      const double rk = row[j] * ip;
      double v;
      if (i == k) v = j == k ? ip : rk;
      else v = j == k ? -col[i] * ip : M[i + j * ld] - col[i] * rk;
      M[i + j * ld] = v;
    }
    __syncthreads();
  }
  return ok;
}

// LDS of k_sd_factor / k_sd_invert: an m x (m + 1) matrix and three vectors of m
inline size_t sd_lds_bytes(int m) { return sizeof(double) * ((size_t)m * (m + 1) + 3 * (size_t)m); }

// one workgroup per piece: dinv_i, G_i = D_i^-1 B_i', patch_i = B_i G_i; flag[0] = 1 on a bad pivot
__global__ __launch_bounds__(256) void k_sd_factor(SdPlanDev p, int64_t d_total, const double *__restrict__ work,
                                                   double *__restrict__ dinv, double *__restrict__ G, double *__restrict__ patch,
                                                   int *__restrict__ flag) {
  extern __shared__ double sm[];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int ni = p.piece_ptr[i + 1] - p.piece_ptr[i], si = p.sig_ptr[i + 1] - p.sig_ptr[i], ld = ni + 1;
  double *M = sm, *row = sm + (size_t)ni * ld, *col = row + ni, *dg = col + ni;
  const double *D = work + p.d_off[i], *Bt = work + d_total + p.b_off[i];
  for (int e = tid; e < ni * ni; e += 256) M[e % ni + (e / ni) * ld] = D[e];
  __syncthreads();
  if (!sd_gj_lds(M, ni, ld, row, col, dg) && tid == 0) flag[0] = 1;
  double *Di = dinv + p.d_off[i], *Gi = G + p.b_off[i];
  for (int e = tid; e < ni * ni; e += 256) Di[e] = M[e % ni + (e / ni) * ld];
  for (int e = tid; e < ni * si; e += 256) {
    const int r = e % ni, k = e / ni;
    double acc = 0.0;
    for (int c = 0; c < ni; ++c) acc += M[r + c * ld] * Bt[c + (size_t)k * ni];
    Gi[e] = acc;
  }
  __syncthreads();   // G_i (global) written by this workgroup before it reads it back
  double *Pi = patch + p.s_off[i];
  for (int e = tid; e < si * si; e += 256) {
    const int k1 = e % si, k2 = e / si;
    double acc = 0.0;
    for (int c = 0; c < ni; ++c) acc += Bt[c + (size_t)k1 * ni] * Gi[c + (size_t)k2 * ni];
    Pi[e] = acc;
  }
}

// s = A_ΣΣ - Σ_i patch_i (column-major), one thread per entry; the patches that hold entry (a, b) are those of the pieces
// in the slot list of a that also have b in Σ_i, summed in ascending piece order
__global__ __launch_bounds__(256) void k_sd_schur(SdPlanDev p, const double *__restrict__ Ass, const double *__restrict__ patch,
                                                  double *__restrict__ S) {
  const int ns = p.ns;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < (int64_t)ns * ns; e += (int64_t)gridDim.x * 256) {
    const int a = (int)(e % ns), b = (int)(e / ns);
    double acc = 0.0;
    for (int t = p.slot_ptr[a]; t < p.slot_ptr[a + 1]; ++t) {
      const int q = p.slot[t], i = p.slot_piece[q], lo = p.sig_ptr[i], si = p.sig_ptr[i + 1] - lo;
      int l = lo, h = lo + si;   // b in Σ_i ?
      while (l < h) { const int m = (l + h) >> 1; if (p.sig_idx[m] < b) l = m + 1; else h = m; }
      if (l < lo + si && p.sig_idx[l] == b) acc += patch[p.s_off[i] + (q - lo) + (int64_t)(l - lo) * si];
    }
    S[e] = Ass[e] - acc;
  }
}

// s^-1 of a small s, one workgroup in LDS; flag[1] = 1 on a bad pivot
__global__ __launch_bounds__(256) void k_sd_invert(int n, const double *__restrict__ S, double *__restrict__ Z, int *__restrict__ flag) {
  extern __shared__ double sm[];
  const int ld = n + 1;
  double *M = sm, *row = sm + (size_t)n * ld, *col = row + n, *dg = col + n;
  for (int e = threadIdx.x; e < n * n; e += 256) M[e % n + (e / n) * ld] = S[e];
  __syncthreads();
  if (!sd_gj_lds(M, n, ld, row, col, dg) && threadIdx.x == 0) flag[1] = 1;
  for (int e = threadIdx.x; e < n * n; e += 256) Z[e] = M[e % n + (e / n) * ld];
}

// one Gauss-Jordan step k of a large s, src -> dst (ping-pong: no launch reads what it writes); dg = diagonal of s
__global__ __launch_bounds__(256) void k_sd_gj_step(int n, int k, const double *__restrict__ src, double *__restrict__ dst,
                                                    const double *__restrict__ dg, int *__restrict__ flag) {
  const double p = src[k + (int64_t)k * n], ip = 1.0 / p;
  if (blockIdx.x == 0 && threadIdx.x == 0 && !(isfinite(p) && p > (double)n * 2.220446049250313e-16 * dg[k])) flag[1] = 1;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < (int64_t)n * n; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e % n), j = (int)(e / n);
    const double rk = src[k + (int64_t)j * n] * ip;
    double v;
    if (i == k) v = j == k ? ip : rk;
    else v = j == k ? -src[i + (int64_t)k * n] * ip : src[e] - src[i + (int64_t)k * n] * rk;
    dst[e] = v;
  }
}
__global__ __launch_bounds__(256) void k_sd_diag(int n, const double *__restrict__ S, double *__restrict__ dg) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dg[i] = S[i + (int64_t)i * n];
}
// ZT = Z' (row a of s^-1 contiguous for the apply)
__global__ __launch_bounds__(256) void k_sd_transpose(int n, const double *__restrict__ Z, double *__restrict__ ZT) {
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < (int64_t)n * n; e += (int64_t)gridDim.x * 256) {
    const int a = (int)(e % n), b = (int)(e / n);
    ZT[b + (int64_t)a * n] = Z[e];
  }
}

__device__ __forceinline__ double sd_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// apply, launch 1: y_i = D_i^-1 r_i (the columns dealt to the four waves, partials summed in wave order), slot values G_i' r_i
__global__ __launch_bounds__(256) void k_sd_apply1(SdPlanDev p, const double *__restrict__ dinv, const double *__restrict__ G,
                                                   const double *__restrict__ x, double *__restrict__ y, double *__restrict__ slotv,
                                                   const int *done) {
  if (done && *done) return;
  __shared__ double r[spd::P_MAX], part[4][spd::P_MAX];
  const int i = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int p0 = p.piece_ptr[i], ni = p.piece_ptr[i + 1] - p0, q0 = p.sig_ptr[i], si = p.sig_ptr[i + 1] - q0;
  for (int t = tid; t < ni; t += 256) r[t] = x[p.piece_node[p0 + t]];
  __syncthreads();
  const double *Di = dinv + p.d_off[i], *Gi = G + p.b_off[i];
  for (int rr = lane; rr < ni; rr += 64) {
    double acc = 0.0;
    for (int c = w; c < ni; c += 4) acc += Di[rr + c * ni] * r[c];
    part[w][rr] = acc;
  }
  for (int k = w; k < si; k += 4) {
    double acc = 0.0;
    for (int c = lane; c < ni; c += 64) acc += Gi[c + (size_t)k * ni] * r[c];
    acc = sd_wave_sum(acc);
    if (lane == 0) slotv[q0 + k] = acc;
  }
  __syncthreads();
  for (int t = tid; t < ni; t += 256) y[p0 + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

// apply, launch 2: workgroup i < n_pieces: piece i; workgroup n_pieces: the orphan Σ nodes
__global__ __launch_bounds__(256) void k_sd_apply2(SdPlanDev p, const double *__restrict__ G, const double *__restrict__ ZT,
                                                   const double *__restrict__ x, const double *__restrict__ y,
                                                   const double *__restrict__ slotv, double *__restrict__ z, const int *done) {
  if (done && *done) return;
  __shared__ double t[spd::SIGMA_MAX], zs[spd::SIGMA_MAX];
  const int i = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, ns = p.ns;
  for (int a = tid; a < ns; a += 256) {
    double acc = x[p.sigma[a]];
    for (int q = p.slot_ptr[a]; q < p.slot_ptr[a + 1]; ++q) acc -= slotv[p.slot[q]];
    t[a] = acc;
  }
  __syncthreads();
  const bool piece = i < p.n_pieces;
  const int q0 = piece ? p.sig_ptr[i] : 0, cnt = piece ? p.sig_ptr[i + 1] - q0 : p.n_orphan;
  const int *list = piece ? p.sig_idx + q0 : p.orphan;
  for (int k = w; k < cnt; k += 4) {
    const int a = list[k];
    const double *za = ZT + (int64_t)a * ns;
    double acc = 0.0;
    for (int b = lane; b < ns; b += 64) acc += za[b] * t[b];
    acc = sd_wave_sum(acc);
    if (lane == 0) {
      zs[k] = acc;
      if (!piece || p.slot[p.slot_ptr[a]] == q0 + k) z[p.sigma[a]] = acc;   // the first piece next to a writes z_a
    }
  }
  if (!piece) return;
  __syncthreads();
  const int p0 = p.piece_ptr[i], ni = p.piece_ptr[i + 1] - p0;
  const double *Gi = G + p.b_off[i];
  for (int rr = tid; rr < ni; rr += 256) {
    double acc = y[p0 + rr];
    for (int k = 0; k < cnt; ++k) acc -= Gi[rr + (size_t)k * ni] * zs[k];
    z[p.piece_node[p0 + rr]] = acc;
  }
}

struct SpdDirectOp : Operator {
  spd::Plan pl;
  SdPlanDev pd{};
  DevBuf<int> piece_ptr, piece_node, sigma, sig_ptr, sig_idx, slot_ptr, slot, slot_piece, orphan, flag;
  DevBuf<int64_t> d_off, b_off, s_off, dst;
  DevBuf<double> dinv, G, ZT, y, slotv, sink;

  // colptr / rowval / nzval: host arrays of a CSC matrix with `base`-based indices (nzval may be NULL: set_values later)
  SpdDirectOp(mi_ctx_s *c, int64_t n_, const int64_t *colptr, const int64_t *rowval, const double *nzval, int base)
      : Operator(c, n_) {
    if (n_ < 0 || n_ >= INT32_MAX || !colptr || (base != 0 && base != 1)) raise(MI_ERR_BAD_ARG, "mi_spd_direct_create: bad n, colptr or index_base");
    if (colptr[0] != base) raise(MI_ERR_BAD_ARG, "mi_spd_direct_create: colptr[0] != index_base");
    const int64_t nnz = colptr[n_] - base;
    if (nnz < 0 || nnz >= INT32_MAX || (nnz && !rowval)) raise(MI_ERR_BAD_ARG, "mi_spd_direct_create: bad nnz or NULL rowval");
    std::vector<int64_t> cp((size_t)n_ + 1), rv((size_t)nnz);
    for (int64_t k = 0; k <= n_; ++k) cp[k] = colptr[k] - base;
    for (int64_t k = 0; k < nnz; ++k) rv[k] = rowval[k] - base;
    const int P = env_int("MI355_SPD_PIECE", spd::P_DEFAULT);
    std::string err;
    const int st = spd::make_plan((int)n_, cp.data(), rv.data(), P, spd::SIGMA_MAX, pl, err);
    if (st != spd::OK) raise(MI_ERR_BAD_ARG, "mi_spd_direct_create: %s", err.c_str());
    hipStream_t s = c->stream;
    auto up = [&](DevBuf<int> &d, const std::vector<int> &h) { d.upload(h.empty() ? std::vector<int>{0} : h, s); };
    auto up64 = [&](DevBuf<int64_t> &d, const std::vector<int64_t> &h) { d.upload(h.empty() ? std::vector<int64_t>{0} : h, s); };
    up(piece_ptr, pl.piece_ptr); up(piece_node, pl.piece_node); up(sigma, pl.sigma); up(sig_ptr, pl.sig_ptr);
    up(sig_idx, pl.sig_idx); up(slot_ptr, pl.slot_ptr); up(slot, pl.slot); up(slot_piece, pl.slot_piece); up(orphan, pl.orphan);
    up64(d_off, pl.d_off); up64(b_off, pl.b_off); up64(s_off, pl.s_off); up64(dst, pl.dst);
    if (pl.slot_ptr.empty()) up(slot_ptr, std::vector<int>{0});
    pd = SdPlanDev{pl.n_pieces(), pl.n_sigma(), (int)pl.orphan.size(), piece_ptr.p, piece_node.p, sigma.p, sig_ptr.p, sig_idx.p,
                   slot_ptr.p, slot.p, slot_piece.p, orphan.p, d_off.p, b_off.p, s_off.p};
    const int ns = pl.n_sigma();
    dinv.alloc((size_t)pl.d_total); G.alloc((size_t)pl.b_total); ZT.alloc((size_t)ns * ns);
    y.alloc((size_t)pl.piece_ptr.back()); slotv.alloc((size_t)pl.sig_idx.size()); sink.alloc((size_t)n + 1);
    flag.alloc(2);
    // The attribute belongs to the function, not to this operator, and the last value set holds: with it set to this
    // operator's own need, the set_values of another live operator that needs more would launch above it. Both kernels
    // are therefore always allowed the most any operator can ask for (P or |Σ| = P_MAX: 132 KiB of the 160 KiB).
    const int lds = (int)sd_lds_bytes(spd::P_MAX);
    MI_HIP(hipFuncSetAttribute((const void *)k_sd_factor, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    MI_HIP(hipFuncSetAttribute((const void *)k_sd_invert, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (nzval) {
      DevBuf<double> v;
      v.upload(nzval, (size_t)nnz, s);
      factor(v.p);
    }
    MI_HIP(hipStreamSynchronize(s));
  }
  int64_t nnz() const { return pl.nnz; }

  // The numeric phase on device values `val` (nnz, the CSC order of create). Synchronous; raises MI_ERR_SINGULAR and keeps
  // the previous factor when a pivot or the certificate of s^-1 fails.
  void factor(const double *val) {
    hipStream_t s = ctx->stream;
    const int np = pl.n_pieces(), ns = pl.n_sigma();
    auto cdiv = [](int64_t a, int64_t b) { return (int)std::max<int64_t>(1, std::min<int64_t>((a + b - 1) / b, 4096)); };
    DevBuf<double> work((size_t)pl.work_total()), patch((size_t)pl.patch_total), cd((size_t)pl.d_total), cg((size_t)pl.b_total);
    DevBuf<double> S((size_t)ns * ns), Z0((size_t)ns * ns), Z1((size_t)ns * ns), dg((size_t)ns + 1), probe((size_t)ns + 1), norms(24);
    MI_HIP(hipMemsetAsync(work.p, 0, sizeof(double) * work.n, s));
    MI_HIP(hipMemsetAsync(flag.p, 0, 2 * sizeof(int), s));
    if (pl.nnz) hipLaunchKernelGGL(k_sd_scatter, dim3(cdiv(pl.nnz, 256)), dim3(256), 0, s, (int64_t)pl.nnz, dst.p, val, work.p);
    if (np) hipLaunchKernelGGL(k_sd_factor, dim3(np), dim3(256), sd_lds_bytes(pl.P), s, pd, (int64_t)pl.d_total,
                               (const double *)work.p, cd.p, cg.p, patch.p, flag.p);
    const double *Z = Z0.p;
    if (ns) {
      hipLaunchKernelGGL(k_sd_schur, dim3(cdiv((int64_t)ns * ns, 256)), dim3(256), 0, s, pd,
                         (const double *)work.p + pl.d_total + pl.b_total, (const double *)patch.p, S.p);
      if (ns <= spd::P_MAX) {
        hipLaunchKernelGGL(k_sd_invert, dim3(1), dim3(256), sd_lds_bytes(ns), s, ns, (const double *)S.p, Z0.p, flag.p);
      } else {
        hipLaunchKernelGGL(k_sd_diag, dim3(cdiv(ns, 256)), dim3(256), 0, s, ns, (const double *)S.p, dg.p);
        const double *src = S.p;
        for (int k = 0; k < ns; ++k) {
          double *d = (k & 1) ? Z1.p : Z0.p;
          hipLaunchKernelGGL(k_sd_gj_step, dim3(cdiv((int64_t)ns * ns, 256)), dim3(256), 0, s, ns, k, src, d, (const double *)dg.p, flag.p);
          src = d;
        }
        Z = src;
      }
      // certificate (mi_nn_pinv's probe): t = s v, residual max |v - Z t|, ||s||_inf, ||Z||_inf
      hipLaunchKernelGGL(k_probe_apply, dim3(8), dim3(256), 0, s, ns, (const double *)S.p, 0.0, probe.p);
      hipLaunchKernelGGL(k_probe_residual, dim3(8), dim3(256), 0, s, ns, Z, (const double *)probe.p, norms.p);
      hipLaunchKernelGGL(k_rowsum_max_t<false>, dim3(8), dim3(256), 0, s, ns, (const double *)S.p, norms.p + 8);
      hipLaunchKernelGGL(k_rowsum_max_t<false>, dim3(8), dim3(256), 0, s, ns, Z, norms.p + 16);
    }
    MI_HIP(hipGetLastError());
    int fh[2] = {0, 0};
    double nh[24] = {0};
    MI_HIP(hipMemcpyAsync(fh, flag.p, sizeof fh, hipMemcpyDeviceToHost, s));
    if (ns) MI_HIP(hipMemcpyAsync(nh, norms.p, sizeof nh, hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (fh[0]) raise(MI_ERR_SINGULAR, "mi_spd_direct: a diagonal block of a piece is singular or not positive definite");
    if (fh[1]) raise(MI_ERR_SINGULAR, "mi_spd_direct: the separator's Schur complement (%d x %d) is singular or not positive definite", ns, ns);
    if (ns) {
      double res = 0, nS = 0, nZ = 0;
      for (int k = 0; k < 8; ++k) { res = std::max(res, nh[k]); nS = std::max(nS, nh[8 + k]); nZ = std::max(nZ, nh[16 + k]); }
      const double bar = 4.0 * ns * std::numeric_limits<double>::epsilon() * nS * nZ;
      if (!std::isfinite(res) || !std::isfinite(nZ) || res > bar)
        raise(MI_ERR_SINGULAR, "mi_spd_direct: s^-1 fails its certificate (probe residual %.3e > %.3e)", res, bar);
    }
    // accepted: into the live factor (same addresses, so captured solve graphs stay valid)
    if (pl.d_total) MI_HIP(hipMemcpyAsync(dinv.p, cd.p, sizeof(double) * pl.d_total, hipMemcpyDeviceToDevice, s));
    if (pl.b_total) MI_HIP(hipMemcpyAsync(G.p, cg.p, sizeof(double) * pl.b_total, hipMemcpyDeviceToDevice, s));
    if (ns) hipLaunchKernelGGL(k_sd_transpose, dim3(cdiv((int64_t)ns * ns, 256)), dim3(256), 0, s, ns, Z, ZT.p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));   // the work buffers go out of scope
    factored = true;
  }
  bool factored = false;

  void launch1(const double *x, double *yy, double *sv, const int *done) {
    if (pl.n_pieces())
      hipLaunchKernelGGL(k_sd_apply1, dim3(pl.n_pieces()), dim3(256), 0, ctx->stream, pd, (const double *)dinv.p,
                         (const double *)G.p, x, yy, sv, done);
  }
  void apply(const double *x, double *z, const int *done) override {
    if (!factored) raise(MI_ERR_BAD_ARG, "mi_spd_direct: no values yet (mi_spd_direct_set_values)");
    if (n == 0) return;
    launch1(x, y.p, slotv.p, done);
    const int grid = pl.n_pieces() + (pl.orphan.empty() ? 0 : 1);
    hipLaunchKernelGGL(k_sd_apply2, dim3(grid), dim3(256), 0, ctx->stream, pd, (const double *)G.p, (const double *)ZT.p, x,
                       (const double *)y.p, (const double *)slotv.p, z, done);
    MI_HIP(hipGetLastError());
  }
  // bytes that the two launches move: the factor (D_i^-1; G_i twice; the rows of s^-1 that each workgroup reads) and the vectors
  void bytes(int64_t *a, int64_t *d) const override {
    const int64_t ns = pl.n_sigma(), nP = pl.piece_ptr.back(), nslot = (int64_t)pl.sig_idx.size();
    const int64_t rows = nslot + (int64_t)pl.orphan.size();
    *d = 8 * (pl.d_total + pl.b_total + 2 * nP + nslot) + 4 * nP;
    *a = *d + 8 * (pl.b_total + rows * ns + nP + ns + n + nslot) + 4 * (nP + ns);
  }
  void apply_dominant(const double *x) override { launch1(x, y.p, slotv.p, nullptr); }
};

}  // namespace mi
