// Numeric phase of the smoothed-aggregation hierarchy on the device, on the frozen patterns of amg_plan.hpp: what
// fem.prepare_amg_precond redoes on the host for every realization (2.2 s at 1 M unknowns), as launches on the context's
// stream (mi_amg_plan_create / mi_amg_set_values). The cycle is amg.hpp's, unchanged.
//
// Per smoothed level l, in this order, no atomics, every sum in a fixed order — two refreshes give the same bits:
//   k_as_gersh    ratio_i = (Σ_j |a_ij|, CSR order) / a_ii; the maximum over a workgroup's rows (order-free)
//   k_as_omega    g = max of the workgroup maxima; ω = 4 / (3 g), left on the device
//   k_as_prolong  one thread per row: wd_i = ω / a_ii;  P[k] = T[k] - wd_i (Σ_{s in segment k} A[src[s]] tw[J]), the segment in
//                 ascending column of A_l (the order of scipy's A @ T)
//   k_as_gather   R = P' by the plan's permutation
//   k_as_product  AP = A_l P_l, then M = R_l (AP): one thread per entry (i, J) of the structural output pattern, the row of
//                 the left factor walked in ascending inner index j, J located in row j of the right factor by binary search
//                 (a structural miss adds nothing). Any row length is one loop: the R row of a giant aggregate (more than
//                 SPMV_TILE entries) takes the same path as every other.
//   k_as_sym      A_{l+1}[k] = (M[k] + M[sym[k]]) / 2: exactly symmetric
// A diagonal entry that is missing or not positive sets flag[0], a row whose sum is not finite flag[1] (plain stores of 1).
// Coarsest level: scattered into a dense block, symmetrised, inverted by the SPD route of mi_nn_pinv (Gauss-Jordan with the
// probe certificate, pinv_blocks_fast(spd_only)), the inverse symmetrised as prepare_amg_precond does.
// Everything is computed into candidate buffers; only a phase that succeeds is committed, by device copies into the buffers
// the cycle reads — their addresses never change, so captured solve graphs stay valid and see the new values.
#pragma once
#include "amg.hpp"
#include "amg_plan.hpp"
#include "setup_gj.hpp"

namespace mi {

constexpr int AS_NT = 256;

__global__ __launch_bounds__(AS_NT) void k_as_gersh(int n, const int *__restrict__ ptr, const double *__restrict__ val, const int *__restrict__ diag,
                                                    double *__restrict__ part, int *flag) {
  __shared__ double sm[AS_NT / 64];
  const int i = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  double ratio = 0.0;
  if (i < n) {
    double sum = 0.0;
    for (int k = ptr[i]; k < ptr[i + 1]; ++k) sum += fabs(val[k]);
    const int dk = diag[i];
    const double d = dk >= 0 ? val[dk] : 0.0;
    if (!(d > 0.0)) flag[0] = 1;
    if (!isfinite(sum)) flag[1] = 1;
    ratio = sum / d;
  }
  for (int o = 32; o > 0; o >>= 1) ratio = fmax(ratio, __shfl_down(ratio, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = ratio;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}
// one workgroup: g = max(part[0 .. m)), out[0] = ω = 4 / (3 g), out[1] = g
__global__ __launch_bounds__(AS_NT) void k_as_omega(int m, const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double sm[AS_NT / 64];
  double g = 0.0;
  for (int k = threadIdx.x; k < m; k += AS_NT) g = fmax(g, part[k]);
  for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_down(g, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = g;
  __syncthreads();
  if (threadIdx.x == 0) {
    g = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
    out[0] = 4.0 / (3.0 * g);
    out[1] = g;
  }
}
__global__ __launch_bounds__(AS_NT) void k_as_prolong(int n, const double *__restrict__ a_val, const int *__restrict__ diag, const int *__restrict__ agg,
                                                      const double *__restrict__ tw, const int *__restrict__ p_ptr, const int *__restrict__ p_col,
                                                      const int *__restrict__ seg_ptr, const int *__restrict__ seg_src, const double *__restrict__ omega,
                                                      double *__restrict__ wd, double *__restrict__ p_val) {
  const int i = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (i >= n) return;
  const int dk = diag[i];
  const double w = omega[0] / (dk >= 0 ? a_val[dk] : 0.0);
  wd[i] = w;
  const int own = agg[i];
  for (int k = p_ptr[i]; k < p_ptr[i + 1]; ++k) {
    const int J = p_col[k];
    const double t = tw[J];
    double s = 0.0;
    for (int q = seg_ptr[k]; q < seg_ptr[k + 1]; ++q) s += a_val[seg_src[q]] * t;
    p_val[k] = (J == own ? t : 0.0) - w * s;
  }
}
__global__ __launch_bounds__(AS_NT) void k_as_gather(int m, const int *__restrict__ from, const double *__restrict__ src, double *__restrict__ dst) {
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k < m) dst[k] = src[from[k]];
}
// the row of entry k: the last i with ptr[i] <= k (rows without entries are passed over)
__device__ __forceinline__ int as_row_of(const int *__restrict__ ptr, int n, int k) {
  int lo = 0, hi = n;   // invariant: ptr[lo] <= k < ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(AS_NT) void k_as_product(int n, int nnz_c, const int *__restrict__ c_ptr, const int *__restrict__ c_col,
                                                      const int *__restrict__ a_ptr, const int *__restrict__ a_col, const double *__restrict__ a_val,
                                                      const int *__restrict__ b_ptr, const int *__restrict__ b_col, const double *__restrict__ b_val,
                                                      double *__restrict__ c_val) {
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k >= nnz_c) return;
  const int i = as_row_of(c_ptr, n, k), J = c_col[k];
  double s = 0.0;
  for (int q = a_ptr[i]; q < a_ptr[i + 1]; ++q) {
    const int j = a_col[q];
    int lo = b_ptr[j], hi = b_ptr[j + 1];
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (b_col[mid] < J) lo = mid + 1; else hi = mid;
    }
    if (lo < b_ptr[j + 1] && b_col[lo] == J) s += a_val[q] * b_val[lo];
  }
  c_val[k] = s;
}
__global__ __launch_bounds__(AS_NT) void k_as_sym(int m, const int *__restrict__ sym, const double *__restrict__ src, double *__restrict__ dst) {
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k < m) dst[k] = (src[k] + src[sym[k]]) * 0.5;
}
// D (n x n, zeroed before) gets the stored entries
__global__ __launch_bounds__(AS_NT) void k_as_dense(int n, int nnz, const int *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                    double *__restrict__ D) {
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k >= nnz) return;
  const int i = as_row_of(ptr, n, k);
  D[(size_t)i + (size_t)col[k] * n] = val[k];
}
__global__ __launch_bounds__(AS_NT) void k_as_sym_dense(int n, const double *__restrict__ src, double *__restrict__ dst) {
  const long long e = (long long)blockIdx.x * AS_NT + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int i = (int)(e % n), j = (int)(e / n);
  dst[e] = (src[e] + src[(size_t)j + (size_t)i * n]) * 0.5;
}

struct AmgPlanOp : AmgOp {
  struct Dev {   // the plan of one level on the device; patterns of A, P, R are those of the CsrDev of the cycle
    DevBuf<int> diag, sym, agg, seg_ptr, seg_src, r_from, ap_ptr, ap_col;
    DevBuf<double> tw;
    DevBuf<double> cA, cP, cR, cwd;   // candidates (cA: levels >= 1; level 0 reads the caller's values)
    int64_t ap_nnz = 0;
  };
  amgp::Plan plan;
  std::vector<Dev> dv;
  DevBuf<double> w_ap, w_m;             // A_l P_l and the unsymmetrised Galerkin product, shared by the levels
  DevBuf<double> part, om_c, om;        // workgroup maxima; (ω, g) per smoothed level: candidate and committed
  DevBuf<double> dense, dense_s, z_raw, z_c;
  DevBuf<int> flag;
  DevBuf<double> stage;                 // host-pointer set_values
  int64_t nnz0 = 0, extra = 0;          // stored entries of A_0; bytes of the plan and of the second buffers
  bool ready = false;
  // mi_amg_refresh_profile: events between the kernel groups of one refresh (phase of the interval that ends there, event)
  enum { PH_GERSH = 0, PH_PROLONG, PH_AP, PH_RAP, PH_COARSE, PH_COMMIT, PH_COUNT };
  std::vector<std::pair<int, hipEvent_t>> *trace = nullptr;
  void mark(int phase) {
    if (!trace) return;
    hipEvent_t e;
    MI_HIP(hipEventCreate(&e));
    trace->emplace_back(phase, e);
    MI_HIP(hipEventRecord(e, ctx->stream));
  }

  static int grid(int64_t m) { return (int)((std::max<int64_t>(m, 1) + AS_NT - 1) / AS_NT); }

  AmgPlanOp(mi_ctx_s *c, int64_t n0, const int64_t *rowptr, const int64_t *colidx, const double *val, int64_t nlevels, const int64_t *n_l,
            const int64_t *const *agg, int base, const std::vector<int> *breaks0 = nullptr)
      : AmgOp(c, n0) {   // breaks0 (interior_amg.hpp): rows the row blocks of A_0 do not cross; val == NULL (amg_bank.hpp): the
                         // plan, the patterns and the work only — a set-up engine that is never applied
    std::string err;
    if (n0 < 1 || n0 >= INT32_MAX) raise(MI_ERR_BAD_ARG, "mi_amg_plan_create: n = %lld rows", (long long)n0);
    if (amgp::make_plan(n0, rowptr, colidx, nlevels, n_l, agg, base, c->rank, c->n_ranks, plan, err) != amgp::OK) raise(MI_ERR_BAD_ARG, "%s", err.c_str());
    hipStream_t s = c->stream;
    nlev = plan.nlev; nc = plan.lv.back().n;
    nnz0 = plan.lv[0].a_nnz();
    lv.resize((size_t)nlev);
    dv.resize((size_t)nlev);
    int64_t w1 = 1, w2 = 1, second = 0;
    size_t nmax = 1;
    auto pattern = [](int nr, int ncol, const std::vector<int> &ptr, const std::vector<int> &col) {
      HostCsr h;
      h.n_rows = nr; h.n_cols = ncol; h.rowptr = ptr; h.col = col; h.val.assign(col.size(), 0.0);
      return h;
    };
    auto up = [&](DevBuf<int> &dst, const std::vector<int> &h) { dst.upload(h.empty() ? std::vector<int>{0} : h, s); };
    for (int l = 0; l < nlev; ++l) {
      const amgp::Level &H = plan.lv[(size_t)l];
      Level &L = lv[(size_t)l];
      Dev &D = dv[(size_t)l];
      L.n = H.n;
      nmax = std::max(nmax, (size_t)H.n);
      op_nnz += H.a_nnz();
      L.A.upload(pattern(H.n, H.n, H.a_ptr, H.a_col), s, l == 0 ? breaks0 : nullptr);
      up(D.diag, H.diag); up(D.sym, H.sym);
      if (l) { D.cA.alloc((size_t)H.a_nnz() + 1); second += 8 * H.a_nnz(); }
      if (l == nlev - 1) break;
      L.P.upload(pattern(H.n, H.nc, H.p_ptr, H.p_col), s);
      L.R.upload(pattern(H.nc, H.n, H.r_ptr, H.r_col), s);
      L.wd.alloc((size_t)H.n + 1);
      up(D.agg, H.agg); up(D.seg_ptr, H.seg_ptr); up(D.seg_src, H.seg_src); up(D.r_from, H.r_from); up(D.ap_ptr, H.ap_ptr); up(D.ap_col, H.ap_col);
      D.tw.upload(H.tw, s);
      D.ap_nnz = H.ap_nnz();
      D.cP.alloc((size_t)H.p_nnz() + 1); D.cR.alloc((size_t)H.p_nnz() + 1); D.cwd.alloc((size_t)H.n + 1);
      second += 16 * H.p_nnz() + 8 * (int64_t)H.n;
      w1 = std::max(w1, H.ap_nnz()); w2 = std::max(w2, plan.lv[(size_t)l + 1].a_nnz());
      // the cycle's byte counts: as in mi_amg_create
      kept += 12 * H.a_nnz() + 24 * H.p_nnz() + 8 * (int64_t)H.n;
      alg += 2 * (12 * H.a_nnz() + 4 * ((int64_t)H.n + 1)) + 24 * H.p_nnz() + 4 * ((int64_t)H.n + 1) + 4 * ((int64_t)H.nc + 1) + 88 * (int64_t)H.n +
             16 * (int64_t)H.nc;
      if (l == 0) dom = 12 * H.a_nnz() + 4 * ((int64_t)H.n + 1) + 32 * (int64_t)H.n;
    }
    kept += 8 * (int64_t)nc * nc;
    alg += 8 * (int64_t)nc * nc + 16 * (int64_t)nc;
    if (nlev == 1) dom = alg;
    w_ap.alloc((size_t)w1 + 1); w_m.alloc((size_t)w2 + 1);
    part.alloc((size_t)grid((int64_t)nmax) + 1);
    om_c.alloc((size_t)2 * nlev + 2); om.alloc((size_t)2 * nlev + 2);
    const size_t nn = (size_t)nc * nc;
    zinv.alloc(nn + 1); dense.alloc(nn + 1); dense_s.alloc(nn + 1); z_raw.alloc(nn + 1); z_c.alloc(nn + 1);
    flag.alloc(2);
    second += 8 * (w1 + w2) + 8 * 4 * (int64_t)nn + 12 * plan.lv.back().a_nnz();   // (the coarsest A_L is kept for the read-back: values and columns)
    extra = plan.bytes() + second;
    kept += extra;
    omega_h.assign((size_t)std::max(0, nlev - 1), 0.0);
    if (!val) return;
    alloc_vectors();
    DevBuf<double> v;
    v.upload(val, (size_t)nnz0, s);
    refresh(v.p, "mi_amg_plan_create");
    MI_HIP(hipStreamSynchronize(s));
  }

  // The numeric phase on the device values `a0` (the CSR order of create). Synchronous. Raises MI_ERR_SINGULAR and leaves
  // every committed buffer as it was.
  void refresh(const double *a0, const char *me) {
    hipStream_t s = ctx->stream;
    MI_HIP(hipMemsetAsync(flag.p, 0, 2 * sizeof(int), s));
    mark(-1);
    for (int l = 0; l + 1 < nlev; ++l) {
      const amgp::Level &H = plan.lv[(size_t)l], &HN = plan.lv[(size_t)l + 1];
      Level &L = lv[(size_t)l], &N = lv[(size_t)l + 1];
      Dev &D = dv[(size_t)l], &DN = dv[(size_t)l + 1];
      const double *a = l ? D.cA.p : a0;
      const int n = H.n, nb = grid(n);
      const int pn = (int)H.p_nnz(), apn = (int)H.ap_nnz(), cn = (int)HN.a_nnz();
      double *om_l = om_c.p + 2 * l;
      hipLaunchKernelGGL(k_as_gersh, dim3(nb), dim3(AS_NT), 0, s, n, (const int *)L.A.rowptr.p, a, (const int *)D.diag.p, part.p, flag.p);
      hipLaunchKernelGGL(k_as_omega, dim3(1), dim3(AS_NT), 0, s, nb, (const double *)part.p, om_l);
      mark(PH_GERSH);
      hipLaunchKernelGGL(k_as_prolong, dim3(nb), dim3(AS_NT), 0, s, n, a, (const int *)D.diag.p, (const int *)D.agg.p, (const double *)D.tw.p,
                         (const int *)L.P.rowptr.p, (const int *)L.P.col.p, (const int *)D.seg_ptr.p, (const int *)D.seg_src.p, (const double *)om_l, D.cwd.p,
                         D.cP.p);
      hipLaunchKernelGGL(k_as_gather, dim3(grid(pn)), dim3(AS_NT), 0, s, pn, (const int *)D.r_from.p, (const double *)D.cP.p, D.cR.p);
      mark(PH_PROLONG);
      hipLaunchKernelGGL(k_as_product, dim3(grid(apn)), dim3(AS_NT), 0, s, n, apn, (const int *)D.ap_ptr.p, (const int *)D.ap_col.p,
                         (const int *)L.A.rowptr.p, (const int *)L.A.col.p, a, (const int *)L.P.rowptr.p, (const int *)L.P.col.p, (const double *)D.cP.p,
                         w_ap.p);
      mark(PH_AP);
      hipLaunchKernelGGL(k_as_product, dim3(grid(cn)), dim3(AS_NT), 0, s, HN.n, cn, (const int *)N.A.rowptr.p, (const int *)N.A.col.p,
                         (const int *)L.R.rowptr.p, (const int *)L.R.col.p, (const double *)D.cR.p, (const int *)D.ap_ptr.p, (const int *)D.ap_col.p,
                         (const double *)w_ap.p, w_m.p);
      hipLaunchKernelGGL(k_as_sym, dim3(grid(cn)), dim3(AS_NT), 0, s, cn, (const int *)DN.sym.p, (const double *)w_m.p, DN.cA.p);
      mark(PH_RAP);
    }
    MI_HIP(hipGetLastError());
    const amgp::Level &HC = plan.lv[(size_t)nlev - 1];
    Level &C = lv[(size_t)nlev - 1];
    Dev &DC = dv[(size_t)nlev - 1];
    const double *ac = nlev > 1 ? DC.cA.p : a0;
    const int cn = (int)HC.a_nnz();
    const size_t nn = (size_t)nc * nc;
    // the diagonal and the values of the coarsest level are tested like those of the others
    hipLaunchKernelGGL(k_as_gersh, dim3(grid(nc)), dim3(AS_NT), 0, s, nc, (const int *)C.A.rowptr.p, ac, (const int *)DC.diag.p, part.p, flag.p);
    MI_HIP(hipMemsetAsync(dense.p, 0, nn * sizeof(double), s));
    hipLaunchKernelGGL(k_as_dense, dim3(grid(cn)), dim3(AS_NT), 0, s, nc, cn, (const int *)C.A.rowptr.p, (const int *)C.A.col.p, ac, dense.p);
    hipLaunchKernelGGL(k_as_sym_dense, dim3(grid((int64_t)nn)), dim3(AS_NT), 0, s, nc, (const double *)dense.p, dense_s.p);
    MI_HIP(hipGetLastError());
    int fh[2] = {0, 0};
    MI_HIP(hipMemcpyAsync(fh, flag.p, sizeof fh, hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (fh[1]) raise(MI_ERR_SINGULAR, "%s: a value of the matrix, or of a level built from it, is not finite; the previous hierarchy is kept", me);
    if (fh[0]) raise(MI_ERR_SINGULAR, "%s: a diagonal entry of a level is missing or not positive (the matrix is not positive definite); the previous hierarchy is kept", me);
    const int64_t nc64 = nc;
    try {
      pinv_blocks_fast(ctx, 1, &nc64, dense_s.p, 0.0, z_raw.p, true);
    } catch (const Error &e) {
      if (e.code != MI_ERR_SINGULAR) throw;
      const std::string why = last_error();
      raise(MI_ERR_SINGULAR, "%s: the coarsest level (%d rows): %s; the previous hierarchy is kept", me, nc, why.c_str());
    }
    hipLaunchKernelGGL(k_as_sym_dense, dim3(grid((int64_t)nn)), dim3(AS_NT), 0, s, nc, (const double *)z_raw.p, z_c.p);
    MI_HIP(hipGetLastError());
    mark(PH_COARSE);
    // accepted: into the buffers the cycle reads (same addresses: captured solve graphs stay valid)
    auto copy = [&](double *dst, const double *src, size_t cnt) {
      if (cnt && dst != src) MI_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
    };
    for (int l = 0; l < nlev; ++l) {
      const amgp::Level &H = plan.lv[(size_t)l];
      Level &L = lv[(size_t)l];
      Dev &D = dv[(size_t)l];
      copy(L.A.val.p, l ? D.cA.p : a0, (size_t)H.a_nnz());
      if (l == nlev - 1) break;
      copy(L.P.val.p, D.cP.p, (size_t)H.p_nnz()); copy(L.R.val.p, D.cR.p, (size_t)H.p_nnz()); copy(L.wd.p, D.cwd.p, (size_t)H.n);
    }
    copy(om.p, om_c.p, (size_t)2 * (nlev - 1));
    copy(zinv.p, z_c.p, nn);
    std::vector<double> oh((size_t)2 * std::max(1, nlev - 1));
    if (nlev > 1) MI_HIP(hipMemcpyAsync(oh.data(), om_c.p, sizeof(double) * 2 * (size_t)(nlev - 1), hipMemcpyDeviceToHost, s));
    mark(PH_COMMIT);
    MI_HIP(hipStreamSynchronize(s));
    for (int l = 0; l + 1 < nlev; ++l) omega_h[(size_t)l] = oh[(size_t)2 * l];
    ready = true;
  }

  // One refresh on the committed values of A_0, timed by events: ms[PH_COUNT] = Gershgorin + ω, prolongator + R, A P,
  // R (A P) + symmetrisation, coarsest level (scatter, inverse with its certificate and host synchronisations), commit copies.
  void profile(double *ms) {
    std::vector<std::pair<int, hipEvent_t>> ev;
    trace = &ev;
    try {
      refresh(lv[0].A.val.p, "mi_amg_refresh_profile");
    } catch (...) {
      trace = nullptr;
      for (auto &e : ev) (void)hipEventDestroy(e.second);
      throw;
    }
    trace = nullptr;
    for (int k = 0; k < PH_COUNT; ++k) ms[k] = 0.0;
    for (size_t k = 1; k < ev.size(); ++k) {
      float t = 0.f;
      MI_HIP(hipEventElapsedTime(&t, ev[k - 1].second, ev[k].second));
      ms[ev[k].first] += t;
    }
    for (auto &e : ev) (void)hipEventDestroy(e.second);
  }
};

}  // namespace mi
