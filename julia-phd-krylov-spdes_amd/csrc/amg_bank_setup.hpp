// The numeric set-up of amg_setup.hpp for k <= AMGB_MAX_TERMS members of a bank at once (mi_amg_bank_set_values_batch): the
// hierarchies of the loop `Π_amg_t = AMGPreconditioner{SmoothedAggregation}(A_t)` (Example06:167-182) for k realizations whose
// matrices lie in k slots of a CsrBatch, in ONE sequence of launches. Term t is blockIdx.y; the x-geometry (AS_NT, grid(m)),
// the arithmetic and the order of every sum are those of k_as_*: a member built here carries the bits of
// mi_amg_bank_set_values on the same values.
//
// Every kernel reads a small device array
//   sel[0] = k, sel[1 + t] = member of term t, sel[1 + 16 + t] = slot of term t, sel[33] = k', sel[34 + j] = the term of block j
// and forms its pointers as base + index * stride: the values of A_0 are read in place at slab_A + slot_t * stride_A, everything
// a term computes lies at index t of a workspace of its own:
//   cand   k candidate slots in the layout of a bank slot without its A_0:  A_1 .. | P | R | ω/d | coarse inverse | (ω, g)
//   w_ap, w_m, part, flag pair, dense, dense_s: one of each per term;  z_raw: the inverses of the k' healthy blocks, packed
// A term whose flag is raised goes on computing on its own candidates (all indices are the plan's, none depends on a
// value) and is not committed. Commit of a healthy term: A_0 from its batch slot, then ONE copy of the candidate slot.
#pragma once
#include "amg_setup.hpp"

namespace mi {

constexpr int ASB_MAX = 16;                  // = AMGB_MAX_TERMS = BATCH_MAX
constexpr int ASB_SLOT = 1 + ASB_MAX;        // sel[ASB_SLOT + t]: the batch slot of term t
constexpr int ASB_NZ = 1 + 2 * ASB_MAX;      // sel[ASB_NZ]: k', the blocks that were inverted
constexpr int ASB_ZTERM = ASB_NZ + 1;        // sel[ASB_ZTERM + j]: the term of packed block j
constexpr int ASB_SEL = ASB_ZTERM + ASB_MAX;

// `by_slot`: the array is A_0 in the batch's slab (indexed by the term's slot); otherwise it is the term's own
#define MI_ASB_TERM                    \
  const int t = (int)blockIdx.y;       \
  if (t >= sel[0]) return
__device__ __forceinline__ size_t asb_at(const int *__restrict__ sel, int t, int by_slot) { return (size_t)(by_slot ? sel[ASB_SLOT + t] : t); }

__global__ __launch_bounds__(AS_NT) void k_asb_gersh(int n, const int *__restrict__ ptr, const double *__restrict__ a0, long long as, int by_slot,
                                                     const int *__restrict__ diag, double *__restrict__ part0, long long ps, int *flag0,
                                                     const int *__restrict__ sel) {
  MI_ASB_TERM;
  const double *val = a0 + asb_at(sel, t, by_slot) * (size_t)as;
  double *part = part0 + (size_t)t * (size_t)ps;
  int *flag = flag0 + 2 * t;
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
// one workgroup per term: out[0] = ω = 4 / (3 g), out[1] = g
__global__ __launch_bounds__(AS_NT) void k_asb_omega(int m, const double *__restrict__ part0, long long ps, double *__restrict__ out0, long long os,
                                                     const int *__restrict__ sel) {
  MI_ASB_TERM;
  const double *part = part0 + (size_t)t * (size_t)ps;
  double *out = out0 + (size_t)t * (size_t)os;
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
// cand0 / cs: the candidate slots; off_om, off_wd, off_p: doubles from the start of a candidate slot
__global__ __launch_bounds__(AS_NT) void k_asb_prolong(int n, const double *__restrict__ a0, long long as, int by_slot, const int *__restrict__ diag,
                                                       const int *__restrict__ agg, const double *__restrict__ tw, const int *__restrict__ p_ptr,
                                                       const int *__restrict__ p_col, const int *__restrict__ seg_ptr, const int *__restrict__ seg_src,
                                                       double *cand0, long long cs, long long off_om, long long off_wd, long long off_p,
                                                       const int *__restrict__ sel) {
  MI_ASB_TERM;
  const double *a_val = a0 + asb_at(sel, t, by_slot) * (size_t)as;
  double *cand = cand0 + (size_t)t * (size_t)cs;
  const double *omega = cand + off_om;
  double *wd = cand + off_wd, *p_val = cand + off_p;
  const int i = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (i >= n) return;
  const int dk = diag[i];
  const double w = omega[0] / (dk >= 0 ? a_val[dk] : 0.0);
  wd[i] = w;
  const int own = agg[i];
  for (int k = p_ptr[i]; k < p_ptr[i + 1]; ++k) {
    const int J = p_col[k];
    const double tj = tw[J];
    double s = 0.0;
    for (int q = seg_ptr[k]; q < seg_ptr[k + 1]; ++q) s += a_val[seg_src[q]] * tj;
    p_val[k] = (J == own ? tj : 0.0) - w * s;
  }
}
__global__ __launch_bounds__(AS_NT) void k_asb_gather(int m, const int *__restrict__ from, double *cand0, long long cs, long long off_src,
                                                      long long off_dst, const int *__restrict__ sel) {
  MI_ASB_TERM;
  double *cand = cand0 + (size_t)t * (size_t)cs;
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k < m) cand[off_dst + k] = cand[off_src + from[k]];
}
// C = A B on the structural pattern of C; A's values may be A_0 in the batch's slab, B's and C's are the term's own
__global__ __launch_bounds__(AS_NT) void k_asb_product(int n, int nnz_c, const int *__restrict__ c_ptr, const int *__restrict__ c_col,
                                                       const int *__restrict__ a_ptr, const int *__restrict__ a_col, const double *__restrict__ a0,
                                                       long long as, int by_slot, const int *__restrict__ b_ptr, const int *__restrict__ b_col,
                                                       const double *__restrict__ b0, long long bs, double *__restrict__ c0, long long cstr,
                                                       const int *__restrict__ sel) {
  MI_ASB_TERM;
  const double *a_val = a0 + asb_at(sel, t, by_slot) * (size_t)as, *b_val = b0 + (size_t)t * (size_t)bs;
  double *c_val = c0 + (size_t)t * (size_t)cstr;
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
__global__ __launch_bounds__(AS_NT) void k_asb_sym(int m, const int *__restrict__ sym, const double *__restrict__ src0, long long ss,
                                                   double *__restrict__ dst0, long long ds, const int *__restrict__ sel) {
  MI_ASB_TERM;
  const double *src = src0 + (size_t)t * (size_t)ss;
  double *dst = dst0 + (size_t)t * (size_t)ds;
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k < m) dst[k] = (src[k] + src[sym[k]]) * 0.5;
}
// D_t (n x n, zeroed before) gets the stored entries
__global__ __launch_bounds__(AS_NT) void k_asb_dense(int n, int nnz, const int *__restrict__ ptr, const int *__restrict__ col,
                                                     const double *__restrict__ a0, long long as, int by_slot, double *__restrict__ D0, long long ds,
                                                     const int *__restrict__ sel) {
  MI_ASB_TERM;
  const double *val = a0 + asb_at(sel, t, by_slot) * (size_t)as;
  double *D = D0 + (size_t)t * (size_t)ds;
  const int k = (int)blockIdx.x * AS_NT + (int)threadIdx.x;
  if (k >= nnz) return;
  const int i = as_row_of(ptr, n, k);
  D[(size_t)i + (size_t)col[k] * n] = val[k];
}
// packed == 0: block t of src to block t of dst. packed == 1: block j < k' of src (the packed inverses) to the candidate
// slot of the term it belongs to.
__global__ __launch_bounds__(AS_NT) void k_asb_sym_dense(int n, const double *__restrict__ src0, long long ss, double *__restrict__ dst0,
                                                         long long ds, int packed, const int *__restrict__ sel) {
  const int j = (int)blockIdx.y;
  if (j >= (packed ? sel[ASB_NZ] : sel[0])) return;
  const double *src = src0 + (size_t)j * (size_t)ss;
  double *dst = dst0 + (size_t)(packed ? sel[ASB_ZTERM + j] : j) * (size_t)ds;
  const long long e = (long long)blockIdx.x * AS_NT + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int i = (int)(e % n), jj = (int)(e / n);
  dst[e] = (src[e] + src[(size_t)jj + (size_t)i * n]) * 0.5;
}
#undef MI_ASB_TERM

// The workspace of the batched set-up of one bank, for kcap terms. Allocated at the first batched call; a later call with
// more terms than any before allocates it anew (nothing outside a call points into it).
struct AmgBankSetupWs {
  int kcap = 0;
  int64_t cs = 0, wap_s = 0, wm_s = 0, part_s = 0, nn = 0;   // strides in doubles
  DevBuf<double> cand, w_ap, w_m, part, dense, dense_s, z_raw;
  DevBuf<int> flag, sel;
  int64_t bytes() const {
    return 8 * (int64_t)(cand.n + w_ap.n + w_m.n + part.n + dense.n + dense_s.n + z_raw.n) + 4 * (int64_t)(flag.n + sel.n);
  }
};

// One term's verdict
struct AsbTerm {
  bool ok = true;
  std::string why;
};

// The chain on the engine `eng` (plan, patterns) for k terms: values of A_0 at a_slab + slots[t] * a_stride. `off_*`: the
// bank's slot layout, `a0_len` the (even) doubles of A_0 at its head. On return the candidate slot of every healthy term
// holds everything of the member's slot behind A_0, and term[t] says which are healthy. Synchronous up to the inverses;
// the caller commits.
inline void amg_bank_setup_batch(AmgPlanOp &eng, AmgBankSetupWs &W, int k, const int64_t *members, const int64_t *slots, const double *a_slab,
                                 int64_t a_stride, const std::vector<int64_t> &off_a, const std::vector<int64_t> &off_p,
                                 const std::vector<int64_t> &off_r, const std::vector<int64_t> &off_wd, int64_t off_z, int64_t off_om, int64_t stride,
                                 int64_t a0_len, std::vector<AsbTerm> &term) {
  mi_ctx_s *ctx = eng.ctx;
  hipStream_t s = ctx->stream;
  const int nlev = eng.nlev, nc = eng.nc;
  const amgp::Plan &plan = eng.plan;
  auto grid = [](int64_t m) { return (unsigned)AmgPlanOp::grid(m); };
  if (k > W.kcap) {
    int64_t w1 = 1, w2 = 1;
    size_t nmax = 1;
    for (int l = 0; l < nlev; ++l) {
      nmax = std::max(nmax, (size_t)plan.lv[(size_t)l].n);
      if (l + 1 < nlev) { w1 = std::max(w1, plan.lv[(size_t)l].ap_nnz()); w2 = std::max(w2, plan.lv[(size_t)l + 1].a_nnz()); }
    }
    W = AmgBankSetupWs();
    W.cs = stride - a0_len; W.wap_s = w1 + 1; W.wm_s = w2 + 1; W.part_s = (int64_t)grid((int64_t)nmax) + 1; W.nn = (int64_t)nc * nc;
    const size_t K = (size_t)k;
    W.cand.alloc((size_t)W.cs * K); W.w_ap.alloc((size_t)W.wap_s * K); W.w_m.alloc((size_t)W.wm_s * K); W.part.alloc((size_t)W.part_s * K);
    W.dense.alloc((size_t)W.nn * K); W.dense_s.alloc((size_t)W.nn * K); W.z_raw.alloc((size_t)W.nn * K);
    W.flag.alloc(2 * K); W.sel.alloc((size_t)ASB_SEL);
    MI_HIP(hipMemsetAsync(W.cand.p, 0, (size_t)W.cs * K * sizeof(double), s));   // the padding doubles travel with a commit: zeros
    W.kcap = k;
  }
  term.assign((size_t)k, AsbTerm());
  std::vector<int> sh((size_t)ASB_SEL, 0);
  sh[0] = k;
  for (int t = 0; t < k; ++t) { sh[(size_t)1 + t] = (int)members[t]; sh[(size_t)ASB_SLOT + t] = (int)slots[t]; }
  MI_HIP(hipMemcpyAsync(W.sel.p, sh.data(), sh.size() * sizeof(int), hipMemcpyHostToDevice, s));
  MI_HIP(hipMemsetAsync(W.flag.p, 0, 2 * (size_t)k * sizeof(int), s));
  const int *sel = W.sel.p;
  const unsigned ky = (unsigned)k;
  const long long cs = W.cs;
  auto co = [&](int64_t off) { return (long long)(off - a0_len); };   // an offset of the bank's slot, in a candidate slot
  for (int l = 0; l + 1 < nlev; ++l) {
    const amgp::Level &H = plan.lv[(size_t)l], &HN = plan.lv[(size_t)l + 1];
    AmgOp::Level &L = eng.lv[(size_t)l], &N = eng.lv[(size_t)l + 1];
    AmgPlanOp::Dev &D = eng.dv[(size_t)l], &DN = eng.dv[(size_t)l + 1];
    const int by_slot = l == 0;
    const double *a = l ? W.cand.p + co(off_a[(size_t)l]) : a_slab;
    const long long as = l ? cs : (long long)a_stride;
    const int n = H.n;
    const unsigned nb = grid(n);
    const int pn = (int)H.p_nnz(), apn = (int)H.ap_nnz(), cn = (int)HN.a_nnz();
    const long long o_om = co(off_om) + 2 * l, o_wd = co(off_wd[(size_t)l]), o_p = co(off_p[(size_t)l]), o_r = co(off_r[(size_t)l]);
    hipLaunchKernelGGL(k_asb_gersh, dim3(nb, ky), dim3(AS_NT), 0, s, n, (const int *)L.A.rowptr.p, a, as, by_slot, (const int *)D.diag.p, W.part.p,
                       (long long)W.part_s, W.flag.p, sel);
    hipLaunchKernelGGL(k_asb_omega, dim3(1, ky), dim3(AS_NT), 0, s, (int)nb, (const double *)W.part.p, (long long)W.part_s, W.cand.p + o_om, cs, sel);
    hipLaunchKernelGGL(k_asb_prolong, dim3(nb, ky), dim3(AS_NT), 0, s, n, a, as, by_slot, (const int *)D.diag.p, (const int *)D.agg.p,
                       (const double *)D.tw.p, (const int *)L.P.rowptr.p, (const int *)L.P.col.p, (const int *)D.seg_ptr.p, (const int *)D.seg_src.p,
                       W.cand.p, cs, o_om, o_wd, o_p, sel);
    hipLaunchKernelGGL(k_asb_gather, dim3(grid(pn), ky), dim3(AS_NT), 0, s, pn, (const int *)D.r_from.p, W.cand.p, cs, o_p, o_r, sel);
    hipLaunchKernelGGL(k_asb_product, dim3(grid(apn), ky), dim3(AS_NT), 0, s, n, apn, (const int *)D.ap_ptr.p, (const int *)D.ap_col.p,
                       (const int *)L.A.rowptr.p, (const int *)L.A.col.p, a, as, by_slot, (const int *)L.P.rowptr.p, (const int *)L.P.col.p,
                       (const double *)W.cand.p + o_p, cs, W.w_ap.p, (long long)W.wap_s, sel);
    hipLaunchKernelGGL(k_asb_product, dim3(grid(cn), ky), dim3(AS_NT), 0, s, HN.n, cn, (const int *)N.A.rowptr.p, (const int *)N.A.col.p,
                       (const int *)L.R.rowptr.p, (const int *)L.R.col.p, (const double *)W.cand.p + o_r, cs, 0, (const int *)D.ap_ptr.p,
                       (const int *)D.ap_col.p, (const double *)W.w_ap.p, (long long)W.wap_s, W.w_m.p, (long long)W.wm_s, sel);
    hipLaunchKernelGGL(k_asb_sym, dim3(grid(cn), ky), dim3(AS_NT), 0, s, cn, (const int *)DN.sym.p, (const double *)W.w_m.p, (long long)W.wm_s,
                       W.cand.p + co(off_a[(size_t)l + 1]), cs, sel);
  }
  MI_HIP(hipGetLastError());
  const amgp::Level &HC = plan.lv[(size_t)nlev - 1];
  AmgOp::Level &C = eng.lv[(size_t)nlev - 1];
  AmgPlanOp::Dev &DC = eng.dv[(size_t)nlev - 1];
  const int c_slot = nlev == 1;
  const double *ac = nlev > 1 ? W.cand.p + co(off_a[(size_t)nlev - 1]) : a_slab;
  const long long acs = nlev > 1 ? cs : (long long)a_stride;
  const int cn = (int)HC.a_nnz();
  const size_t nn = (size_t)W.nn;
  hipLaunchKernelGGL(k_asb_gersh, dim3(grid(nc), ky), dim3(AS_NT), 0, s, nc, (const int *)C.A.rowptr.p, ac, acs, c_slot, (const int *)DC.diag.p, W.part.p,
                     (long long)W.part_s, W.flag.p, sel);
  MI_HIP(hipMemsetAsync(W.dense.p, 0, nn * (size_t)k * sizeof(double), s));
  hipLaunchKernelGGL(k_asb_dense, dim3(grid(cn), ky), dim3(AS_NT), 0, s, nc, cn, (const int *)C.A.rowptr.p, (const int *)C.A.col.p, ac, acs, c_slot,
                     W.dense.p, (long long)nn, sel);
  hipLaunchKernelGGL(k_asb_sym_dense, dim3(grid((int64_t)nn), ky), dim3(AS_NT), 0, s, nc, (const double *)W.dense.p, (long long)nn, W.dense_s.p,
                     (long long)nn, 0, sel);
  MI_HIP(hipGetLastError());
  std::vector<int> fh(2 * (size_t)k, 0);
  MI_HIP(hipMemcpyAsync(fh.data(), W.flag.p, fh.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  MI_HIP(hipStreamSynchronize(s));
  std::vector<int> healthy;
  for (int t = 0; t < k; ++t) {
    AsbTerm &T = term[(size_t)t];
    if (fh[(size_t)2 * t + 1]) { T.ok = false; T.why = "a value of the matrix, or of a level built from it, is not finite"; }
    else if (fh[(size_t)2 * t]) { T.ok = false; T.why = "a diagonal entry of a level is missing or not positive (the matrix is not positive definite)"; }
    else healthy.push_back(t);
  }
  if (healthy.empty()) return;
  // the healthy blocks, packed to the front of dense_s in the order of their terms (block j <= its term: a move downwards)
  const int kz = (int)healthy.size();
  for (int j = 0; j < kz; ++j)
    if (healthy[(size_t)j] != j)
      MI_HIP(hipMemcpyAsync(W.dense_s.p + (size_t)j * nn, W.dense_s.p + (size_t)healthy[(size_t)j] * nn, nn * sizeof(double), hipMemcpyDeviceToDevice, s));
  std::vector<int64_t> sizes((size_t)kz, (int64_t)nc);
  std::vector<std::string> failed;
  pinv_blocks_fast(ctx, kz, sizes.data(), W.dense_s.p, 0.0, W.z_raw.p, true, &failed);
  std::vector<int> good;
  for (int j = 0; j < kz; ++j) {
    AsbTerm &T = term[(size_t)healthy[(size_t)j]];
    if (failed[(size_t)j].empty()) { good.push_back(j); continue; }
    char buf[512];
    std::snprintf(buf, sizeof buf, "the coarsest level (%d rows): %s", nc, failed[(size_t)j].c_str());
    T.ok = false; T.why = buf;
  }
  // the inverses symmetrised into the candidate slots: all k' blocks in one launch (a block without its certificate holds
  // what it held before; its term is not committed)
  sh[(size_t)ASB_NZ] = kz;
  for (int j = 0; j < kz; ++j) sh[(size_t)ASB_ZTERM + j] = healthy[(size_t)j];
  MI_HIP(hipMemcpyAsync(W.sel.p, sh.data(), sh.size() * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_asb_sym_dense, dim3(grid((int64_t)nn), (unsigned)kz), dim3(AS_NT), 0, s, nc, (const double *)W.z_raw.p, (long long)nn,
                     W.cand.p + co(off_z), cs, 1, sel);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));   // `sh` dies with this frame
}

}  // namespace mi
