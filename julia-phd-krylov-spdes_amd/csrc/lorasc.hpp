// LORASC preconditioner `ΠA_lorasc \ r` on the full system (Grigori, Nataf, Yousef, Inria RR-8557): the reference's
// `LorascPreconditioner` / `apply_lorasc` (EPDD.jl:1406-1428, 1908-1976), the M of `pcg(A, b, zeros, ΠA_lorasc)` and
// `defpcg(A, b, zeros, ϕ, ΠA_lorasc)` in Example03:255-268.
//
// x is indexed like the rows of A (`not_dirichlet_inds_g2l`); pos_I / pos_Γ say where the interior nodes (concatenated,
// the order of the set-up plan's b_I) and the Γ nodes sit in it. One apply, all on the context's stream, no host, no
// atomics, every sum in a fixed order:
//   1 k_lo_gather    f_I = x[pos_I]                                                            (:1922-1926)
//   2 level solve    y_I = A_IId \ f_I, all subdomains at once (setup_gj.hpp, gj_level_enqueue) (:1938)
//   3 k_lo_zgamma    z_Γ = x[pos_Γ] - Σ_d A_IΓd' y_Id: per Γ node, d ascending, each column summed from 0 in stored order and
//                    then subtracted — Julia's `z_Γ .-= A_IΓd' * x_Id` (:1941); then the workgroup's partial dots E_k' z_Γ
//   4 A_ΓΓ \ z_Γ     the sparse direct operator (spd_direct.hpp), two launches                  (:1950)
//   5 k_lo_correct   x_Γ += Σ_k (coef_k E_k' z_Γ) E_k, k ascending (:1954-1957); stores x_Γ and u[pos_Γ] (:1971-1973)
//   6 k_lo_coupling  w_I = A_IΓd x_Γ: per interior row, ascending Γ column from 0 — the bits of Julia's CSC product (:1960)
//   7 level solve    v_I = A_IId \ w_I
//   8 k_lo_finish    u[pos_I] = y_I - v_I                                                       (:1960, 1964-1968)
//
// The quirk of :1954-1957: the loop runs `for (k, σ) in enumerate(Σ)` and never uses σ, although prepare_lorasc_precond
// stores Σ[k] = (ε - σ)/σ (:1596) and leaves E[k] A_ΓΓ-orthonormal — the paper's correction would be Σ_k Σ[k] (E_k'z) E_k.
// coef == NULL (ones) is the reference as written; the paper's form is coef = Σ.
#pragma once
#include "setup_gj.hpp"
#include "spd_direct.hpp"

namespace mi {

constexpr int LO_MAX_NEV = 1024;   // t_k of k_lo_correct: 8 KiB of LDS

__global__ __launch_bounds__(256) void k_lo_gather(int n, const int *__restrict__ pos, const double *__restrict__ x,
                                                   double *__restrict__ f, const int *done) {
  if (done && *done) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) f[q] = x[pos[q]];
}

// One thread per Γ node g (grid = ceil(n_g / 256), the slices of the partial dots). Column form: the segments
// gseg_ptr[g] .. gseg_ptr[g + 1] are the subdomains (ascending) that hold entries in column g, a segment's entries
// seg_ptr[s] .. seg_ptr[s + 1] are in stored order: c_row = row in the concatenated interior vector, c_src = index into val.
// part[k * nwg + workgroup] = Σ_{g in slice} E[g, k] z[g]: four strided terms per lane, then the wave's shuffle tree.
__global__ __launch_bounds__(256) void k_lo_zgamma(int n_g, int nev, int nwg, const int *__restrict__ pos_g,
                                                   const int *__restrict__ gseg_ptr, const int *__restrict__ seg_ptr,
                                                   const int *__restrict__ c_row, const int *__restrict__ c_src,
                                                   const double *__restrict__ val, const double *__restrict__ x,
                                                   const double *__restrict__ y_I, const double *__restrict__ E,
                                                   double *__restrict__ z_out, double *__restrict__ part, const int *done) {
  if (done && *done) return;
  __shared__ double zs[256];
  const int tid = threadIdx.x, g0 = blockIdx.x * 256, g = g0 + tid;
  double z = 0.0;
  if (g < n_g) {
    z = x[pos_g[g]];
    for (int sg = gseg_ptr[g]; sg < gseg_ptr[g + 1]; ++sg) {
      double s = 0.0;
      for (int e = seg_ptr[sg]; e < seg_ptr[sg + 1]; ++e) s += val[c_src[e]] * y_I[c_row[e]];
      z -= s;
    }
    z_out[g] = z;
  }
  if (nev == 0) return;
  zs[tid] = z;
  __syncthreads();
  const int w = tid >> 6, lane = tid & 63;
  for (int k = w; k < nev; k += 4) {
    const double *Ek = E + (size_t)k * n_g + g0;
    double p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = lane + 64 * j;
      p[j] = g0 + t < n_g ? Ek[t] * zs[t] : 0.0;
    }
    const double v = sd_wave_sum(((p[0] + p[1]) + p[2]) + p[3]);
    if (lane == 0) part[(size_t)k * nwg + blockIdx.x] = v;
  }
}

// Every workgroup: t_k = coef_k Σ_wg part[k][wg] (ascending workgroup) in LDS; then its 256 Γ nodes.
__global__ __launch_bounds__(256) void k_lo_correct(int n_g, int nev, int nwg, const int *__restrict__ pos_g,
                                                    const double *__restrict__ E, const double *__restrict__ coef,
                                                    const double *__restrict__ part, double *__restrict__ xg,
                                                    double *__restrict__ u, const int *done) {
  if (done && *done) return;
  __shared__ double t[LO_MAX_NEV];
  const int tid = threadIdx.x, g = blockIdx.x * 256 + tid;
  for (int k = tid; k < nev; k += 256) {
    const double *pk = part + (size_t)k * nwg;
    double s = 0.0;
    for (int wg = 0; wg < nwg; ++wg) s += pk[wg];
    t[k] = coef[k] * s;
  }
  __syncthreads();
  if (g >= n_g) return;
  double acc = xg[g];
  for (int k = 0; k < nev; ++k) acc += t[k] * E[g + (size_t)k * n_g];
  xg[g] = acc;
  u[pos_g[g]] = acc;
}

// Row form: w_I[i] = Σ_j A_IΓ[i, j] x_Γ[j], the entries of row i in ascending Γ column
__global__ __launch_bounds__(256) void k_lo_coupling(int n_I, const int *__restrict__ r_ptr, const int *__restrict__ r_col,
                                                     const int *__restrict__ r_src, const double *__restrict__ val,
                                                     const double *__restrict__ xg, double *__restrict__ w, const int *done) {
  if (done && *done) return;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_I; i += gridDim.x * 256) {
    double s = 0.0;
    for (int e = r_ptr[i]; e < r_ptr[i + 1]; ++e) s += val[r_src[e]] * xg[r_col[e]];
    w[i] = s;
  }
}

__global__ __launch_bounds__(256) void k_lo_finish(int n_I, const int *__restrict__ pos_I, const double *__restrict__ y,
                                                   const double *__restrict__ v, double *__restrict__ u, const int *done) {
  if (done && *done) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n_I; q += gridDim.x * 256) u[pos_I[q]] = y[q] - v[q];
}

struct LorascOp : Operator {
  mi_setup_s *plan;      // borrowed: the interior solves (its `bound` count refuses mi_schur_setup_destroy while we live)
  mi_op_s *gg_h;         // borrowed: the A_ΓΓ solver's handle (`bound` refuses mi_op_destroy)
  SpdDirectOp *gg;
  int n_I = 0, n_g = 0, nev = 0, nwg = 0;
  int64_t nnz = 0;
  DevBuf<int> pos_I, pos_g, gseg_ptr, seg_ptr, c_row, c_src, r_ptr, r_col, r_src;
  DevBuf<double> val, E, coef, part, f_I, y_I, w_I, v_I, z_g, x_g;

  LorascOp(mi_ctx_s *c, int64_t ndom, int64_t n_, int64_t n_gamma, const int64_t *n_i, const int64_t *const *pI,
           const int64_t *pG, const int64_t *const *ig_ptr, const int64_t *const *ig_idx, const double *const *ig_val,
           mi_setup_s *plan_, mi_op_s *gg_h_, int64_t nev_, const double *E_, const double *coef_, int base)
      : Operator(c, n_), plan(plan_), gg_h(gg_h_), gg(nullptr) {
    const char *me = "mi_lorasc_create";
    if (c->n_ranks > 1) raise(MI_ERR_BAD_ARG, "%s: the operator is replicated only; this context is rank %d of %d", me, c->rank, c->n_ranks);
    if (ndom <= 0 || n_ <= 0 || n_ >= INT32_MAX || n_gamma <= 0 || !n_i || !pI || !pG || !ig_ptr || !ig_idx || !ig_val ||
        (base != 0 && base != 1))
      raise(MI_ERR_BAD_ARG, "%s: NULL argument, bad size or index_base", me);
    if (!plan || plan->ctx != c) raise(MI_ERR_BAD_ARG, "%s: the set-up plan is NULL or lives on another context", me);
    gg = gg_h && gg_h->impl ? dynamic_cast<SpdDirectOp *>(gg_h->impl.get()) : nullptr;
    if (!gg || gg->ctx != c) raise(MI_ERR_BAD_ARG, "%s: a_gg_solver is not a sparse direct operator (mi_spd_direct_create) of this context", me);
    if (gg->n != n_gamma) raise(MI_ERR_BAD_ARG, "%s: a_gg_solver has size %lld, n_gamma is %lld", me, (long long)gg->n, (long long)n_gamma);
    if (plan->ndom != ndom) raise(MI_ERR_BAD_ARG, "%s: %lld subdomains, the plan has %d", me, (long long)ndom, plan->ndom);
    int64_t tot = 0;
    for (int64_t d = 0; d < ndom; ++d) {
      if (n_i[d] != plan->dom[d].n_i)
        raise(MI_ERR_BAD_ARG, "%s: n_i[%lld] = %lld, the plan's subdomain has %d interior nodes", me, (long long)d, (long long)n_i[d], plan->dom[d].n_i);
      tot += n_i[d];
    }
    if (!plan->gj || !plan->gj->keep || !plan->gj->have_levels)
      raise(MI_ERR_BAD_ARG, "%s: the plan keeps no level inverses (mi_schur_setup_keep_levels(plan, 1) and a run after it)", me);
    if (tot <= 0 || tot + n_gamma != n_) raise(MI_ERR_BAD_ARG, "%s: n = %lld is not Σ n_i + n_gamma = %lld", me, (long long)n_, (long long)(tot + n_gamma));
    n_I = (int)tot; n_g = (int)n_gamma; nwg = (n_g + 255) / 256;
    // the two maps: together a permutation of 0..n-1
    std::vector<int> hI((size_t)n_I), hG((size_t)n_g);
    std::vector<char> seen((size_t)n_, 0);
    auto place = [&](int64_t v, const char *what) {
      v -= base;
      if (v < 0 || v >= n_) raise(MI_ERR_BAD_ARG, "%s: %s index %lld out of range (n = %lld)", me, what, (long long)(v + base), (long long)n_);
      if (seen[(size_t)v]) raise(MI_ERR_BAD_ARG, "%s: pos_I and pos_gamma are not a permutation of the rows: index %lld appears twice", me, (long long)(v + base));
      seen[(size_t)v] = 1;
      return (int)v;
    };
    size_t q = 0;
    for (int64_t d = 0; d < ndom; ++d) {
      if (n_i[d] && !pI[d]) raise(MI_ERR_BAD_ARG, "%s: pos_I[%lld] is NULL", me, (long long)d);
      for (int64_t i = 0; i < n_i[d]; ++i) hI[q++] = place(pI[d][i], "pos_I");
    }
    for (int64_t g = 0; g < n_gamma; ++g) hG[(size_t)g] = place(pG[g], "pos_gamma");
    // the stacked A_IΓd: values in the caller's concatenated CSC order, a column form and a row form that point into them
    std::vector<int64_t> voff((size_t)ndom + 1, 0), ioff((size_t)ndom + 1, 0);
    for (int64_t d = 0; d < ndom; ++d) {
      if (!ig_ptr[d]) raise(MI_ERR_BAD_ARG, "%s: ig_colptr[%lld] is NULL", me, (long long)d);
      if (ig_ptr[d][0] != base) raise(MI_ERR_BAD_ARG, "%s: ig_colptr[%lld][0] != index_base", me, (long long)d);
      for (int64_t g = 0; g < n_gamma; ++g)
        if (ig_ptr[d][g + 1] < ig_ptr[d][g]) raise(MI_ERR_BAD_ARG, "%s: ig_colptr[%lld] decreases at column %lld", me, (long long)d, (long long)g);
      const int64_t nz = ig_ptr[d][n_gamma] - base;
      if (nz && (!ig_idx[d] || !ig_val[d])) raise(MI_ERR_BAD_ARG, "%s: ig_rowval / ig_nzval [%lld] is NULL", me, (long long)d);
      voff[d + 1] = voff[d] + nz; ioff[d + 1] = ioff[d] + n_i[d];
      if (voff[d + 1] >= INT32_MAX) raise(MI_ERR_BAD_ARG, "%s: more than 2^31 stored entries", me);
    }
    nnz = voff[ndom];
    std::vector<int> gp((size_t)n_g + 1), sp, cr((size_t)nnz), cs((size_t)nnz), rp((size_t)n_I + 1, 0), rc((size_t)nnz), rs((size_t)nnz);
    std::vector<double> hv((size_t)nnz);
    size_t e = 0;
    for (int g = 0; g < n_g; ++g) {
      gp[g] = (int)sp.size();
      for (int64_t d = 0; d < ndom; ++d) {
        const int64_t a = ig_ptr[d][g] - base, b = ig_ptr[d][g + 1] - base;
        if (a == b) continue;
        sp.push_back((int)e);
        for (int64_t k = a; k < b; ++k, ++e) {
          const int64_t r = ig_idx[d][k] - base;
          if (r < 0 || r >= n_i[d]) raise(MI_ERR_BAD_ARG, "%s: ig_rowval[%lld] holds row %lld out of range (n_i = %lld)", me, (long long)d, (long long)(r + base), (long long)n_i[d]);
          cr[e] = (int)(ioff[d] + r); cs[e] = (int)(voff[d] + k);
          ++rp[(size_t)cr[e] + 1];
        }
      }
    }
    gp[n_g] = (int)sp.size();
    sp.push_back((int)e);
    for (int i = 0; i < n_I; ++i) rp[i + 1] += rp[i];
    {   // rows: the column form runs through the columns in ascending order, so each row fills in ascending Γ column
      std::vector<int> fill(rp.begin(), rp.end() - 1);
      for (int g = 0; g < n_g; ++g)
        for (int x = sp[gp[g]]; x < sp[gp[g + 1]]; ++x) { const int at = fill[cr[x]]++; rc[at] = g; rs[at] = cs[x]; }
    }
    for (int64_t d = 0; d < ndom; ++d)
      if (voff[d + 1] > voff[d]) std::memcpy(hv.data() + voff[d], ig_val[d], sizeof(double) * (size_t)(voff[d + 1] - voff[d]));
    hipStream_t s = c->stream;
    auto up = [&](DevBuf<int> &dst, const std::vector<int> &h) { dst.upload(h.empty() ? std::vector<int>{0} : h, s); };
    up(pos_I, hI); up(pos_g, hG); up(gseg_ptr, gp); up(seg_ptr, sp); up(c_row, cr); up(c_src, cs); up(r_ptr, rp); up(r_col, rc); up(r_src, rs);
    val.upload(hv.empty() ? std::vector<double>{0.0} : hv, s);
    f_I.alloc((size_t)n_I); y_I.alloc((size_t)n_I); w_I.alloc((size_t)n_I); v_I.alloc((size_t)n_I);
    z_g.alloc((size_t)n_g); x_g.alloc((size_t)n_g);
    set_correction_host(nev_, E_, coef_, me);
    MI_HIP(hipStreamSynchronize(s));
    ++plan->bound; ++gg_h->bound;   // last: nothing above may leave a count behind
  }
  ~LorascOp() override { --plan->bound; --gg_h->bound; }

  static void check_nev(int64_t k, const double *E_, const char *me) {
    if (k < 0 || k > LO_MAX_NEV) raise(MI_ERR_BAD_ARG, "%s: nev = %lld, the correction holds at most %d vectors", me, (long long)k, LO_MAX_NEV);
    if (k && !E_) raise(MI_ERR_BAD_ARG, "%s: E is NULL with nev = %lld", me, (long long)k);
  }
  // E (n_g x k, column-major) and coef (k, or NULL: ones) as HOST arrays
  void set_correction_host(int64_t k, const double *E_, const double *coef_, const char *me) {
    check_nev(k, E_, me);
    hipStream_t s = ctx->stream;
    std::vector<double> ones((size_t)k, 1.0);
    E.upload(E_, (size_t)k * n_g, s);
    coef.upload(coef_ ? coef_ : ones.data(), (size_t)k, s);
    part.ensure((size_t)k * nwg);
    MI_HIP(hipStreamSynchronize(s));
    nev = (int)k;
  }
  // the same with DEVICE arrays
  void set_correction_dev(int64_t k, const double *E_, const double *coef_) {
    hipStream_t s = ctx->stream;
    E.ensure((size_t)k * n_g); coef.ensure((size_t)k); part.ensure((size_t)k * nwg);
    if (k) MI_HIP(hipMemcpyAsync(E.p, E_, sizeof(double) * (size_t)k * n_g, hipMemcpyDeviceToDevice, s));
    if (k && coef_) MI_HIP(hipMemcpyAsync(coef.p, coef_, sizeof(double) * (size_t)k, hipMemcpyDeviceToDevice, s));
    else if (k) coef.upload(std::vector<double>((size_t)k, 1.0), s);
    MI_HIP(hipStreamSynchronize(s));
    nev = (int)k;
  }
  // new A_IΓd values (device pointer, the concatenated CSC order of create): one copy
  void set_values(const double *v) {
    if (nnz) MI_HIP(hipMemcpyAsync(val.p, v, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, ctx->stream));
  }

  void level_solve(const double *f, double *u) {
    if (!plan->gj || !plan->gj->keep || !plan->gj->have_levels)
      raise(MI_ERR_BAD_ARG, "mi_lorasc: the plan keeps no level inverses any more (mi_schur_setup_keep_levels(plan, 1) and a run after it)");
    gj_level_enqueue(*plan, ctx->stream, f, u);
  }
  static int grid(int n) { return std::max(1, std::min((n + 255) / 256, 4096)); }
  void apply(const double *x, double *u, const int *done) override {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_lo_gather, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, x, f_I.p, done);
    level_solve(f_I.p, y_I.p);
    hipLaunchKernelGGL(k_lo_zgamma, dim3(nwg), dim3(256), 0, s, n_g, nev, nwg, (const int *)pos_g.p, (const int *)gseg_ptr.p,
                       (const int *)seg_ptr.p, (const int *)c_row.p, (const int *)c_src.p, (const double *)val.p, x,
                       (const double *)y_I.p, (const double *)E.p, z_g.p, part.p, done);
    gg->apply(z_g.p, x_g.p, done);
    hipLaunchKernelGGL(k_lo_correct, dim3(nwg), dim3(256), 0, s, n_g, nev, nwg, (const int *)pos_g.p, (const double *)E.p,
                       (const double *)coef.p, (const double *)part.p, x_g.p, u, done);
    hipLaunchKernelGGL(k_lo_coupling, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)r_ptr.p, (const int *)r_col.p,
                       (const int *)r_src.p, (const double *)val.p, (const double *)x_g.p, w_I.p, done);
    level_solve(w_I.p, v_I.p);
    hipLaunchKernelGGL(k_lo_finish, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, (const double *)y_I.p,
                       (const double *)v_I.p, u, done);
    MI_HIP(hipGetLastError());
  }
  bool writes_y_once() const override { return false; }   // u is written by two launches (5 and 8)
  // bytes: one level solve streams the kept inverses once (the dominant figure; its vectors ride along); the apply is two
  // of them, the A_ΓΓ solve, and the glue: both forms of A_IΓ (value, source index and row / column index per entry), E
  // twice, the partials, and the vectors of launches 1, 3, 5, 6 and 8
  void bytes(int64_t *a, int64_t *d) const override {
    const int64_t lv = 8 * ((int64_t)(plan->gj ? plan->gj->zstore.n : 0) + 4 * (int64_t)n_I);
    int64_t ga = 0, gd = 0;
    gg->bytes(&ga, &gd);
    const int64_t glue = 2 * 16 * nnz + 4 * ((int64_t)n_I + 2 * n_g) + 2 * 8 * (int64_t)nev * n_g + 8 * (int64_t)nev * nwg * (1 + nwg) +
                         (8 + 4) * 2 * ((int64_t)n_I + n_g) + 8 * (4 * (int64_t)n_I + 5 * (int64_t)n_g);
    *d = lv;
    *a = 2 * lv + ga + glue;
  }
  void apply_dominant(const double *x) override {
    hipLaunchKernelGGL(k_lo_gather, dim3(grid(n_I)), dim3(256), 0, ctx->stream, n_I, (const int *)pos_I.p, x, f_I.p, (const int *)nullptr);
    level_solve(f_I.p, y_I.p);
  }
};

}  // namespace mi
