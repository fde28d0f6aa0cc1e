// What the full-system preconditioners built on an interior/Γ split share on the device (lorasc.hpp, nn_induced.hpp): the
// uploaded index arrays of full_split_plan.hpp, the values of the stacked A_IΓ, the interior vectors, the two level solves
// through the borrowed set-up plan, and the launches that are the same in both applies:
//   k_lo_gather       f_I = x[pos_I]
//   level solve       y_I = A_IId \ f_I, all subdomains at once (setup_gj.hpp, gj_level_enqueue)
//   k_lo_zgamma       z_Γ = x[pos_Γ] - Σ_d A_IΓd' y_Id over the column form (and LORASC's partial dots)
//   k_split_coupling  w_I = A_IΓ v or f_I - A_IΓ v over the row form
//   level solve       v_I = A_IId \ w_I
//   k_lo_finish / k_nni_scatter   u[pos_I] = y_I - v_I / v_I
// All on the context's stream, no host, no atomics, every sum in a fixed order.
#pragma once
#include "full_split_plan.hpp"
#include "spd_direct.hpp"   // setup_gj.hpp (the level solves) and sd_wave_sum

namespace mi {

__global__ __launch_bounds__(256) void k_lo_gather(int n, const int *__restrict__ pos, const double *__restrict__ x,
                                                   double *__restrict__ f, const int *done) {
  if (done && *done) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) f[q] = x[pos[q]];
}

// One thread per Γ node g (grid = ceil(n_g / 256), the slices of the partial dots). Column form: the segments
// gseg_ptr[g] .. gseg_ptr[g + 1] are the subdomains (ascending) that hold entries in column g, a segment's entries
// seg_ptr[s] .. seg_ptr[s + 1] are in stored order: c_row = row in the concatenated interior vector, c_src = index into val.
// Each column is summed from 0 and then subtracted — Julia's `z_Γ .-= A_IΓd' * x_Id`.
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

// Row form: s = Σ_j A_IΓ[i, j] v[r_col[j]], the entries of row i in ascending column from 0 — the bits of Julia's CSC
// product; w_I[i] = s, or f[i] - s where f is given
__global__ __launch_bounds__(256) void k_split_coupling(int n_I, const int *__restrict__ r_ptr, const int *__restrict__ r_col,
                                                        const int *__restrict__ r_src, const double *__restrict__ val,
                                                        const double *__restrict__ v, const double *__restrict__ f,
                                                        double *__restrict__ w, const int *done) {
  if (done && *done) return;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_I; i += gridDim.x * 256) {
    double s = 0.0;
    for (int e = r_ptr[i]; e < r_ptr[i + 1]; ++e) s += val[r_src[e]] * v[r_col[e]];
    w[i] = f ? f[i] - s : s;
  }
}

// u[pos_I] = y - v (LORASC) and u[pos_I] = v (induced): two kernels — merged into one with `y ? y[q] - v[q] : v[q]` the
// launch measured 15 % above k_lo_finish, outside the spread of five applies (profiles/NOTES.md)
__global__ __launch_bounds__(256) void k_lo_finish(int n_I, const int *__restrict__ pos_I, const double *__restrict__ y,
                                                   const double *__restrict__ v, double *__restrict__ u, const int *done) {
  if (done && *done) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n_I; q += gridDim.x * 256) u[pos_I[q]] = y[q] - v[q];
}

__global__ __launch_bounds__(256) void k_nni_scatter(int n_I, const int *__restrict__ pos_I, const double *__restrict__ v,
                                                     double *__restrict__ z, const int *done) {
  if (done && *done) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n_I; q += gridDim.x * 256) z[pos_I[q]] = v[q];
}

struct SplitOp : Operator {
  mi_setup_s *plan;      // borrowed: the interior solves (the derived operator's count refuses mi_schur_setup_destroy while it lives)
  const char *kind;      // "mi_lorasc" / "mi_nn_induced": the name in a message of the apply
  int n_I = 0, n_g = 0, nwg = 0;
  int64_t nnz = 0, totg = 0;
  DevBuf<int> pos_I, pos_g, gseg_ptr, seg_ptr, c_row, c_src, r_ptr, r_loc, r_gam, r_src;   // r_loc: gathered form only
  DevBuf<double> val, f_I, y_I, w_I, v_I;

  SplitOp(mi_ctx_s *c, int64_t n_, mi_setup_s *plan_, const char *kind_) : Operator(c, n_), plan(plan_), kind(kind_) {}

  bool has_levels() const { return plan->gj && plan->gj->keep && plan->gj->have_levels; }
  // first in a constructor: the context, the arguments' sizes and pointers (`others_ok`: the derived operator's own), the plan
  void check_args(const char *me, const split::Input &in, bool others_ok) const {
    std::string err;
    if (ctx->n_ranks > 1) raise(MI_ERR_BAD_ARG, "%s: the operator is replicated only; this context is rank %d of %d", me, ctx->rank, ctx->n_ranks);
    if (split::check_input(in, others_ok, err)) raise(MI_ERR_BAD_ARG, "%s: %s", me, err.c_str());
    if (!plan || plan->ctx != ctx) raise(MI_ERR_BAD_ARG, "%s: the set-up plan is NULL or lives on another context", me);
  }
  // the split (checked against the plan's sizes), its arrays on the device, the values and the interior vectors
  void build(const char *me, split::Input in) {
    if (plan->ndom != in.ndom) raise(MI_ERR_BAD_ARG, "%s: %lld subdomains, the plan has %d", me, (long long)in.ndom, plan->ndom);
    if (!has_levels())
      raise(MI_ERR_BAD_ARG, "%s: the plan keeps no level inverses (mi_schur_setup_keep_levels(plan, 1) and a run after it)", me);
    std::vector<int64_t> p_ni((size_t)in.ndom), p_ng((size_t)in.ndom);
    for (int64_t d = 0; d < in.ndom; ++d) { p_ni[d] = plan->dom[d].n_i; p_ng[d] = plan->dom[d].n_g; }
    in.plan_n_i = p_ni.data(); in.plan_n_gamma_d = p_ng.data();
    split::Plan pl;
    std::string err;
    if (split::make_plan(in, pl, err)) raise(MI_ERR_BAD_ARG, "%s: %s", me, err.c_str());
    n_I = pl.n_I; n_g = pl.n_g; nwg = (n_g + 255) / 256; nnz = pl.nnz; totg = pl.totg;
    std::vector<double> hv((size_t)nnz);
    for (int64_t d = 0; d < in.ndom; ++d)
      if (pl.voff[d + 1] > pl.voff[d]) std::memcpy(hv.data() + pl.voff[d], in.nzval[d], sizeof(double) * (size_t)(pl.voff[d + 1] - pl.voff[d]));
    hipStream_t s = ctx->stream;
    auto up = [&](DevBuf<int> &dst, const std::vector<int> &h) { dst.upload(h.empty() ? std::vector<int>{0} : h, s); };
    up(pos_I, pl.pos_I); up(pos_g, pl.pos_g); up(gseg_ptr, pl.gseg_ptr); up(seg_ptr, pl.seg_ptr); up(c_row, pl.c_row); up(c_src, pl.c_src);
    up(r_ptr, pl.r_ptr); up(r_gam, pl.r_gam); up(r_src, pl.r_src);
    if (in.gather) up(r_loc, pl.r_loc);
    val.upload(hv.empty() ? std::vector<double>{0.0} : hv, s);
    f_I.alloc((size_t)n_I); y_I.alloc((size_t)n_I); w_I.alloc((size_t)n_I); v_I.alloc((size_t)n_I);
  }

  // new A_IΓ values (device pointer, the concatenated CSC order of create): one copy
  void set_values(const double *v) {
    if (nnz) MI_HIP(hipMemcpyAsync(val.p, v, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, ctx->stream));
  }
  void level_solve(const double *f, double *u) {
    if (!has_levels())
      raise(MI_ERR_BAD_ARG, "%s: the plan keeps no level inverses any more (mi_schur_setup_keep_levels(plan, 1) and a run after it)", kind);
    gj_level_enqueue(*plan, ctx->stream, f, u);
  }
  static int grid(int n) { return std::max(1, std::min((n + 255) / 256, 4096)); }
  // launches 1 - 3: f_I, y_I and z_Γ (with the partial dots E_k' z_Γ where nev > 0)
  void interior_to_gamma(const double *x, int nev, const double *E, double *z_g, double *part, const int *done) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_lo_gather, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, x, f_I.p, done);
    level_solve(f_I.p, y_I.p);
    hipLaunchKernelGGL(k_lo_zgamma, dim3(nwg), dim3(256), 0, s, n_g, nev, nwg, (const int *)pos_g.p, (const int *)gseg_ptr.p,
                       (const int *)seg_ptr.p, (const int *)c_row.p, (const int *)c_src.p, (const double *)val.p, x,
                       (const double *)y_I.p, E, z_g, part, done);
  }
  // launches 6 - 8: w_I = [f -] A_IΓ v over the columns `r_col`, v_I = A_IId \ w_I, u[pos_I] = [y -] v_I
  void gamma_to_interior(const int *r_col, const double *v, const double *f, const double *y, double *u, const int *done) {
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_split_coupling, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)r_ptr.p, r_col, (const int *)r_src.p,
                       (const double *)val.p, v, f, w_I.p, done);
    level_solve(w_I.p, v_I.p);
    if (y) hipLaunchKernelGGL(k_lo_finish, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, y, (const double *)v_I.p, u, done);
    else hipLaunchKernelGGL(k_nni_scatter, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, (const double *)v_I.p, u, done);
    MI_HIP(hipGetLastError());
  }
  bool writes_y_once() const override { return false; }   // u is written by two launches (5 and 8)
  // bytes of one level solve: it streams the kept inverses once (the dominant figure; its vectors ride along)
  int64_t level_bytes() const { return 8 * ((int64_t)(plan->gj ? plan->gj->zstore.n : 0) + 4 * (int64_t)n_I); }
  // ... and of the shared glue: both forms of A_IΓ (value, source index and row / column index per entry), their pointers,
  // and the index and value of every gathered or scattered vector entry
  int64_t split_bytes() const { return 2 * 16 * nnz + 4 * ((int64_t)n_I + 2 * n_g) + (8 + 4) * 2 * ((int64_t)n_I + n_g); }
  void apply_dominant(const double *x) override {
    hipLaunchKernelGGL(k_lo_gather, dim3(grid(n_I)), dim3(256), 0, ctx->stream, n_I, (const int *)pos_I.p, x, f_I.p, (const int *)nullptr);
    level_solve(f_I.p, y_I.p);
  }
};

}  // namespace mi
