// The preconditioner that the Neumann-Neumann Schur preconditioner induces on the full system: the reference's
// `NeumannNeumannInducedPreconditioner` / `apply_neumann_neumann_induced` (EPDD.jl:2274-2285, 2363-2423), the M of
// `defpcg(A, b, ϕ, M=ΠA_induced_nn_local_mat)` and `pcg(A, b, M=ΠA_induced_nn_local_mat)` in Example03:300-319.
//
// r is indexed like the rows of A (`not_dirichlet_inds_g2l`); pos_I / pos_Γ say where the interior nodes (concatenated,
// the order of the set-up plan's b_I) and the Γ nodes sit in it. One apply, all on the context's stream, no host, no
// atomics, every sum in a fixed order:
//   1 k_lo_gather     f_I = r[pos_I]                                                             (:2383-2387)
//   2 level solve     y_I = A_IId \ f_I, all subdomains at once (setup_gj.hpp, gj_level_enqueue)  (:2395)
//   3 k_lo_zgamma     r_schur = r[pos_Γ] - Σ_d A_IΓdd' y_Id: per Γ node, d ascending over the subdomains that hold it, each
//                     column summed from 0 in stored order and then subtracted (nev = 0: no partial dots)  (:2393-2400)
//   4 k_gemv_nni      z_Γd = ΠS_d (r_schur[gather_d] / cnt): the SCALE GEMV of k_gemv_batched with two outputs per row,
//                     the slot value z_Γd / cnt and the local unweighted z_loc = z_Γd                      (:2403-2406)
//   5 k_nni_assemble  z_Γ[g] = Σ of the slots of g, ascending subdomain; stored into z_Γ and z[pos_Γ]      (:2408-2410, 2418-2420)
//   6 k_nni_coupling  w_I = f_I - A_IΓdd v: per interior row, ascending local column from 0 — the bits of Julia's CSC
//                     product and the broadcast of :2411
//   7 level solve     v_I = A_IId \ w_I                                                           (:2412)
//   8 k_nni_scatter   z[pos_I] = v_I                                                              (:2413-2415)
//
// The quirk of :2411: the interior is coupled to the LOCAL, unweighted, unassembled z_Γd, not to the assembled
// z_Γ[gather_d]. As written the operator is neither symmetric nor positive definite — the reference's own
// notice "this preconditioner only seems to work with deflation". MI_NNI_AS_WRITTEN keeps it; MI_NNI_ASSEMBLED is
// v = z_Γ[gather_d], the textbook form [I -A_II⁻¹A_IΓ; 0 I] diag(A_II⁻¹, M_NN) [I 0; -A_ΓI A_II⁻¹ I].
#pragma once
#include "lorasc.hpp"

namespace mi {

// k_gemv_batched<RPW, true, WAVES, MT> (kernels.hpp) with a second output: the same tile records, the same operand-first
// ordering, the same GemvRows — for the same x the slot values carry the bits of the Neumann-Neumann apply.
template <int RPW, int WAVES, typename MT = double>
__global__ __launch_bounds__(64 * WAVES) void k_gemv_nni(DenseMeta m, const double *__restrict__ x, double *__restrict__ yslots,
                                                         double *__restrict__ z_loc, const int *done) {
  constexpr int NTH = 64 * WAVES;
  const GemvTile t = m.tiles[blockIdx.x];
  const int done0 = done ? *done : 0;
  asm volatile("" ::"s"(t.mat_off), "s"(t.n), "s"(t.ld), "s"(t.loc_off), "s"(t.row0), "s"(t.active), "s"(done0));
  if (done0) return;
  __shared__ __attribute__((aligned(16))) double xs[GEMV_PANEL];
  if (!t.active) return;
  const int off = t.loc_off, n = t.n;
  GemvRows<RPW, MT> rows;
  for (int c0 = 0; c0 < t.ld; c0 += GEMV_PANEL) {
    const int pw = min(GEMV_PANEL, t.ld - c0);  // multiple of 16
    if (c0) __syncthreads();
    // the operand gather (index -> value, two dependent loads) is issued BEFORE the first group of the matrix stream
    constexpr int XPT = (GEMV_PANEL + NTH - 1) / NTH;
    int gi[XPT];
#pragma unroll
    for (int q = 0; q < XPT; ++q) {
      const int j = c0 + q * NTH + (int)threadIdx.x;
      gi[q] = (q * NTH + (int)threadIdx.x < pw && j < n) ? m.gidx[off + j] : -1;
    }
    double xv[XPT];
#pragma unroll
    for (int q = 0; q < XPT; ++q) {
      const int j = c0 + q * NTH + (int)threadIdx.x;
      xv[q] = 0.0;
      if (gi[q] >= 0) xv[q] = x[gi[q]] / m.cnt[off + j];
    }
    if (c0 == 0) rows.begin(m, t);
#pragma unroll
    for (int q = 0; q < XPT; ++q) {
      const int l = q * NTH + (int)threadIdx.x;
      if (l < pw) xs[l] = xv[q];
    }
    __syncthreads();
    rows.panel(xs, c0, pw);
  }
  double sum[RPW];
  rows.finish(sum);
  const int row_base = t.row0 + (threadIdx.x >> 6) * RPW;
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int r = row_base + k;
    if (rows.lane == 0 && r < n) {
      yslots[m.out_pos[off + r]] = sum[k] / m.cnt[off + r];
      z_loc[off + r] = sum[k];
    }
  }
}

// k_assemble_slots (kernels.hpp) with both destinations of the Γ part
__global__ __launch_bounds__(256) void k_nni_assemble(int n_g, int width, const double *__restrict__ yslots,
                                                      const int *__restrict__ pos_g, double *__restrict__ z_g,
                                                      double *__restrict__ z, const int *done) {
  if (done && *done) return;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < n_g; g += gridDim.x * 256) {
    double s = 0.0;
    for (int j = 0; j < width; ++j) s += yslots[(long long)g * width + j];
    z_g[g] = s;
    z[pos_g[g]] = s;
  }
}

// Row form: w_I[i] = f_I[i] - Σ_j A_IΓdd[i, j] v[r_col[j]], the entries of row i in ascending local column
__global__ __launch_bounds__(256) void k_nni_coupling(int n_I, const int *__restrict__ r_ptr, const int *__restrict__ r_col,
                                                      const int *__restrict__ r_src, const double *__restrict__ val,
                                                      const double *__restrict__ v, const double *__restrict__ f,
                                                      double *__restrict__ w, const int *done) {
  if (done && *done) return;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_I; i += gridDim.x * 256) {
    double s = 0.0;
    for (int e = r_ptr[i]; e < r_ptr[i + 1]; ++e) s += val[r_src[e]] * v[r_col[e]];
    w[i] = f[i] - s;
  }
}

__global__ __launch_bounds__(256) void k_nni_scatter(int n_I, const int *__restrict__ pos_I, const double *__restrict__ v,
                                                     double *__restrict__ z, const int *done) {
  if (done && *done) return;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n_I; q += gridDim.x * 256) z[pos_I[q]] = v[q];
}

struct NnInducedOp : Operator {
  mi_setup_s *plan;                    // borrowed: the interior solves (its `bound_nni` count refuses mi_schur_setup_destroy while we live)
  std::unique_ptr<DenseBlockOp> nn;    // owned: the ΠS_d blocks (padded row-major, fp64 or fp32), gather maps, cnt, tiles, slots
  int coupling = MI_NNI_AS_WRITTEN;
  int n_I = 0, n_g = 0, nwg = 0;
  int64_t nnz = 0;
  DevBuf<int> pos_I, pos_g, gseg_ptr, seg_ptr, c_row, c_src, r_ptr, r_loc, r_gam, r_src;
  DevBuf<double> val, f_I, y_I, w_I, v_I, r_schur, z_loc, z_g;

  static void check_coupling(int cpl, const char *me) {
    if (cpl != MI_NNI_AS_WRITTEN && cpl != MI_NNI_ASSEMBLED)
      raise(MI_ERR_BAD_ARG, "%s: unknown coupling %d (MI_NNI_AS_WRITTEN = %d, MI_NNI_ASSEMBLED = %d)", me, cpl, MI_NNI_AS_WRITTEN, MI_NNI_ASSEMBLED);
  }

  NnInducedOp(mi_ctx_s *c, int64_t ndom, int64_t n_, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *n_i,
              const int64_t *const *pI, const int64_t *pG, const int64_t *const *gather_idx, const int64_t *node_cnt,
              const int64_t *const *ig_ptr, const int64_t *const *ig_idx, const double *const *ig_val,
              const double *const *PiSd, int storage, mi_setup_s *plan_, int coupling_, int base)
      : Operator(c, n_), plan(plan_), coupling(coupling_) {
    const char *me = "mi_nn_induced_create";
    if (c->n_ranks > 1) raise(MI_ERR_BAD_ARG, "%s: the operator is replicated only; this context is rank %d of %d", me, c->rank, c->n_ranks);
    if (ndom <= 0 || n_ <= 0 || n_ >= INT32_MAX || n_gamma <= 0 || !n_gamma_d || !n_i || !pI || !pG || !gather_idx || !node_cnt ||
        !ig_ptr || !ig_idx || !ig_val || !PiSd || (base != 0 && base != 1))
      raise(MI_ERR_BAD_ARG, "%s: NULL argument, bad size or index_base (ndom = %lld, n = %lld, n_gamma = %lld, index_base = %d)", me,
            (long long)ndom, (long long)n_, (long long)n_gamma, base);
    if (storage != MI_STORE_F64 && storage != MI_STORE_F32)
      raise(MI_ERR_BAD_ARG, "%s: unknown storage %d (MI_STORE_F64 = %d, MI_STORE_F32 = %d)", me, storage, MI_STORE_F64, MI_STORE_F32);
    check_coupling(coupling, me);
    if (!plan || plan->ctx != c) raise(MI_ERR_BAD_ARG, "%s: the set-up plan is NULL or lives on another context", me);
    if (plan->ndom != ndom) raise(MI_ERR_BAD_ARG, "%s: %lld subdomains, the plan has %d", me, (long long)ndom, plan->ndom);
    int64_t tot = 0, totg = 0;
    for (int64_t d = 0; d < ndom; ++d) {
      if (n_i[d] != plan->dom[d].n_i)
        raise(MI_ERR_BAD_ARG, "%s: n_i[%lld] = %lld, the plan's subdomain has %d interior nodes", me, (long long)d, (long long)n_i[d], plan->dom[d].n_i);
      if (n_gamma_d[d] != plan->dom[d].n_g)
        raise(MI_ERR_BAD_ARG, "%s: n_gamma_d[%lld] = %lld, the plan's subdomain has %d interface nodes", me, (long long)d, (long long)n_gamma_d[d], plan->dom[d].n_g);
      tot += n_i[d]; totg += n_gamma_d[d];
    }
    if (!plan->gj || !plan->gj->keep || !plan->gj->have_levels)
      raise(MI_ERR_BAD_ARG, "%s: the plan keeps no level inverses (mi_schur_setup_keep_levels(plan, 1) and a run after it)", me);
    if (tot <= 0 || tot + n_gamma != n_) raise(MI_ERR_BAD_ARG, "%s: n = %lld is not Σ n_i + n_gamma = %lld", me, (long long)n_, (long long)(tot + n_gamma));
    if (totg >= INT32_MAX) raise(MI_ERR_BAD_ARG, "%s: Σ n_gamma_d = %lld is too large", me, (long long)totg);
    n_I = (int)tot; n_g = (int)n_gamma; nwg = (n_g + 255) / 256;
    // the two maps: together a permutation of 0..n-1
    std::vector<int> hI((size_t)n_I), hG((size_t)n_g);
    {
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
    }
    // gather lists: inside [0, n_gamma), unique per subdomain, and cnt[g] = the number of subdomains that hold g
    std::vector<int> mult((size_t)n_g, 0), last((size_t)n_g, -1);
    for (int64_t d = 0; d < ndom; ++d) {
      if (n_gamma_d[d] && !gather_idx[d]) raise(MI_ERR_BAD_ARG, "%s: gather_idx[%lld] is NULL", me, (long long)d);
      for (int64_t l = 0; l < n_gamma_d[d]; ++l) {
        const int64_t g = gather_idx[d][l] - base;
        if (g < 0 || g >= n_gamma)
          raise(MI_ERR_BAD_ARG, "%s: gather_idx[%lld][%lld] = %lld lies outside [%d, %lld)", me, (long long)d, (long long)l, (long long)(g + base), base, (long long)(n_gamma + base));
        if (last[(size_t)g] == (int)d) raise(MI_ERR_BAD_ARG, "%s: gather_idx[%lld] repeats the interface index %lld", me, (long long)d, (long long)(g + base));
        last[(size_t)g] = (int)d;
        ++mult[(size_t)g];
      }
    }
    for (int64_t g = 0; g < n_gamma; ++g)
      if (node_cnt[g] != mult[(size_t)g])
        raise(MI_ERR_BAD_ARG, "%s: node_gamma_cnt[%lld] = %lld, but %d subdomain(s) hold that interface node in their gather_idx", me, (long long)g,
              (long long)node_cnt[g], mult[(size_t)g]);
    // the stacked A_IΓdd (LOCAL columns): values in the caller's concatenated CSC order, a column form (per Γ node, the
    // subdomains that hold it in ascending order, each one's column in stored order) and a row form (ascending local
    // column) that point into them
    std::vector<int64_t> voff((size_t)ndom + 1, 0), ioff((size_t)ndom + 1, 0), goff((size_t)ndom + 1, 0);
    for (int64_t d = 0; d < ndom; ++d) {
      if (!ig_ptr[d]) raise(MI_ERR_BAD_ARG, "%s: ig_colptr[%lld] is NULL", me, (long long)d);
      if (ig_ptr[d][0] != base) raise(MI_ERR_BAD_ARG, "%s: ig_colptr[%lld][0] = %lld is not index_base = %d", me, (long long)d, (long long)ig_ptr[d][0], base);
      for (int64_t j = 0; j < n_gamma_d[d]; ++j)
        if (ig_ptr[d][j + 1] < ig_ptr[d][j]) raise(MI_ERR_BAD_ARG, "%s: ig_colptr[%lld] decreases at column %lld", me, (long long)d, (long long)j);
      const int64_t nz = ig_ptr[d][n_gamma_d[d]] - base;
      if (nz && (!ig_idx[d] || !ig_val[d])) raise(MI_ERR_BAD_ARG, "%s: ig_rowval / ig_nzval [%lld] is NULL", me, (long long)d);
      voff[d + 1] = voff[d] + nz; ioff[d + 1] = ioff[d] + n_i[d]; goff[d + 1] = goff[d] + n_gamma_d[d];
      if (voff[d + 1] >= INT32_MAX) raise(MI_ERR_BAD_ARG, "%s: more than 2^31 stored entries", me);
      for (int64_t k = 0; k < nz; ++k) {
        const int64_t r = ig_idx[d][k] - base;
        if (r < 0 || r >= n_i[d]) raise(MI_ERR_BAD_ARG, "%s: ig_rowval[%lld] holds row %lld out of range (n_i = %lld)", me, (long long)d, (long long)(r + base), (long long)n_i[d]);
      }
    }
    nnz = voff[ndom];
    // holders of every Γ node: (subdomain, local column), subdomain ascending
    std::vector<int> hp((size_t)n_g + 1, 0);
    for (int g = 0; g < n_g; ++g) hp[g + 1] = hp[g] + mult[g];
    std::vector<int> hd((size_t)totg), hl((size_t)totg), fillh(hp.begin(), hp.end() - 1);
    for (int64_t d = 0; d < ndom; ++d)
      for (int64_t l = 0; l < n_gamma_d[d]; ++l) { const int at = fillh[(size_t)(gather_idx[d][l] - base)]++; hd[at] = (int)d; hl[at] = (int)l; }
    std::vector<int> gp((size_t)n_g + 1), sp, cr((size_t)nnz), cs((size_t)nnz), rp((size_t)n_I + 1, 0), rl((size_t)nnz), rg((size_t)nnz), rs((size_t)nnz);
    std::vector<double> hv((size_t)nnz);
    size_t e = 0;
    for (int g = 0; g < n_g; ++g) {
      gp[g] = (int)sp.size();
      for (int h = hp[g]; h < hp[g + 1]; ++h) {
        const int d = hd[h], l = hl[h];
        const int64_t a = ig_ptr[d][l] - base, b = ig_ptr[d][l + 1] - base;
        if (a == b) continue;      // an empty column subtracts +0: nothing changes
        sp.push_back((int)e);
        for (int64_t k = a; k < b; ++k, ++e) { cr[e] = (int)(ioff[d] + (ig_idx[d][k] - base)); cs[e] = (int)(voff[d] + k); }
      }
    }
    gp[n_g] = (int)sp.size();
    sp.push_back((int)e);
    for (int64_t d = 0; d < ndom; ++d)
      for (int64_t k = 0; k < voff[d + 1] - voff[d]; ++k) ++rp[(size_t)(ioff[d] + (ig_idx[d][k] - base)) + 1];
    for (int i = 0; i < n_I; ++i) rp[i + 1] += rp[i];
    {   // rows: a subdomain's columns in ascending local order, so each row fills in ascending local column
      std::vector<int> fill(rp.begin(), rp.end() - 1);
      for (int64_t d = 0; d < ndom; ++d)
        for (int64_t j = 0; j < n_gamma_d[d]; ++j)
          for (int64_t k = ig_ptr[d][j] - base; k < ig_ptr[d][j + 1] - base; ++k) {
            const int at = fill[(size_t)(ioff[d] + (ig_idx[d][k] - base))]++;
            rl[at] = (int)(goff[d] + j); rg[at] = (int)(gather_idx[d][j] - base); rs[at] = (int)(voff[d] + k);
          }
    }
    for (int64_t d = 0; d < ndom; ++d)
      if (voff[d + 1] > voff[d]) std::memcpy(hv.data() + voff[d], ig_val[d], sizeof(double) * (size_t)(voff[d + 1] - voff[d]));
    // the ΠS_d blocks and everything the GEMV needs: a replicated Neumann-Neumann operator of all subdomains
    nn.reset(new DenseBlockOp(c, ndom, n_gamma, n_gamma_d, gather_idx, PiSd, node_cnt, base, 0, ndom, storage));
    hipStream_t s = c->stream;
    auto up = [&](DevBuf<int> &dst, const std::vector<int> &h) { dst.upload(h.empty() ? std::vector<int>{0} : h, s); };
    up(pos_I, hI); up(pos_g, hG); up(gseg_ptr, gp); up(seg_ptr, sp); up(c_row, cr); up(c_src, cs);
    up(r_ptr, rp); up(r_loc, rl); up(r_gam, rg); up(r_src, rs);
    val.upload(hv.empty() ? std::vector<double>{0.0} : hv, s);
    f_I.alloc((size_t)n_I); y_I.alloc((size_t)n_I); w_I.alloc((size_t)n_I); v_I.alloc((size_t)n_I);
    r_schur.alloc((size_t)n_g); z_g.alloc((size_t)n_g); z_loc.alloc((size_t)totg + 1);
    MI_HIP(hipStreamSynchronize(s));
    ++plan->bound_nni;   // last: nothing above may leave a count behind
  }
  ~NnInducedOp() override { --plan->bound_nni; }

  // new A_IΓdd values (device pointer, the concatenated CSC order of create): one copy
  void set_values(const double *v) {
    if (nnz) MI_HIP(hipMemcpyAsync(val.p, v, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, ctx->stream));
  }

  void level_solve(const double *f, double *u) {
    if (!plan->gj || !plan->gj->keep || !plan->gj->have_levels)
      raise(MI_ERR_BAD_ARG, "mi_nn_induced: the plan keeps no level inverses any more (mi_schur_setup_keep_levels(plan, 1) and a run after it)");
    gj_level_enqueue(*plan, ctx->stream, f, u);
  }
  void gemv(const double *x, const int *done) {
    if (!nn->ntiles) return;
    const int nt = nn->ntiles, rpw = nn->rpw, waves = nn->waves;
    const DenseMeta &meta = nn->meta;
    double *ys = nn->yslots.p, *zl = z_loc.p;
    hipStream_t s = ctx->stream;
#define MI_NNI(R, V, T) hipLaunchKernelGGL((k_gemv_nni<R, V, T>), dim3(nt), dim3(64 * V), 0, s, meta, x, ys, zl, done)
#define MI_NNI_R(V, T) do { if (rpw == 1) MI_NNI(1, V, T); else if (rpw == 2) MI_NNI(2, V, T); else MI_NNI(4, V, T); } while (0)
#define MI_NNI_V(T) do { if (waves == 16) MI_NNI_R(16, T); else if (waves == 8) MI_NNI_R(8, T); else MI_NNI_R(4, T); } while (0)
    if (nn->f32()) MI_NNI_V(float); else MI_NNI_V(double);
#undef MI_NNI_V
#undef MI_NNI_R
#undef MI_NNI
  }
  static int grid(int n) { return std::max(1, std::min((n + 255) / 256, 4096)); }
  void apply(const double *x, double *u, const int *done) override {
    hipStream_t s = ctx->stream;
    const bool asm_form = coupling == MI_NNI_ASSEMBLED;
    hipLaunchKernelGGL(k_lo_gather, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, x, f_I.p, done);
    level_solve(f_I.p, y_I.p);
    hipLaunchKernelGGL(k_lo_zgamma, dim3(nwg), dim3(256), 0, s, n_g, 0, nwg, (const int *)pos_g.p, (const int *)gseg_ptr.p,
                       (const int *)seg_ptr.p, (const int *)c_row.p, (const int *)c_src.p, (const double *)val.p, x,
                       (const double *)y_I.p, (const double *)nullptr, r_schur.p, (double *)nullptr, done);
    gemv(r_schur.p, done);
    hipLaunchKernelGGL(k_nni_assemble, dim3(grid(n_g)), dim3(256), 0, s, n_g, nn->maps.slot_width, (const double *)nn->yslots.p,
                       (const int *)pos_g.p, z_g.p, u, done);
    hipLaunchKernelGGL(k_nni_coupling, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)r_ptr.p,
                       (const int *)(asm_form ? r_gam.p : r_loc.p), (const int *)r_src.p, (const double *)val.p,
                       (const double *)(asm_form ? z_g.p : z_loc.p), (const double *)f_I.p, w_I.p, done);
    level_solve(w_I.p, v_I.p);
    hipLaunchKernelGGL(k_nni_scatter, dim3(grid(n_I)), dim3(256), 0, s, n_I, (const int *)pos_I.p, (const double *)v_I.p, u, done);
    MI_HIP(hipGetLastError());
  }
  bool writes_y_once() const override { return false; }   // z is written by two launches (5 and 8)
  // bytes: one level solve streams the kept inverses once (the dominant figure; its vectors ride along); the apply is two
  // of them, the ΠS_d GEMV (blocks, maps, cnt: the Neumann-Neumann operator's own count, plus the second output), and the
  // glue: both forms of A_IΓdd (value, source index and row / column index per entry), their pointers, and the vectors of
  // launches 1, 3, 5, 6 and 8
  void bytes(int64_t *a, int64_t *d) const override {
    const int64_t lv = 8 * ((int64_t)(plan->gj ? plan->gj->zstore.n : 0) + 4 * (int64_t)n_I);
    int64_t na = 0, nd = 0;
    nn->bytes(&na, &nd);
    const int64_t nloc = nn->maps.nloc;
    const int64_t glue = 2 * 16 * nnz + 4 * ((int64_t)n_I + 2 * n_g) + 8 * nloc + 8 * (int64_t)nn->maps.slot_width * n_g +
                         (8 + 4) * 2 * ((int64_t)n_I + n_g) + 8 * (5 * (int64_t)n_I + 3 * (int64_t)n_g);
    *d = lv;
    *a = 2 * lv + na + glue;
  }
  void apply_dominant(const double *x) override {
    hipLaunchKernelGGL(k_lo_gather, dim3(grid(n_I)), dim3(256), 0, ctx->stream, n_I, (const int *)pos_I.p, x, f_I.p, (const int *)nullptr);
    level_solve(f_I.p, y_I.p);
  }
};

}  // namespace mi
