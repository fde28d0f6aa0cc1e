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
//   6 k_split_coupling  w_I = f_I - A_IΓdd v: per interior row, ascending local column from 0 — the bits of Julia's CSC
//                     product and the broadcast of :2411
//   7 level solve     v_I = A_IId \ w_I                                                           (:2412)
//   8 k_nni_scatter   z[pos_I] = v_I                                                              (:2413-2415)
// Launches 1 - 3 and 6 - 8, the index arrays and the interior vectors are SplitOp's (full_split.hpp), in the gathered form
// of full_split_plan.hpp; 4 and 5 are this operator's own.
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

struct NnInducedOp : SplitOp {
  std::unique_ptr<DenseBlockOp> nn;    // owned: the ΠS_d blocks (padded row-major, fp64 or fp32), gather maps, cnt, tiles, slots
  int coupling = MI_NNI_AS_WRITTEN;
  DevBuf<double> r_schur, z_loc, z_g;  // the plan's `bound_nni` count refuses mi_schur_setup_destroy while we live

  static void check_coupling(int cpl, const char *me) {
    if (cpl != MI_NNI_AS_WRITTEN && cpl != MI_NNI_ASSEMBLED)
      raise(MI_ERR_BAD_ARG, "%s: unknown coupling %d (MI_NNI_AS_WRITTEN = %d, MI_NNI_ASSEMBLED = %d)", me, cpl, MI_NNI_AS_WRITTEN, MI_NNI_ASSEMBLED);
  }

  NnInducedOp(mi_ctx_s *c, int64_t ndom, int64_t n_, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *n_i,
              const int64_t *const *pI, const int64_t *pG, const int64_t *const *gather_idx, const int64_t *node_cnt,
              const int64_t *const *ig_ptr, const int64_t *const *ig_idx, const double *const *ig_val,
              const double *const *PiSd, int storage, mi_setup_s *plan_, int coupling_, int base)
      : SplitOp(c, n_, plan_, "mi_nn_induced"), coupling(coupling_) {
    const char *me = "mi_nn_induced_create";
    split::Input in;     // gathered form: column j of A_IΓdd[d] is the Γ node gather_idx[d][j]
    in.ndom = ndom; in.n = n_; in.n_gamma = n_gamma; in.base = base; in.n_i = n_i; in.pos_I = pI; in.pos_g = pG;
    in.colptr = ig_ptr; in.rowval = ig_idx; in.nzval = ig_val; in.n_gamma_d = n_gamma_d; in.gather = gather_idx; in.node_cnt = node_cnt;
    check_args(me, in, n_gamma_d && gather_idx && node_cnt && PiSd);
    if (storage != MI_STORE_F64 && storage != MI_STORE_F32)
      raise(MI_ERR_BAD_ARG, "%s: unknown storage %d (MI_STORE_F64 = %d, MI_STORE_F32 = %d)", me, storage, MI_STORE_F64, MI_STORE_F32);
    check_coupling(coupling, me);
    build(me, in);
    // the ΠS_d blocks and everything the GEMV needs: a replicated Neumann-Neumann operator of all subdomains
    nn.reset(new DenseBlockOp(c, ndom, n_gamma, n_gamma_d, gather_idx, PiSd, node_cnt, base, 0, ndom, storage));
    r_schur.alloc((size_t)n_g); z_g.alloc((size_t)n_g); z_loc.alloc((size_t)totg + 1);
    MI_HIP(hipStreamSynchronize(c->stream));
    ++plan->bound_nni;   // last: nothing above may leave a count behind
  }
  ~NnInducedOp() override { --plan->bound_nni; }

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
  void apply(const double *x, double *u, const int *done) override {
    const bool asm_form = coupling == MI_NNI_ASSEMBLED;
    interior_to_gamma(x, 0, nullptr, r_schur.p, nullptr, done);
    gemv(r_schur.p, done);
    hipLaunchKernelGGL(k_nni_assemble, dim3(grid(n_g)), dim3(256), 0, ctx->stream, n_g, nn->maps.slot_width, (const double *)nn->yslots.p,
                       (const int *)pos_g.p, z_g.p, u, done);
    gamma_to_interior(asm_form ? r_gam.p : r_loc.p, asm_form ? z_g.p : z_loc.p, f_I.p, nullptr, u, done);
  }
  // bytes: two level solves, the ΠS_d GEMV (blocks, maps, cnt: the Neumann-Neumann operator's own count, plus the second
  // output), the split's glue, the slots, and the vectors of launches 1, 3, 5, 6 and 8
  void bytes(int64_t *a, int64_t *d) const override {
    int64_t na = 0, nd = 0;
    nn->bytes(&na, &nd);
    *d = level_bytes();
    *a = 2 * level_bytes() + na + split_bytes() + 8 * (int64_t)nn->maps.nloc + 8 * (int64_t)nn->maps.slot_width * n_g +
         8 * (5 * (int64_t)n_I + 3 * (int64_t)n_g);
  }
};

}  // namespace mi
