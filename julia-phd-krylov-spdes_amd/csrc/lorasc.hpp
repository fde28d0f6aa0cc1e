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
//   6 k_split_coupling  w_I = A_IΓd x_Γ: per interior row, ascending Γ column from 0 — the bits of Julia's CSC product (:1960)
//   7 level solve    v_I = A_IId \ w_I
//   8 k_lo_finish    u[pos_I] = y_I - v_I                                                       (:1960, 1964-1968)
// Launches 1 - 3 and 6 - 8, the index arrays and the interior vectors are SplitOp's (full_split.hpp), in the identity form
// of full_split_plan.hpp; 4 and 5 are this operator's own.
//
// The quirk of :1954-1957: the loop runs `for (k, σ) in enumerate(Σ)` and never uses σ, although prepare_lorasc_precond
// stores Σ[k] = (ε - σ)/σ (:1596) and leaves E[k] A_ΓΓ-orthonormal — the paper's correction would be Σ_k Σ[k] (E_k'z) E_k.
// coef == NULL (ones) is the reference as written; the paper's form is coef = Σ.
#pragma once
#include "full_split.hpp"

namespace mi {

constexpr int LO_MAX_NEV = 1024;   // t_k of k_lo_correct: 8 KiB of LDS

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

struct LorascOp : SplitOp {
  mi_op_s *gg_h;         // borrowed: the A_ΓΓ solver's handle (`bound` refuses mi_op_destroy); the plan's `bound` counts us too
  SpdDirectOp *gg;
  int nev = 0;
  DevBuf<double> E, coef, part, z_g, x_g;

  LorascOp(mi_ctx_s *c, int64_t ndom, int64_t n_, int64_t n_gamma, const int64_t *n_i, const int64_t *const *pI,
           const int64_t *pG, const int64_t *const *ig_ptr, const int64_t *const *ig_idx, const double *const *ig_val,
           mi_setup_s *plan_, mi_op_s *gg_h_, int64_t nev_, const double *E_, const double *coef_, int base)
      : SplitOp(c, n_, plan_, "mi_lorasc"), gg_h(gg_h_), gg(nullptr) {
    const char *me = "mi_lorasc_create";
    split::Input in;     // identity form: the columns of A_IΓd are the Γ nodes
    in.ndom = ndom; in.n = n_; in.n_gamma = n_gamma; in.base = base; in.n_i = n_i; in.pos_I = pI; in.pos_g = pG;
    in.colptr = ig_ptr; in.rowval = ig_idx; in.nzval = ig_val;
    check_args(me, in, true);
    gg = gg_h && gg_h->impl ? dynamic_cast<SpdDirectOp *>(gg_h->impl.get()) : nullptr;
    if (!gg || gg->ctx != c) raise(MI_ERR_BAD_ARG, "%s: a_gg_solver is not a sparse direct operator (mi_spd_direct_create) of this context", me);
    if (gg->n != n_gamma) raise(MI_ERR_BAD_ARG, "%s: a_gg_solver has size %lld, n_gamma is %lld", me, (long long)gg->n, (long long)n_gamma);
    build(me, in);
    z_g.alloc((size_t)n_g); x_g.alloc((size_t)n_g);
    set_correction_host(nev_, E_, coef_, me);
    MI_HIP(hipStreamSynchronize(c->stream));
    ++plan->bound; ++gg_h->bound;   // last: nothing above may leave a count behind
  }
  ~LorascOp() override { --plan->bound; --gg_h->bound; }
  bool uses(const Operator *o) const override { return o == this || gg->uses(o); }
  bool usable(std::string &why) const override { return gg->usable(why); }

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
  void apply(const double *x, double *u, const int *done) override {
    interior_to_gamma(x, nev, E.p, z_g.p, part.p, done);
    gg->apply(z_g.p, x_g.p, done);
    hipLaunchKernelGGL(k_lo_correct, dim3(nwg), dim3(256), 0, ctx->stream, n_g, nev, nwg, (const int *)pos_g.p, (const double *)E.p,
                       (const double *)coef.p, (const double *)part.p, x_g.p, u, done);
    gamma_to_interior(r_gam.p, x_g.p, nullptr, y_I.p, u, done);
  }
  // bytes: two level solves, the A_ΓΓ solve, the split's glue, E twice, the partials, and the vectors of launches 1, 3, 5, 6 and 8
  void bytes(int64_t *a, int64_t *d) const override {
    int64_t ga = 0, gd = 0;
    gg->bytes(&ga, &gd);
    *d = level_bytes();
    *a = 2 * level_bytes() + ga + split_bytes() + 2 * 8 * (int64_t)nev * n_g + 8 * (int64_t)nev * nwg * (1 + nwg) +
         8 * (4 * (int64_t)n_I + 5 * (int64_t)n_g);
  }
};

}  // namespace mi
