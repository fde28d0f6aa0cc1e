// Karhunen-Loève operators on the matrix-free covariance kernel (cov_kernels.hpp).
// The reference assembles C[i, j] = ∫∫ ϕ_i(P) cov(P, P') ϕ_j(P') dense, by two element loops (do_mass_covariance_assembly,
// Fem/KarhunenLoeve.jl:27-108; the local form Fem/KarhunenLoeveDomainDecomposition.jl:120-204): the first builds
// R[i, j] = Σ_el (2 cov(p_r, p_j) + cov(p_s, p_j) + cov(p_t, p_j)) Area / 12 = (M K)[i, j] — the element mass matrix is
// Area / 12 [2 1 1; 1 2 1; 1 1 2] — and the second C[i, j] = Σ_el (2 R[i, j] + R[i, k] + R[i, ℓ]) Area / 12 = (R M)[i, j].
// So C = M K M with K[i, j] = cov(p_i, p_j), and C x is SpMV, covariance launch, SpMV: nothing of size n² exists.
#pragma once
#include "cov_kernels.hpp"
#include "operators.hpp"

namespace mi {

inline void cov_check_model(const char *me, int model, double sig2, double L) {
  if (model != MI_COV_SEXP && model != MI_COV_EXP) raise(MI_ERR_BAD_ARG, "%s: model = %d is neither MI_COV_SEXP nor MI_COV_EXP", me, model);
  if (!std::isfinite(sig2) || !std::isfinite(L)) raise(MI_ERR_BAD_ARG, "%s: sig2 = %g, L = %g: both must be finite", me, sig2, L);
  if (!(L > 0.0) || sig2 < 0.0) raise(MI_ERR_BAD_ARG, "%s: sig2 = %g, L = %g: L > 0 and sig2 >= 0 expected", me, sig2, L);
}
inline void cov_check_points(const char *me, const char *what, const double *p, int64_t n) {
  for (int64_t k = 0; k < 2 * n; ++k)
    if (!std::isfinite(p[k])) raise(MI_ERR_BAD_ARG, "%s: %s holds %g at node %lld (not finite)", me, what, p[k], (long long)(k / 2));
}

struct KlCovOp : Operator {
  int model;
  double sig2, L;
  CsrDev M;
  DevBuf<double> pts, t1, t2, work, sink;
  DevBuf<double> T1, T2;   // panels of COV_CB columns for apply_multi
  long long ld;

  KlCovOp(mi_ctx_s *c, int model_, double sig2_, double L_, int64_t n_, const double *points, const HostCsr &hm)
      : Operator(c, n_), model(model_), sig2(sig2_), L(L_), ld((long long)n_) {
    hipStream_t s = c->stream;
    M.upload(hm, s);
    pts.upload(points, 2 * (size_t)n, s);
    MI_HIP(hipStreamSynchronize(s));
    t1.alloc((size_t)n + 1); t2.alloc((size_t)n + 1); sink.alloc((size_t)n + 1);
    T1.alloc((size_t)ld * COV_CB); T2.alloc((size_t)ld * COV_CB);
    work.alloc(std::max<size_t>(1, std::max(cov_workspace(n, n, 1), cov_workspace(n, n, COV_CB))));
  }
  void cov(int m, const double *X, double *Y, const int *done) {
    cov_launch(ctx->stream, model, sig2, L, (int)n, pts.p, (int)n, pts.p, m, X, ld, Y, ld, work.p, done);
    MI_HIP(hipGetLastError());
  }
  void apply(const double *x, double *y, const int *done) override {
    hipStream_t s = ctx->stream;
    M.launch(0, x, nullptr, t1.p, done, s);
    cov(1, t1.p, t2.p, done);
    M.launch(0, t2.p, nullptr, y, done, s);
  }
  // panels of COV_CB columns: one exp per (i, j) feeds the whole panel
  void apply_multi(const double *X, int64_t ldx, int k, double *Y, int64_t ldy) override {
    hipStream_t s = ctx->stream;
    for (int v0 = 0; v0 < k; v0 += COV_CB) {
      const int w = std::min(COV_CB, k - v0);
      for (int v = 0; v < w; ++v) M.launch(0, X + (size_t)(v0 + v) * ldx, nullptr, T1.p + (size_t)v * ld, nullptr, s);
      cov(w, T1.p, T2.p, nullptr);   // w <= COV_CB columns are one column block: the splits, and so the workspace, of COV_CB at most
      for (int v = 0; v < w; ++v) M.launch(0, T2.p + (size_t)v * ld, nullptr, Y + (size_t)(v0 + v) * ldy, nullptr, s);
    }
  }
  // Bytes: the covariance launch reads the points twice and one vector, writes one (it is compute bound: n² exp); the two
  // SpMVs as CsrDev counts them.
  void bytes(int64_t *a, int64_t *d) const override { *d = 48 * n; *a = *d + 2 * M.bytes(); }
  void apply_dominant(const double *x) override { cov(1, x, sink.p, nullptr); }
};

}  // namespace mi
