// The spectral pseudo-inverse ΠS_d = pinv(S_d, rtol = sqrt(eps)) of `prepare_neumann_neumann_schur_precond(Sd, ...)`
// (EPDD.jl:1201-1220): S_d = V diag(lam) V' by rocSOLVER's dsyevd, the filter on the singular values |lam|
// as a kernel of this file, ΠS_d = (V filtered) V' by rocBLAS' dgemm. The two libraries are bound with dlopen like RCCL.
// This is the FALLBACK of pinv_blocks_fast (setup_gj.hpp), which inverts well-conditioned and floating blocks with the
// Gauss-Jordan kernels: only the blocks that fail its certificates come here (counted in MI_QUERY_SPECTRAL_PINV), or all
// of them with MI355_PINV_EIG=1.
#pragma once
#include <dlfcn.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <cmath>

#include "operators.hpp"

namespace mi {

struct RocLa {
  void *hb = nullptr, *hs = nullptr;
  rocblas_status (*create_handle)(rocblas_handle *) = nullptr;
  rocblas_status (*destroy_handle)(rocblas_handle) = nullptr;
  rocblas_status (*set_stream)(rocblas_handle, hipStream_t) = nullptr;
  rocblas_status (*dgemm)(rocblas_handle, rocblas_operation, rocblas_operation, rocblas_int, rocblas_int, rocblas_int, const double *,
                          const double *, rocblas_int, const double *, rocblas_int, const double *, double *, rocblas_int) = nullptr;
  rocblas_status (*dsyevd)(rocblas_handle, const rocblas_evect, const rocblas_fill, const rocblas_int, double *, const rocblas_int,
                           double *, double *, rocblas_int *) = nullptr;
  static RocLa &get() {
    static RocLa r;
    static bool tried = false;
    if (!tried) {
      tried = true;
      // By SONAME, never by path: when a framework in the process has already loaded its own rocBLAS / rocSOLVER pair
      // (torch ships one with the same SONAMEs), that pair is reused — a second rocBLAS copy would be bound to the first
      // one's rocSOLVER and would page in another 0.6 GB of kernel libraries; otherwise the system pair is loaded.
      const char *nb[] = {"librocblas.so.5", "librocblas.so"};
      const char *ns[] = {"librocsolver.so.0", "librocsolver.so"};
      for (const char *n : nb) if ((r.hb = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
      if (!r.hb) for (const char *n : nb) if ((r.hb = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
      for (const char *n : ns) if ((r.hs = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
      if (!r.hs) for (const char *n : ns) if ((r.hs = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
      if (r.hb && r.hs) {
#define MI_SYM(h, field, name) r.field = (decltype(r.field))dlsym(h, name)
        MI_SYM(r.hb, create_handle, "rocblas_create_handle"); MI_SYM(r.hb, destroy_handle, "rocblas_destroy_handle");
        MI_SYM(r.hb, set_stream, "rocblas_set_stream"); MI_SYM(r.hb, dgemm, "rocblas_dgemm");
        MI_SYM(r.hs, dsyevd, "rocsolver_dsyevd");
#undef MI_SYM
      }
    }
    if (!r.create_handle || !r.destroy_handle || !r.set_stream || !r.dgemm || !r.dsyevd)
      raise(MI_ERR_HIP, "rocBLAS / rocSOLVER could not be loaded: %s", dlerror() ? dlerror() : "missing symbols");
    return r;
  }
};
#define MI_ROC(expr)                                                                                       \
  do {                                                                                                     \
    rocblas_status s_ = (expr);                                                                            \
    if (s_ != rocblas_status_success) ::mi::raise(MI_ERR_HIP, "%s failed with rocblas_status %d", #expr, (int)s_); \
  } while (0)

// B[:, j] = V[:, j] * (|lam_j| > tol ? 1 / lam_j : 0), tol = rtol * max_k |lam_k|  (pinv's filter on singular values |lam|)
__global__ __launch_bounds__(NT) void k_pinv_scale(int n, const double *__restrict__ V, const double *__restrict__ lam, double rtol,
                                                   double *__restrict__ B) {
  const double tol = rtol * fmax(fabs(lam[0]), fabs(lam[n - 1]));   // syevd returns the eigenvalues in ascending order
  const long long tot = (long long)n * n;
  for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < tot; e += (long long)gridDim.x * NT) {
    const double l = lam[e / n];
    B[e] = fabs(l) > tol ? V[e] / l : 0.0;
  }
}

// ΠS_d = pinv(S_d, rtol) for the concatenated symmetric blocks (device pointers): S = V diag(lam) V', singular values |lam|.
inline void pinv_blocks(mi_ctx_s *c, int ndom, const int64_t *n_gamma_d, const double *Sd, double rtol, double *Pi) {
  RocLa &la = RocLa::get();
  rocblas_handle h = nullptr;
  MI_ROC(la.create_handle(&h));
  struct Guard { RocLa &la; rocblas_handle h; ~Guard() { (void)la.destroy_handle(h); } } guard{la, h};
  MI_ROC(la.set_stream(h, c->stream));
  size_t nmax = 1;
  for (int d = 0; d < ndom; ++d) nmax = std::max<size_t>(nmax, (size_t)n_gamma_d[d]);
  DevBuf<double> V(nmax * nmax), B(nmax * nmax), lam(nmax), E(nmax);
  DevBuf<int> info(1);
  const double one = 1.0, zero = 0.0;
  size_t off = 0;
  std::vector<int> infos(ndom, 0);
  for (int d = 0; d < ndom; ++d) {
    const int n = (int)n_gamma_d[d];
    if (n == 0) continue;
    MI_HIP(hipMemcpyAsync(V.p, Sd + off, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, c->stream));
    MI_ROC(la.dsyevd(h, rocblas_evect_original, rocblas_fill_upper, n, V.p, n, lam.p, E.p, info.p));
    hipLaunchKernelGGL(k_pinv_scale, dim3(grid_for((long long)n * n)), dim3(NT), 0, c->stream, n, V.p, lam.p, rtol, B.p);
    MI_HIP(hipGetLastError());
    MI_ROC(la.dgemm(h, rocblas_operation_none, rocblas_operation_transpose, n, n, n, &one, B.p, n, V.p, n, &zero, Pi + off, n));
    MI_HIP(hipMemcpyAsync(&infos[d], info.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    off += (size_t)n * n;
  }
  MI_HIP(hipStreamSynchronize(c->stream));
  for (int d = 0; d < ndom; ++d)
    if (infos[d] != 0) raise(MI_ERR_HIP, "pinv: the symmetric eigensolver did not converge on block %d (info = %d)", d, infos[d]);
}

}  // namespace mi
