// How long does the 64 x 64 pivot-block inversion of csrc/setup_gj.hpp take inside a kernel? (wall_clock64 stamps, 100 MHz;
// one workgroup of 256 threads, as in k_gj_pivot / the look-ahead tile of k_gj_update)
#include <hip/hip_runtime.h>
#include "../../julia-phd-krylov-spdes_amd/csrc/setup_gj.hpp"
#include "../../julia-phd-krylov-spdes_amd/csrc/pinv_spectral.hpp"
#include <cstdio>
using namespace mi;
__global__ __launch_bounds__(256) void k_probe(const double *A, double *out, long long *stamps) {
  constexpr int LD = GJ_B + 1;
  __shared__ double Mb[GJ_B * LD];
  __shared__ double Wb[GJ_SCRATCH];
  for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256) Mb[(e % GJ_B) * LD + e / GJ_B] = A[e];
  __syncthreads();
  long long t0 = wall_clock64();
  gj_invert_block64(Mb, LD, Wb, true);
  long long t1 = wall_clock64();
  for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256) out[e] = Mb[(e % GJ_B) * LD + e / GJ_B];
  if (threadIdx.x == 0) stamps[0] = t1 - t0;
}
int main() {
  const int n = GJ_B;
  std::vector<double> h(n * n);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) h[i + j * n] = (i == j ? 4.0 + 0.01 * i : 1.0 / (1.0 + abs(i - j)));
  double *A, *out; long long *st;
  hipMalloc(&A, n * n * 8); hipMalloc(&out, n * n * 8); hipMalloc(&st, 64);
  hipMemcpy(A, h.data(), n * n * 8, hipMemcpyHostToDevice);
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(k_probe, dim3(1), dim3(256), 0, 0, A, out, st);
    hipDeviceSynchronize();
    long long s; hipMemcpy(&s, st, 8, hipMemcpyDeviceToHost);
    printf("gj_invert_block64 (64 x 64): %.2f us\n", s / 100.0);
  }
  std::vector<double> o(n * n); hipMemcpy(o.data(), out, n * n * 8, hipMemcpyDeviceToHost);
  double err = 0;   // A * inv - I
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = 0; for (int k = 0; k < n; ++k) s += h[i + k * n] * o[k + j * n]; err = fmax(err, fabs(s - (i == j))); }
  printf("max |A inv(A) - I| = %.2e\n", err);
  return 0;
}
