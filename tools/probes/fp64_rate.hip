// The fp64 vector rate a plain loop reaches: every thread keeps 32 independent accumulators and, per step, forms
// t = x - c, acc = acc + t * t for each of them (the three operations of the quantizer's distance, csrc/vq.hpp, without its
// LDS reads). Built like the library (-O3 -ffp-contract=off): a product and a sum stay two instructions. Prints one JSON line.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); exit(2); } } while (0)
constexpr int ACC = 32;
__global__ __launch_bounds__(256) void k_rate(int steps, const double *__restrict__ in, double *__restrict__ out) {
  double acc[ACC], x[4], c[8];
  const int t = blockIdx.x * 256 + threadIdx.x;
  for (int i = 0; i < 4; ++i) x[i] = in[(t + i) & 1023];
  for (int j = 0; j < 8; ++j) c[j] = in[(t + 7 * j + 5) & 1023];
  for (int a = 0; a < ACC; ++a) acc[a] = 0.0;
  for (int s = 0; s < steps; ++s) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double df = x[i] - c[j];
        acc[i * 8 + j] = acc[i * 8 + j] + df * df;
      }
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = c[j] + 0.5;   // the operands change: nothing is hoisted out of the loop (8 more additions)
  }
  double sum = 0.0;
  for (int a = 0; a < ACC; ++a) sum += acc[a];
  out[t] = sum;
}
int main(int argc, char **argv) {
  const int steps = argc > 1 ? atoi(argv[1]) : 4096, blocks = 256 * 12, reps = 5;
  double *in, *out;
  CK(hipMalloc(&in, 1024 * 8)); CK(hipMalloc(&out, (size_t)blocks * 256 * 8));
  double h[1024];
  for (int i = 0; i < 1024; ++i) h[i] = 0.001 * i;
  CK(hipMemcpy(in, h, sizeof h, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(k_rate, dim3(blocks), dim3(256), 0, 0, steps, in, out);
  CK(hipDeviceSynchronize());
  double best = 0.0, mean = 0.0;
  for (int r = 0; r < reps; ++r) {
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_rate, dim3(blocks), dim3(256), 0, 0, steps, in, out);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    const double ops = (3.0 * ACC + 8.0) * steps * (double)blocks * 256 / (ms * 1e-3);
    mean += ops / reps; if (ops > best) best = ops;
  }
  printf("{\"fp64_ops_per_s_mean\": %.4e, \"fp64_ops_per_s_best\": %.4e, \"steps\": %d, \"threads\": %d, \"repeats\": %d}\n", mean, best, steps, blocks * 256, reps);
  return 0;
}
