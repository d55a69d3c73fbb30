// The relative error of expf -- what hipcc makes of it for gfx950 without fast-math, the function the top-p block selection
// calls (csrc/usp_block_select_top_p.hip) -- against the fp64 exp, over EVERY fp32 argument in [-126 ln 2, 0].  Prints the
// largest relative error and where it falls.  tests/block_select_top_p_ref.py takes twice the printed value as its bound.
//   hipcc --offload-arch=gfx950 -O3 tools/expf_error.hip -o expf_error && ./expf_error
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// arguments: the floats -0.f .. lo as the integers 0x80000000 + i, i in [0, count)
__global__ void expf_error_kernel(uint32_t count, double* worst, float* where) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, n = gridDim.x * blockDim.x;
  double w = 0.0;
  float at = 0.f;
  for (uint32_t i = t; i < count; i += n) {
    const uint32_t bits = 0x80000000u + i;
    float x;
    memcpy(&x, &bits, 4);
    const double want = exp((double)x);
    const double err = fabs((double)expf(x) - want) / want;
    if (err > w) { w = err; at = x; }
  }
  worst[t] = w;
  where[t] = at;
}

int main() {
  const float lo = -126.f * 0.693147180559945309f;
  uint32_t lo_bits;
  memcpy(&lo_bits, &lo, 4);
  const uint32_t count = lo_bits - 0x80000000u + 1u;
  const int blocks = 2048, threads = 256, n = blocks * threads;
  double* worst;
  float* where;
  if (hipMalloc(&worst, n * sizeof(double)) != hipSuccess || hipMalloc(&where, n * sizeof(float)) != hipSuccess) return 1;
  hipLaunchKernelGGL(expf_error_kernel, dim3(blocks), dim3(threads), 0, 0, count, worst, where);
  std::vector<double> w(n);
  std::vector<float> at(n);
  if (hipMemcpy(w.data(), worst, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (hipMemcpy(at.data(), where, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  int best = 0;
  for (int i = 1; i < n; ++i) if (w[i] > w[best]) best = i;
  printf("expf on [%.6f, 0]: %u arguments, largest relative error %.4e (%.3f ulp of 2^-23) at x = %.9g\n", lo, count, w[best],
         w[best] / 1.1920928955078125e-07, at[best]);
  (void)hipFree(worst);
  (void)hipFree(where);
  return 0;
}
