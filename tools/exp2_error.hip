// The relative error of the device's exp2 -- v_exp_f32 through __builtin_amdgcn_exp2f, the instruction the block attention mass
// kernel (csrc/usp_block_mass.hip) and the flash kernels take their probabilities from -- against the fp64 exp2, over EVERY fp32
// argument in [-126, 0].  Prints the largest relative error and where it falls.  tests/block_mass_ref.py takes twice the printed
// value as its e_exp.
//   hipcc --offload-arch=gfx950 -O3 tools/exp2_error.hip -o exp2_error && ./exp2_error
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// arguments: the floats -0.f .. lo as the integers 0x80000000 + i, i in [0, count)
__global__ void exp2_error_kernel(uint32_t count, double* worst, float* where) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, n = gridDim.x * blockDim.x;
  double w = 0.0;
  float at = 0.f;
  for (uint32_t i = t; i < count; i += n) {
    const uint32_t bits = 0x80000000u + i;
    float x;
    memcpy(&x, &bits, 4);
    const double want = exp2((double)x);
    const double err = fabs((double)__builtin_amdgcn_exp2f(x) - want) / want;
    if (err > w) { w = err; at = x; }
  }
  worst[t] = w;
  where[t] = at;
}

int main() {
  const float lo = -126.f;
  uint32_t lo_bits;
  memcpy(&lo_bits, &lo, 4);
  const uint32_t count = lo_bits - 0x80000000u + 1u;
  const int blocks = 2048, threads = 256, n = blocks * threads;
  double* worst;
  float* where;
  if (hipMalloc(&worst, n * sizeof(double)) != hipSuccess || hipMalloc(&where, n * sizeof(float)) != hipSuccess) return 1;
  hipLaunchKernelGGL(exp2_error_kernel, dim3(blocks), dim3(threads), 0, 0, count, worst, where);
  std::vector<double> w(n);
  std::vector<float> at(n);
  if (hipMemcpy(w.data(), worst, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (hipMemcpy(at.data(), where, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  int best = 0;
  for (int i = 1; i < n; ++i) if (w[i] > w[best]) best = i;
  printf("exp2 (v_exp_f32) on [%.6f, 0]: %u arguments, largest relative error %.4e (%.3f ulp of 2^-23) at x = %.9g\n", lo, count, w[best],
         w[best] / 1.1920928955078125e-07, at[best]);
  (void)hipFree(worst);
  (void)hipFree(where);
  return 0;
}
