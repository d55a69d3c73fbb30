// DEV microbenchmark: the per-tile issue budget of the unified dK/dV kernel (csrc/usp_flash_bwd64u.hip) on one wave per SIMD.
// One workgroup of 4 waves per CU.  A tile is two 32-row slices of 64 MFMA gaps (S chain 0-15 | dP chain 16-31 | dV 32-47 | dK
// 48-63; chains accumulate in arch VGPRs, gradients in AGPRs).  Per slice the kernel issues 64 MFMAs, 32 x (v_mul, v_exp) for P,
// 32 x (unpack, v_mul) for dS, 32 packs, 16 row fragments (ds_read_b128) + 32 transposed half-fragments (ds_read_b64) + 16
// statistics reads, 28 address XORs and a counted wait per fragment; per tile one barrier.  Every variant runs that budget on
// independent registers (no dependences, no memory waits beyond the counted lgkmcnt, no LDS-DMA pieces), so each figure is a
// LOWER bound for its placement:
//   mfma      128 MFMAs and nothing else (the floor: 128 x 32 = 4096 cycles)
//   shipped   the shipped placement: P's elements two per gap in gaps 17-32, dS's in gaps 33-54, reads three fragments ahead
//   level     the same instructions levelled over all 64 gaps (2.5 VALU per gap, a v_exp every other gap)
//   level-lds ... and without the statistics reads (what 8 instead of 16 of them per chain pair would approach)
// and, for the instruction diet (profiles/dkdv64u_diet.txt), the shipped placement with what the census of the kernel's plain
// loop has beyond it -- 28 statistics reads (4 + 8 | 8 | 8), the 8 v_mov_b64 of the first chain's constants, two wait states
// in front of each chain's first MFMAs, 50 scalar instructions (40 behind the tile's first MFMAs, 10 at its end) -- and that
// budget minus one step's instructions each:
//   full      the census budget
//   -xor      28 address XORs instead of 56 (a swizzled address serves both phases that differ by an immediate)
//   -copies   no v_mov_b64, no wait states at the chains' heads, 16 statistics reads (the constants land in ONE key block's
//             accumulator; the other block's first MFMA takes them from there as SrcC)
//   -waits    one counted wait per two fragments
//   -salu     36 scalar instructions instead of 50
//   diet      -xor, -copies and -salu together;  diet-waits: ... and -waits
// Prints shader cycles per tile (128 MFMAs per wave) beside 2 x 2863 = 5726, the 128-key kernel's measured tile pair
// (profiles/r05_kernel_experiments.txt).          hipcc --offload-arch=gfx950 -O2 ubench_dkdv_unified.hip -o ubench_dkdv_unified
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <utility>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): `#pragma unroll` gives up on a body of this size
template <int... I, class F> __device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>{}, f); }

struct Regs {
  f32x16 acc[4], acca[4];
  u32x4 a, b, ld[4];
  u32x2 ld2[4];
  float e[8], f[8];
  int laddr, x[4];
  int sg[4], y[4];
};

// fillers of one gap: NEXP x (v_mul, v_exp), NDS x (unpack, v_mul), CVT packs, row / transposed / statistics reads, XORs, a wait
__device__ __forceinline__ void fill(Regs& r, int g, int nexp, int nds, int cvt, int rows, int trs, int stats, int xors, int wait) {
#pragma unroll
  for (int i = 0; i < nexp; ++i) {
    asm volatile("v_mul_f32 %0, %0, %1" : "+v"(r.e[(2 * g + i) & 7]) : "v"(r.f[7]));
    asm volatile("v_exp_f32 %0, %0" : "+v"(r.e[(2 * g + i + 4) & 7]));
  }
#pragma unroll
  for (int i = 0; i < nds; ++i) {
    asm volatile("v_lshlrev_b32 %0, 16, %1" : "+v"(r.f[(2 * g + i) & 3]) : "v"(r.x[i & 3]));
    asm volatile("v_mul_f32 %0, %0, %1" : "+v"(r.f[4 + ((2 * g + i) & 1)]) : "v"(r.f[6]));
  }
#pragma unroll
  for (int i = 0; i < cvt; ++i) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %1" : "+v"(r.x[(g + i) & 3]) : "v"(r.f[6]));
#pragma unroll
  for (int i = 0; i < xors; ++i) asm volatile("v_xor_b32 %0, 32, %1" : "+v"(r.y[(g + i) & 3]) : "v"(r.laddr));
#pragma unroll
  for (int i = 0; i < rows + stats; ++i) asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(r.ld[(g + i) & 3]) : "v"(r.laddr), "n"(2048));
#pragma unroll
  for (int i = 0; i < trs; ++i) asm volatile("ds_read_b64 %0, %1 offset:%2" : "+v"(r.ld2[(2 * g + i) & 3]) : "v"(r.laddr), "n"(4096));
  if (wait) asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
}
// what the kernel's census has beyond fill(): scalar instructions, v_mov_b64 copies, wait states in front of the gap's MFMA
__device__ __forceinline__ void extra(Regs& r, int g, int salu, int movs, int nop) {
#pragma unroll
  for (int i = 0; i < salu; ++i) asm volatile("s_add_i32 %0, %0, 1" : "+s"(r.sg[(g + i) & 3]) : : "scc");      // (writes SCC: the tile loop's compare must not straddle it)
#pragma unroll
  for (int i = 0; i < movs; ++i) asm volatile("v_mov_b64 %0, %1" : "+v"(r.ld2[i & 3]) : "v"(r.ld2[(i + 1) & 3]));
  if (nop) asm volatile("s_nop 1");
}
// MODE >= 4: bit 0 of (MODE - 4) = -xor, bit 1 = -copies, bit 2 = -waits, bit 3 = -salu

template <int MODE>
__global__ __launch_bounds__(256, 1) void k(uint64_t* out, const uint32_t* pat, int tiles) {
  extern __shared__ char lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  Regs r;
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 16; ++j) { r.acc[i][j] = 0.f; r.acca[i][j] = 0.f; }
  r.a = u32x4{pat[lane], pat[64 + lane], pat[128 + lane], pat[192 + lane]};
  r.b = u32x4{pat[256 + lane], pat[320 + lane], pat[384 + lane], pat[448 + lane]};
  for (int i = 0; i < 8; ++i) { r.e[i] = -0.5f - i; r.f[i] = 0.001f * (lane + i); }
  for (int i = 0; i < 4; ++i) { r.ld[i] = r.a; r.ld2[i] = u32x2{r.a[0], r.b[0]}; r.x[i] = lane + i; r.sg[i] = tiles + i; r.y[i] = lane - i; }
  r.laddr = lane * 16;
  ((u32x4*)lds)[threadIdx.x] = r.a;
  ((u32x4*)lds)[256 + threadIdx.x] = r.b;
  __syncthreads();
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < tiles; ++t) {
    static_for<2>([&](auto h_c) __attribute__((always_inline)) {       // straight-line, as the kernel's tile body is
      constexpr int h = decltype(h_c)::value;
      static_for<64>([&](auto g_c) __attribute__((always_inline)) {
        constexpr int g = decltype(g_c)::value;
        constexpr int V = MODE >= 4 ? MODE - 4 : 0;
        constexpr bool NOX = V & 1, NOC = V & 2, NOW = V & 4, NOS = V & 8;
        if (MODE >= 4) extra(r, g, 0, (!NOC && h == 0 && g == 0) ? 8 : 0, !NOC && (g & 15) < 2 && g < 32);
        if (g < 32) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(r.acc[g & 3]) : "v"(r.a), "v"(r.b));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(r.acca[g & 3]) : "v"(r.a), "v"(r.b));
        const int even = !(g & 1);
        const int rows = (even && g < 32) ? 1 : 0, trs = (even && g >= 32) ? 2 : 0;      // one fragment per two gaps
        const int xors = (even && (g & 15)) ? 1 : 0;
        if (MODE == 1) {
          const int stats = ((g >= 6 && g < 14) || (g >= 54 && g < 62)) ? 1 : 0;
          const int nexp = (g >= 17 && g < 33) ? 2 : 0;
          const int nds = (g >= 33 && g < 55) ? (g - 32) * 32 / 22 - (g - 33) * 32 / 22 : 0;       // 32 elements over 22 gaps
          fill(r, g, nexp, nds, (nexp + nds + 1) / 2, rows, trs, stats, xors, even);
        } else if (MODE >= 4) {
          const int nst = NOC ? 4 : 8;                                               // statistics reads of a chain pair
          const int stats = ((h == 0 && g == 0) ? 4 : 0) + ((g >= 6 && g < 6 + nst) ? 1 : 0) + ((h == 0 && g >= 54 && g < 54 + nst) ? 1 : 0);
          const int nexp = (g >= 17 && g < 33) ? 2 : 0;
          const int nds = (g >= 33 && g < 55) ? (g - 32) * 32 / 22 - (g - 33) * 32 / 22 : 0;
          const int xr = NOX ? ((g & 31) < 16 ? xors : 0) : xors;                      // the second phase of a pair reuses the first's
          fill(r, g, nexp, nds, (nexp + nds + 1) / 2, rows, trs, stats, xr, NOW ? !(g & 3) : even);
          extra(r, g, (h == 0 && g < 8) ? ((NOS && g) ? 3 : 5) : ((h == 1 && g == 63) ? 10 : 0), 0, 0);
        } else if (MODE >= 2) {
          const int stats = (MODE == 2 && (g & 3) == 3) ? 1 : 0;
          fill(r, g, even ? 1 : 0, even ? 0 : 1, even ? 1 : 0, rows, trs, stats, xors, even);
        }
      });
    });
    if (MODE) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  float sink = 0.f;
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 16; ++j) sink += r.acc[i][j] + r.acca[i][j];
  for (int i = 0; i < 8; ++i) sink += r.e[i] + r.f[i];
  for (int i = 0; i < 4; ++i) sink += (float)r.ld[i][0] + (float)r.ld2[i][0] + (float)r.x[i] + (float)r.sg[i] + (float)r.y[i];
  if (lane == 0 && blockIdx.x == 0) { out[wave] = t1 - t0; out[8 + wave] = (uint64_t)sink; }
}

template <int MODE> static int run(uint64_t* d, const uint32_t* pat, int cus, const char* what) {
  const int tiles = 300;
  for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL((k<MODE>), dim3(cus), dim3(256), 16384, 0, d, pat, tiles);
  HIP_OK(hipDeviceSynchronize());
  uint64_t h[16];
  HIP_OK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
  uint64_t mx = 0;
  for (int w = 0; w < 4; ++w) mx = h[w] > mx ? h[w] : mx;
  const double cyc = (double)mx / tiles;
  printf("%-58s %7.1f cycles per 128-MFMA tile = %5.1f per MFMA; 2 x 2863 = 5726: %+5.1f %%\n", what, cyc, cyc / 128, 100.0 * (cyc / 5726.0 - 1.0));
  return 0;
}

int main() {
  uint64_t* d; HIP_OK(hipMalloc(&d, 256));
  uint32_t hp[512];
  uint32_t s = 12345u;
  for (int i = 0; i < 512; ++i) {          // pairs of bf16 with pseudo-random sign / mantissa and exponents around 2^-1 .. 2^1
    s = s * 1664525u + 1013904223u; const uint32_t lo = (0x3f00u + ((s >> 9) & 0x1ffu)) | ((s >> 3) & 0x8000u);
    s = s * 1664525u + 1013904223u; const uint32_t hi = (0x3f00u + ((s >> 9) & 0x1ffu)) | ((s >> 3) & 0x8000u);
    hp[i] = lo | (hi << 16);
  }
  uint32_t* pat; HIP_OK(hipMalloc(&pat, sizeof hp)); HIP_OK(hipMemcpy(pat, hp, sizeof hp, hipMemcpyHostToDevice));
  int dev = 0, cus = 256; HIP_OK(hipGetDevice(&dev)); HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  for (int rep = 0; rep < 2; ++rep) {
    if (run<0>(d, pat, cus, "mfma: 128 MFMAs alone")) return 1;
    if (run<1>(d, pat, cus, "shipped: P in gaps 17-32, dS in 33-54")) return 1;
    if (run<2>(d, pat, cus, "level: the same budget over all 64 gaps")) return 1;
    if (run<3>(d, pat, cus, "level-lds: ... without the statistics reads")) return 1;
    if (run<4>(d, pat, cus, "full: the census of the kernel's plain loop")) return 1;
    if (run<5>(d, pat, cus, "-xor: 28 address XORs instead of 56")) return 1;
    if (run<6>(d, pat, cus, "-copies: no v_mov_b64 / head wait states, 16 stat reads")) return 1;
    if (run<8>(d, pat, cus, "-waits: one counted wait per two fragments")) return 1;
    if (run<12>(d, pat, cus, "-salu: 36 scalar instructions instead of 50")) return 1;
    if (run<15>(d, pat, cus, "diet: -xor -copies -salu")) return 1;
    if (run<19>(d, pat, cus, "diet-waits: -xor -copies -salu -waits")) return 1;
  }
  return 0;
}
