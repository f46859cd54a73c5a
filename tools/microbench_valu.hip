// microbench_valu.hip -- what does one SIMD of gfx950 sustain for plain (non-packed) fp32 VALU?
// Inline asm keeps hipcc from SLP-packing the streams.  8 independent chains, 8 waves per SIMD.
// Build: hipcc --offload-arch=gfx950 -O3 tools/microbench_valu.hip -o tools/microbench_valu
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr int kIters = 4096;

#define CHAIN8(OP)                                                                                         \
  asm volatile(OP " %0, %0, %8, %9\n" OP " %1, %1, %8, %9\n" OP " %2, %2, %8, %9\n" OP " %3, %3, %8, %9\n"  \
               OP " %4, %4, %8, %9\n" OP " %5, %5, %8, %9\n" OP " %6, %6, %8, %9\n" OP " %7, %7, %8, %9\n"  \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a), "v"(b))
#define CHAIN8_2(OP)                                                                          \
  asm volatile(OP " %0, %0, %8\n" OP " %1, %1, %8\n" OP " %2, %2, %8\n" OP " %3, %3, %8\n"     \
               OP " %4, %4, %8\n" OP " %5, %5, %8\n" OP " %6, %6, %8\n" OP " %7, %7, %8\n"     \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a))
#define CHAIN8_1(OP)                                                                  \
  asm volatile(OP " %0, %0\n" OP " %1, %1\n" OP " %2, %2\n" OP " %3, %3\n"             \
               OP " %4, %4\n" OP " %5, %5\n" OP " %6, %6\n" OP " %7, %7\n"             \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7))

#define KERNEL(NAME, BODY)                                                                             \
  __global__ __launch_bounds__(256) void NAME(float* out, float a, float b) {                          \
    float x0 = threadIdx.x + 1, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7; \
    for (int i = 0; i < kIters; ++i) { BODY; }                                                         \
    out[blockIdx.x * blockDim.x + threadIdx.x] = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;               \
  }

KERNEL(k_fma, CHAIN8("v_fma_f32"))
KERNEL(k_mul, CHAIN8_2("v_mul_f32"))
KERNEL(k_add, CHAIN8_2("v_add_f32"))
KERNEL(k_rcp, CHAIN8_1("v_rcp_f32"))
KERNEL(k_sqrt, CHAIN8_1("v_sqrt_f32"))
KERNEL(k_cvt, CHAIN8_1("v_cvt_i32_f32"))

// fp16 operands converted on the way in: x = fma(a, (float)half(b), x) with the half taken from either 16 bits of b (op_sel), and
// the explicit conversions (low half plain, high half through SDWA) -- the luma quad table's sample arithmetic
#define CHAIN8_MIX(SEL)                                                                                                      \
  asm volatile("v_fma_mix_f32 %0, %8, %9, %0 " SEL "\nv_fma_mix_f32 %1, %8, %9, %1 " SEL "\nv_fma_mix_f32 %2, %8, %9, %2 " SEL "\n" \
               "v_fma_mix_f32 %3, %8, %9, %3 " SEL "\nv_fma_mix_f32 %4, %8, %9, %4 " SEL "\nv_fma_mix_f32 %5, %8, %9, %5 " SEL "\n" \
               "v_fma_mix_f32 %6, %8, %9, %6 " SEL "\nv_fma_mix_f32 %7, %8, %9, %7 " SEL "\n"                                     \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a), "v"(b))
#define CHAIN8_1S(OP, SUFFIX)                                                                              \
  asm volatile(OP " %0, %0 " SUFFIX "\n" OP " %1, %1 " SUFFIX "\n" OP " %2, %2 " SUFFIX "\n" OP " %3, %3 " SUFFIX "\n" \
               OP " %4, %4 " SUFFIX "\n" OP " %5, %5 " SUFFIX "\n" OP " %6, %6 " SUFFIX "\n" OP " %7, %7 " SUFFIX "\n" \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7))
KERNEL(k_fma_mix_lo, CHAIN8_MIX("op_sel:[0,0,0] op_sel_hi:[0,1,0]"))
KERNEL(k_fma_mix_hi, CHAIN8_MIX("op_sel:[0,1,0] op_sel_hi:[0,1,0]"))
KERNEL(k_fma_mix_2h, CHAIN8_MIX("op_sel:[0,1,0] op_sel_hi:[1,1,0]"))   // both multiplicands fp16 (low half of a, high half of b)
KERNEL(k_cvt_f16, CHAIN8_1("v_cvt_f32_f16"))
KERNEL(k_cvt_f16_hi, CHAIN8_1S("v_cvt_f32_f16_sdwa", "dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1"))

typedef float float2_t __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_pkfma(float* out, float a, float b) {
  float2_t x0 = {(float)threadIdx.x, 1.f}, x1 = x0 + 1.f, x2 = x0 + 2.f, x3 = x0 + 3.f, x4 = x0 + 4.f, x5 = x0 + 5.f, x6 = x0 + 6.f, x7 = x0 + 7.f;
  const float2_t va = {a, a}, vb = {b, b};
  for (int i = 0; i < kIters; ++i) {
    asm volatile("v_pk_fma_f32 %0, %0, %8, %9\nv_pk_fma_f32 %1, %1, %8, %9\nv_pk_fma_f32 %2, %2, %8, %9\nv_pk_fma_f32 %3, %3, %8, %9\n"
                 "v_pk_fma_f32 %4, %4, %8, %9\nv_pk_fma_f32 %5, %5, %8, %9\nv_pk_fma_f32 %6, %6, %8, %9\nv_pk_fma_f32 %7, %7, %8, %9\n"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(va), "v"(vb));
  }
  const float2_t s = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s.x + s.y;
}

// zeroing moves (the pose kernel's accumulators): 8 independent destinations per statement, as above
KERNEL(k_mov32, asm volatile("v_mov_b32 %0, 0\nv_mov_b32 %1, 0\nv_mov_b32 %2, 0\nv_mov_b32 %3, 0\n"
                             "v_mov_b32 %4, 0\nv_mov_b32 %5, 0\nv_mov_b32 %6, 0\nv_mov_b32 %7, 0\n"
                             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7)))
__global__ __launch_bounds__(256) void k_mov64(float* out, float a, float b) {
  double x0 = threadIdx.x + 1, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  for (int i = 0; i < kIters; ++i) {
    asm volatile("v_mov_b64 %0, 0\nv_mov_b64 %1, 0\nv_mov_b64 %2, 0\nv_mov_b64 %3, 0\n"
                 "v_mov_b64 %4, 0\nv_mov_b64 %5, 0\nv_mov_b64 %6, 0\nv_mov_b64 %7, 0\n"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7));
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = (float)(x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7);
}

// The classes of the photometric pair loop that the list above lacks (DESIGN.md section 5 prices the loop with these figures):
// the footprint's floor and clamp, the integer address arithmetic, compares that write a lane mask to an SGPR pair and selects
// that read one, a packed fp32 multiply, and v_fma_f32 with a scalar operand (a VOP3 instruction reads at most one) against the
// all-vector form k_fma measures.
KERNEL(k_floor, CHAIN8_1("v_floor_f32"))
KERNEL(k_med3, CHAIN8("v_med3_f32"))
KERNEL(k_mad_i24, CHAIN8("v_mad_i32_i24"))
KERNEL(k_lshl_add, CHAIN8("v_lshl_add_u32"))
#define CHAIN8_VS(OP)                                                                                      \
  asm volatile(OP " %0, %0, %8, %9\n" OP " %1, %1, %8, %9\n" OP " %2, %2, %8, %9\n" OP " %3, %3, %8, %9\n"  \
               OP " %4, %4, %8, %9\n" OP " %5, %5, %8, %9\n" OP " %6, %6, %8, %9\n" OP " %7, %7, %8, %9\n"  \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a), "s"(b))
KERNEL(k_fma_sgpr, CHAIN8_VS("v_fma_f32"))
__global__ __launch_bounds__(256) void k_pkmul(float* out, float a, float b) {
  float2_t x0 = {(float)threadIdx.x, 1.f}, x1 = x0 + 1.f, x2 = x0 + 2.f, x3 = x0 + 3.f, x4 = x0 + 4.f, x5 = x0 + 5.f, x6 = x0 + 6.f, x7 = x0 + 7.f;
  const float2_t va = {a, a};
  for (int i = 0; i < kIters; ++i) {
    asm volatile("v_pk_mul_f32 %0, %0, %8\nv_pk_mul_f32 %1, %1, %8\nv_pk_mul_f32 %2, %2, %8\nv_pk_mul_f32 %3, %3, %8\n"
                 "v_pk_mul_f32 %4, %4, %8\nv_pk_mul_f32 %5, %5, %8\nv_pk_mul_f32 %6, %6, %8\nv_pk_mul_f32 %7, %7, %8\n"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(va));
  }
  const float2_t s = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s.x + s.y;
}
// eight compares into eight SGPR pairs per statement; the masks are folded into the result after the loop
__global__ __launch_bounds__(256) void k_cmp_sgpr(float* out, float a, float b) {
  float x0 = threadIdx.x + 1, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  unsigned long long m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0, m6 = 0, m7 = 0;
  for (int i = 0; i < kIters; ++i) {
    asm volatile("v_cmp_lt_f32_e64 %0, %8, %16\nv_cmp_lt_f32_e64 %1, %9, %16\nv_cmp_lt_f32_e64 %2, %10, %16\nv_cmp_lt_f32_e64 %3, %11, %16\n"
                 "v_cmp_lt_f32_e64 %4, %12, %16\nv_cmp_lt_f32_e64 %5, %13, %16\nv_cmp_lt_f32_e64 %6, %14, %16\nv_cmp_lt_f32_e64 %7, %15, %16\n"
                 : "=s"(m0), "=s"(m1), "=s"(m2), "=s"(m3), "=s"(m4), "=s"(m5), "=s"(m6), "=s"(m7)
                 : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(x4), "v"(x5), "v"(x6), "v"(x7), "v"(a));
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = (float)__builtin_popcountll(m0 ^ m1 ^ m2 ^ m3 ^ m4 ^ m5 ^ m6 ^ m7);
}
// selects by a lane mask held in an SGPR pair (every other lane)
__global__ __launch_bounds__(256) void k_cndmask_sgpr(float* out, float a, float b) {
  float x0 = threadIdx.x + 1, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
  const unsigned long long mask = 0x5555555555555555ull;
  for (int i = 0; i < kIters; ++i) {
    asm volatile("v_cndmask_b32_e64 %0, %0, %8, %9\nv_cndmask_b32_e64 %1, %1, %8, %9\nv_cndmask_b32_e64 %2, %2, %8, %9\nv_cndmask_b32_e64 %3, %3, %8, %9\n"
                 "v_cndmask_b32_e64 %4, %4, %8, %9\nv_cndmask_b32_e64 %5, %5, %8, %9\nv_cndmask_b32_e64 %6, %6, %8, %9\nv_cndmask_b32_e64 %7, %7, %8, %9\n"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a), "s"(mask));
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
}

template <typename K>
static void run(const char* name, K kernel, float* d_out) {
  const int blocks = 256 * 8;   // 8 blocks of 4 waves per CU = 8 waves per SIMD
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, d_out, 1.0001f, 0.5f);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0);
  for (int rep = 0; rep < 10; ++rep) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, d_out, 1.0001f, 0.5f);
  (void)hipEventRecord(e1);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  ms /= 10;
  const double per_simd = (double)blocks * 4 * kIters * 8 / 1024.0;
  printf("%-14s %8.3f ms  -> %.2f cycles per wave64 instruction at 2.4 GHz (%.2f at 2.0 GHz)\n", name, ms, (ms * 1e6 * 2.4) / per_simd,
         (ms * 1e6 * 2.0) / per_simd);
}

int main() {
  float* d_out;
  (void)hipMalloc(&d_out, 256 * 8 * 256 * sizeof(float));
  run("v_fma_f32", k_fma, d_out);
  run("v_mul_f32", k_mul, d_out);
  run("v_add_f32", k_add, d_out);
  run("v_pk_fma_f32", k_pkfma, d_out);
  run("v_rcp_f32", k_rcp, d_out);
  run("v_sqrt_f32", k_sqrt, d_out);
  run("v_cvt_i32_f32", k_cvt, d_out);
  run("v_fma_mix lo", k_fma_mix_lo, d_out);
  run("v_fma_mix hi", k_fma_mix_hi, d_out);
  run("v_fma_mix 2xh", k_fma_mix_2h, d_out);
  run("v_cvt_f32_f16", k_cvt_f16, d_out);
  run("v_cvt_f32_f16 hi", k_cvt_f16_hi, d_out);
  run("v_mov_b32 0", k_mov32, d_out);
  run("v_mov_b64 0", k_mov64, d_out);
  run("v_fma_f32 sgpr", k_fma_sgpr, d_out);
  run("v_pk_mul_f32", k_pkmul, d_out);
  run("v_floor_f32", k_floor, d_out);
  run("v_med3_f32", k_med3, d_out);
  run("v_cmp_e64 sgpr", k_cmp_sgpr, d_out);
  run("v_cndmask sgpr", k_cndmask_sgpr, d_out);
  run("v_mad_i32_i24", k_mad_i24, d_out);
  run("v_lshl_add_u32", k_lshl_add, d_out);
  return 0;
}
