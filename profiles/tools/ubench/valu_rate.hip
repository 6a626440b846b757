// VALU issue-rate microbenchmark for gfx950: cycles per wave64 instruction for scalar and packed fp32, dependent and independent chains,
// and for the instruction classes the rollout step loop spends its slots on besides v_fma_f32 (compare-and-select pairs with their
// hazard s_nop, v_med3_f32, v_max_f32 with an SGPR operand, v_mov_b32 from an SGPR, s_nop 1, v_rsq_f32, v_fma_f64, and the bookkeeping
// classes: v_mul_lo_u32, v_cvt_f64_f32, v_add_f64, v_readfirstlane_b32, v_lshl_add_u64), at 1..8 waves per SIMD.  Build with the library's flags
// (__graft_entry__.HIPCC_FLAGS; without -fno-slp-vectorize the SLP vectoriser packs the "scalar fma, 8 independent" mode into v_pk_fma_f32 and
// the figure is a packed one): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -Wno-pass-failed -o valu_rate valu_rate.hip ; run: ./valu_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef float f2 __attribute__((ext_vector_type(2)));
#define REP 256
// one instruction (or one compare-and-select pair) on each of eight independent registers; the text is fixed, so the compiler
// neither folds nor reorders it
#define ASM8(text, ...)                                                                                                           \
  asm volatile(text : "+v"(a0) : __VA_ARGS__); asm volatile(text : "+v"(a1) : __VA_ARGS__); asm volatile(text : "+v"(a2) : __VA_ARGS__);   \
  asm volatile(text : "+v"(a3) : __VA_ARGS__); asm volatile(text : "+v"(a4) : __VA_ARGS__); asm volatile(text : "+v"(a5) : __VA_ARGS__);   \
  asm volatile(text : "+v"(a6) : __VA_ARGS__); asm volatile(text : "+v"(a7) : __VA_ARGS__)
template <int MODE> __global__ void k(float* out, unsigned long long* cyc, int iters, float seed, float slo, float shi) {
  float a0 = seed + threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  f2 p0 = {a0, a1}, p1 = {a2, a3}, p2 = {a4, a5}, p3 = {a6, a7};
  double d0 = a0, d1 = a1, d2 = a2, d3 = a3;
  const float m = 1.0000001f, c = 1e-9f;
  const f2 pm = {m, m}, pc = {c, c};
  const double dm = 1.0000001, dc = 1e-9;
  float vlo = slo;                                   // the bound a v_cndmask needs in a VGPR
  asm volatile("" : "+v"(vlo));
  asm volatile("" : "+s"(slo), "+s"(shi));           // ... and the same bounds as SGPR operands
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < REP / 8; ++r) {
      if (MODE == 0) {  // 8 independent scalar fma chains
        a0 = fmaf(a0, m, c); a1 = fmaf(a1, m, c); a2 = fmaf(a2, m, c); a3 = fmaf(a3, m, c);
        a4 = fmaf(a4, m, c); a5 = fmaf(a5, m, c); a6 = fmaf(a6, m, c); a7 = fmaf(a7, m, c);
      } else if (MODE == 1) {  // one dependent scalar chain
        a0 = fmaf(a0, m, c); a0 = fmaf(a0, m, c); a0 = fmaf(a0, m, c); a0 = fmaf(a0, m, c);
        a0 = fmaf(a0, m, c); a0 = fmaf(a0, m, c); a0 = fmaf(a0, m, c); a0 = fmaf(a0, m, c);
      } else if (MODE == 2) {  // 4 independent packed fma chains (8 instructions: two rounds)
        p0 = __builtin_elementwise_fma(p0, pm, pc); p1 = __builtin_elementwise_fma(p1, pm, pc);
        p2 = __builtin_elementwise_fma(p2, pm, pc); p3 = __builtin_elementwise_fma(p3, pm, pc);
        p0 = __builtin_elementwise_fma(p0, pm, pc); p1 = __builtin_elementwise_fma(p1, pm, pc);
        p2 = __builtin_elementwise_fma(p2, pm, pc); p3 = __builtin_elementwise_fma(p3, pm, pc);
      } else if (MODE == 3) {  // one dependent packed chain
        for (int q = 0; q < 8; ++q) p0 = __builtin_elementwise_fma(p0, pm, pc);
      } else if (MODE == 4) {  // packed mul, 4 independent chains
        p0 = p0 * pm; p1 = p1 * pm; p2 = p2 * pm; p3 = p3 * pm; p0 = p0 * pm; p1 = p1 * pm; p2 = p2 * pm; p3 = p3 * pm;
      } else if (MODE == 5) {  // two dependent scalar chains interleaved
        a0 = fmaf(a0, m, c); a1 = fmaf(a1, m, c); a0 = fmaf(a0, m, c); a1 = fmaf(a1, m, c);
        a0 = fmaf(a0, m, c); a1 = fmaf(a1, m, c); a0 = fmaf(a0, m, c); a1 = fmaf(a1, m, c);
      } else if (MODE == 6) {  // x < lo ? lo : x as the compiler emits it back to back: v_cmp -> vcc, the hazard s_nop 1, v_cndmask (8 pairs)
        ASM8("v_cmp_lt_f32_e32 vcc, %1, %0\n\ts_nop 1\n\tv_cndmask_b32_e32 %0, %2, %0, vcc", "s"(slo), "v"(vlo) : "vcc");
      } else if (MODE == 7) {  // the same clamp in one v_med3_f32 (an inline constant and an SGPR bound)
        ASM8("v_med3_f32 %0, %0, 0, %1", "s"(shi));
      } else if (MODE == 8) {  // v_max_f32 with an SGPR operand
        ASM8("v_max_f32_e32 %0, %1, %0", "s"(slo));
      } else if (MODE == 9) {  // v_mov_b32 from an SGPR
        ASM8("v_mov_b32_e32 %0, %1", "s"(slo));
      } else if (MODE == 10) {  // s_nop 1 (counted as one instruction each)
        asm volatile("s_nop 1\n\ts_nop 1\n\ts_nop 1\n\ts_nop 1\n\ts_nop 1\n\ts_nop 1\n\ts_nop 1\n\ts_nop 1");
      } else if (MODE == 11) {  // v_rsq_f32, 8 independent
        ASM8("v_rsq_f32_e32 %0, %0", "s"(slo));
      } else if (MODE == 12) {  // v_fma_f64, 4 independent chains (8 instructions: two rounds)
        d0 = fma(d0, dm, dc); d1 = fma(d1, dm, dc); d2 = fma(d2, dm, dc); d3 = fma(d3, dm, dc);
        d0 = fma(d0, dm, dc); d1 = fma(d1, dm, dc); d2 = fma(d2, dm, dc); d3 = fma(d3, dm, dc);
      } else if (MODE == 13) {  // the compare-and-select pair with two independent instructions between, as a scheduler would hide the hazard
        ASM8("v_cmp_lt_f32_e32 vcc, %1, %0\n\tv_max_f32_e32 %0, %0, %0\n\tv_max_f32_e32 %0, %0, %0\n\tv_cndmask_b32_e32 %0, %2, %0, vcc", "s"(slo), "v"(vlo) : "vcc");
      } else if (MODE == 14) {  // v_mul_lo_u32 with an SGPR factor (the row writer's wave * 5120), 8 independent
        ASM8("v_mul_lo_u32 %0, %0, %1", "s"(slo));
      } else if (MODE == 15) {  // v_cvt_f64_f32 (the double copies of the trajectory parameters), 8 conversions into 4 register pairs
        asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d0) : "v"(a0)); asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d1) : "v"(a1));
        asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d2) : "v"(a2)); asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d3) : "v"(a3));
        asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d0) : "v"(a4)); asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d1) : "v"(a5));
        asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d2) : "v"(a6)); asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(d3) : "v"(a7));
      } else if (MODE == 16) {  // v_add_f64 (the time's t + dt), 4 independent chains, two rounds
        d0 = d0 + dc; d1 = d1 + dc; d2 = d2 + dc; d3 = d3 + dc; d0 = d0 + dc; d1 = d1 + dc; d2 = d2 + dc; d3 = d3 + dc;
      } else if (MODE == 17) {  // v_readfirstlane_b32 into 8 SGPRs
        int s0, s1, s2, s3, s4, s5, s6, s7;
        asm volatile("v_readfirstlane_b32 %0, %8\n\tv_readfirstlane_b32 %1, %9\n\tv_readfirstlane_b32 %2, %10\n\tv_readfirstlane_b32 %3, %11\n\t"
                     "v_readfirstlane_b32 %4, %12\n\tv_readfirstlane_b32 %5, %13\n\tv_readfirstlane_b32 %6, %14\n\tv_readfirstlane_b32 %7, %15"
                     : "=s"(s0), "=s"(s1), "=s"(s2), "=s"(s3), "=s"(s4), "=s"(s5), "=s"(s6), "=s"(s7)
                     : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7));
      } else if (MODE == 18) {  // v_lshl_add_u64 (a 64-bit per-lane address), 4 independent register pairs, two rounds
        asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d0) : "v"(d1)); asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d1) : "v"(d2));
        asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d2) : "v"(d3)); asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d3) : "v"(d0));
        asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d0) : "v"(d1)); asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d1) : "v"(d2));
        asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d2) : "v"(d3)); asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d3) : "v"(d0));
      }
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + p0.x + p0.y + p1.x + p1.y + p2.x + p2.y + p3.x + p3.y +
                                               (float)(d0 + d1 + d2 + d3);
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}
// per: instructions issued per counted unit (a compare-and-select pair is one unit of 2 VALU + s_nop 1)
template <int MODE> void run(const char* name, int waves_per_simd) {
  // workgroups of <= 16 waves on the 4 SIMDs of a CU: one per CU up to 4 waves per SIMD, two above
  const int per_cu = waves_per_simd > 4 ? 2 : 1, block = 64 * 4 * waves_per_simd / per_cu, cus = 256 * per_cu;
  float* out; unsigned long long* cyc;
  hipMalloc(&out, sizeof(float) * cus * block); hipMalloc(&cyc, 8 * cus);
  const int iters = 200;
  k<MODE><<<cus, block>>>(out, cyc, iters, 1.0f, 0.5f, 3.0e4f); hipDeviceSynchronize();
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0); k<MODE><<<cus, block>>>(out, cyc, iters, 1.0f, 0.5f, 3.0e4f); hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> h(cus); hipMemcpy(h.data(), cyc, 8 * cus, hipMemcpyDeviceToHost);
  double mean = 0; for (auto v : h) mean += v; mean /= cus;
  const double instr = (double)iters * REP;   // per wave
  printf("%-44s waves/SIMD %d: %.0f memtime ticks, %.3f ms -> %.2f ticks / instr / wave, %.2f ns * SIMD per instr\n", name, waves_per_simd, mean, ms,
         mean / instr, ms * 1e6 / (instr * waves_per_simd));
  hipEventDestroy(e0); hipEventDestroy(e1);
  hipFree(out); hipFree(cyc);
}
int main() {
  for (int w : {1, 2, 4, 6, 8}) {
    run<0>("scalar fma, 8 independent", w);
    run<1>("scalar fma, dependent", w);
    run<5>("scalar fma, 2 dependent chains", w);
    run<2>("packed fma, 4 independent", w);
    run<3>("packed fma, dependent", w);
    run<4>("packed mul, 4 independent", w);
    run<6>("v_cmp + s_nop 1 + v_cndmask (per pair)", w);
    run<13>("v_cmp + 2 VALU + v_cndmask (per group of 4)", w);
    run<7>("v_med3_f32 (0, SGPR)", w);
    run<8>("v_max_f32, SGPR operand", w);
    run<9>("v_mov_b32 from SGPR", w);
    run<10>("s_nop 1", w);
    run<11>("v_rsq_f32, 8 independent", w);
    run<12>("v_fma_f64, 4 independent", w);
    run<14>("v_mul_lo_u32, SGPR factor", w);
    run<15>("v_cvt_f64_f32", w);
    run<16>("v_add_f64, 4 independent", w);
    run<17>("v_readfirstlane_b32", w);
    run<18>("v_lshl_add_u64", w);
  }
  return 0;
}
