// Microbenchmark: issue cost of gfx950's lane-half swaps (v_permlane32_swap_b32, v_permlane16_swap_b32) — the first exchange
// of the wave-held 1024-point transform (gab_fft.hpp) is 32 of them back to back — beside v_mov_b32 and v_fma_f32, for 1, 2
// and 4 resident waves per SIMD.  Prints clocks per instruction per wave and per SIMD.  Whole waves, EXEC all ones.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { if ((x) != hipSuccess) { std::printf("%s failed\n", #x); std::exit(1); } } while (0)
// MODE 0: v_permlane32_swap, 1: v_permlane16_swap, 2: the transform's mix (16 + 16 on sixteen registers), 3: v_mov_b32, 4: v_fma_f32
template <int MODE>
__global__ void k(float* out, int iters) {
    unsigned a0 = threadIdx.x, a1 = 1 + a0, a2 = 2 + a0, a3 = 3 + a0, a4 = 4 + a0, a5 = 5 + a0, a6 = 6 + a0, a7 = 7 + a0;
    float f0 = threadIdx.x, f1 = 1, f2 = 2, f3 = 3, f4 = 4, f5 = 5, f6 = 6, f7 = 7;
    const float c = 1.0001f, d = 0.5f;
    long long t0 = clock64();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {                            // 4 instructions per line: 32 per trip
            if (MODE == 0)
                asm volatile("v_permlane32_swap_b32 %0, %4\n v_permlane32_swap_b32 %1, %5\n v_permlane32_swap_b32 %2, %6\n v_permlane32_swap_b32 %3, %7"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if (MODE == 1)
                asm volatile("v_permlane16_swap_b32 %0, %4\n v_permlane16_swap_b32 %1, %5\n v_permlane16_swap_b32 %2, %6\n v_permlane16_swap_b32 %3, %7"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if (MODE == 2)
                asm volatile("v_permlane32_swap_b32 %0, %4\n v_permlane32_swap_b32 %1, %5\n v_permlane16_swap_b32 %0, %1\n v_permlane16_swap_b32 %4, %5"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if (MODE == 3)
                asm volatile("v_mov_b32 %0, %4\n v_mov_b32 %1, %5\n v_mov_b32 %2, %6\n v_mov_b32 %3, %7"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else
                asm volatile("v_fma_f32 %0, %0, %4, %5\n v_fma_f32 %1, %1, %4, %5\n v_fma_f32 %2, %2, %4, %5\n v_fma_f32 %3, %3, %4, %5"
                             : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3) : "v"(c), "v"(d));
        }
    }
    long long t1 = clock64();
    unsigned r = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
    float fr = f0 + f1 + f2 + f3 + f4 + f5 + f6 + f7;
    if (r == 0x12345678u || fr == 12345.678f) out[0] = (float)r + fr;
    if (threadIdx.x == 0 && blockIdx.x == 0) out[1] = (float)(t1 - t0);
}
template <int MODE> void run(const char* name, int waves_per_simd) {
    float* d; CK(hipMalloc(&d, 16));
    const int iters = 2000;
    // one block of 256 threads = 1 wave per SIMD on its CU; launch waves_per_simd blocks per CU
    const int blocks = 256 * waves_per_simd;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    k<MODE><<<blocks, 256>>>(d, 10); CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0)); k<MODE><<<blocks, 256>>>(d, iters); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    float h[4]; CK(hipMemcpy(h, d, 16, hipMemcpyDeviceToHost));
    const double instr_per_wave = (double)iters * 32;
    const double per_wave = h[1] / instr_per_wave;
    printf("%-22s waves/SIMD=%d: %.2f clk/instr per wave -> %.2f clk/instr per SIMD, 32 back to back %.0f clk  (kernel %.3f ms)\n",
           name, waves_per_simd, per_wave, per_wave / waves_per_simd, 32 * per_wave, ms);
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    CK(hipFree(d));
}
int main() {
    for (int w : {1, 2, 4}) run<0>("v_permlane32_swap_b32", w);
    for (int w : {1, 2, 4}) run<1>("v_permlane16_swap_b32", w);
    for (int w : {1, 2, 4}) run<2>("16 + 16 as in the fft", w);
    for (int w : {1, 2, 4}) run<3>("v_mov_b32", w);
    for (int w : {1, 2, 4}) run<4>("v_fma_f32", w);
    return 0;
}
