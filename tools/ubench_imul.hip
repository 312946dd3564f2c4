// ubench_imul.hip -- what an integer multiply costs on this chip (profiles/map_hash_notes.md, step 0).
// The hashes of the map walk (csrc/sp_maphash.h) were 32 x 32 multiplies: v_mul_lo_u32 and v_mul_hi_u32 have been
// quarter-rate on every GCN / CDNA part so far, the 24-bit forms v_mul_u32_u24, v_mul_hi_u32_u24 and v_mad_u32_u24
// full-rate; neither figure was on record for gfx950.  This benchmark measures the sustained issue rate of each as a stream
// of instructions that depend on nothing (every one writes its own register from two loop-invariant sources), at the
// occupancy of k5_map2: 512-thread workgroups, four per CU = 8 waves per SIMD, on all CUs.  v_add_u32 and v_xor_b32 are
// the yardstick.  A figure is wave instructions per second, and per SIMD and peak clock (a wave64 instruction occupies a
// 16-lane SIMD for four clocks: "full rate" is 0.25), and how many times the time of a v_add_u32 it takes.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench_imul tools/ubench_imul.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1);} } while (0)

enum { I_ADD, I_XOR, I_MUL_LO, I_MUL_HI, I_MUL24, I_MUL_HI24, I_MAD24 };
#define CHAINS 16
#define REPEAT 4      // CHAINS x REPEAT = 64 instructions per iteration of the loop

template <int INSN>
__global__ void __launch_bounds__(512, 8)
k_stream(uint32_t seed, int iters, unsigned long long *__restrict__ sink) {
    const uint32_t a = seed * (threadIdx.x + 1u) + blockIdx.x, b = (seed ^ 0x9E3779B1u) + threadIdx.x;
    uint32_t r[CHAINS];
#pragma unroll
    for (int i = 0; i < CHAINS; i++) r[i] = 0;
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int rep = 0; rep < REPEAT; rep++)
#pragma unroll
            for (int i = 0; i < CHAINS; i++) {
                if (INSN == I_ADD) asm volatile("v_add_u32 %0, %1, %2" : "=v"(r[i]) : "v"(a), "v"(b));
                else if (INSN == I_XOR) asm volatile("v_xor_b32 %0, %1, %2" : "=v"(r[i]) : "v"(a), "v"(b));
                else if (INSN == I_MUL_LO) asm volatile("v_mul_lo_u32 %0, %1, %2" : "=v"(r[i]) : "v"(a), "v"(b));
                else if (INSN == I_MUL_HI) asm volatile("v_mul_hi_u32 %0, %1, %2" : "=v"(r[i]) : "v"(a), "v"(b));
                else if (INSN == I_MUL24) asm volatile("v_mul_u32_u24 %0, %1, %2" : "=v"(r[i]) : "v"(a), "v"(b));
                else if (INSN == I_MUL_HI24) asm volatile("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r[i]) : "v"(a), "v"(b));
                else asm volatile("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r[i]) : "v"(a), "v"(b), "v"(seed));
            }
    }
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < CHAINS; i++) acc ^= r[i];
    if (acc == 0x1234567u) atomicAdd(sink, 1ULL);
}

template <int INSN>
static double run(const char *what, int cus, double simd_hz, int iters, unsigned long long *sink, double yard) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float best = 1e9;
    for (int t = 0; t < 4; t++) {      // (the first launch also loads the code object)
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL((k_stream<INSN>), dim3(cus * 4), dim3(512), 0, 0, 12345u + t, iters, sink);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (t && ms < best) best = ms;
    }
    const double waves = (double)cus * 4 * 8, insts = waves * (double)iters * CHAINS * REPEAT;
    const double per_s = insts / (best * 1e-3);
    printf("%-18s %8.3f ms  %8.1f G wave-instructions/s  %.4f per SIMD and clock  %5.2f x v_add_u32\n", what, best, per_s / 1e9,
           per_s / ((double)cus * 4 * simd_hz), yard > 0 ? yard / per_s : 1.0);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    return per_s;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const double hz = (double)prop.clockRate * 1e3;      // (the peak engine clock: the rate per clock is a lower bound)
    unsigned long long *sink;
    CK(hipMalloc(&sink, 8));
    CK(hipMemset(sink, 0, 8));
    const int iters = 20000;
    printf("%s, %d CUs, %.0f MHz; %d waves of 64 x %d instructions each\n", prop.name, cus, hz / 1e6, cus * 32, iters * CHAINS * REPEAT);
    const double yard = run<I_ADD>("v_add_u32", cus, hz, iters, sink, 0);
    run<I_XOR>("v_xor_b32", cus, hz, iters, sink, yard);
    run<I_MUL_LO>("v_mul_lo_u32", cus, hz, iters, sink, yard);
    run<I_MUL_HI>("v_mul_hi_u32", cus, hz, iters, sink, yard);
    run<I_MUL24>("v_mul_u32_u24", cus, hz, iters, sink, yard);
    run<I_MUL_HI24>("v_mul_hi_u32_u24", cus, hz, iters, sink, yard);
    run<I_MAD24>("v_mad_u32_u24", cus, hz, iters, sink, yard);
    CK(hipFree(sink));
    return 0;
}
