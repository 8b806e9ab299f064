// LDS 64-bit atomic-add rate microbench: what pair_low_general_kernel's updates (two ds_add_u64 on adjacent words, no
// return) cost, beside lds_add_rate.hip's ds_add_u32.  16 waves per workgroup, 1 or 2 workgroups per CU, a 64-KiB
// accumulator per workgroup -- the product kernel's shape.  Modes:
//   0  ds_add_u64, conflict-free (lane l -> its own 8 bytes, a 16-KiB window)
//   1  two ds_add_u64 at the kernel's addresses: (random row of 64) * 1024 + (random column of 64) * 16, and + 8
// Every mode checks the accumulators' total against the number of adds issued (modulo 2^64).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

constexpr int UNROLL = 16;

template <int MODE>
__global__ __launch_bounds__(1024) void rate(unsigned long long *out, int iters, uint32_t seed, unsigned long long *clk)
{
    __shared__ unsigned long long acc[8192];
    for (int k = threadIdx.x; k < 8192; k += 1024) acc[k] = 0;
    __syncthreads();
    uint32_t addr[UNROLL];
    uint32_t h = threadIdx.x * 2654435761u + seed + blockIdx.x * 40503u;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        if (MODE == 1) {
            h ^= h << 13; h ^= h >> 17; h ^= h << 5;
            addr[u] = ((h >> 8) & 63u) * 1024u + (h & 63u) * 16u;
        } else {
            addr[u] = ((threadIdx.x & 255u) + 256u * (uint32_t)(u & 7)) * 8u;
        }
    }
    const unsigned long long v = ((unsigned long long)seed << 29) | 1ull;
    unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            asm volatile("ds_add_u64 %0, %1" ::"v"(addr[u]), "v"(v) : "memory");
            if (MODE == 1) asm volatile("ds_add_u64 %0, %1 offset:8" ::"v"(addr[u]), "v"(v) : "memory");
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
    unsigned long long t = 0;
    for (int k = threadIdx.x; k < 8192; k += 1024) t += acc[k];
    out[blockIdx.x * blockDim.x + threadIdx.x] = t;
    if (threadIdx.x == 0 && blockIdx.x == 7) { clk[0] = t1 - t0; clk[1] = r1 - r0; }
}

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    unsigned long long *d, *dc, hc[2];
    CK(hipMalloc(&d, (size_t)cus * 2 * 1024 * 8));
    CK(hipMalloc(&dc, 16));
    unsigned long long *h = (unsigned long long *)malloc((size_t)cus * 2 * 1024 * 8);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const char *names[] = {"ds_add_u64 conflict-free", "2 x ds_add_u64, rows x columns of 64"};
    for (int mode = 0; mode < 2; ++mode)
        for (int wg = 1; wg <= 2; ++wg) {
            const int grid = cus * wg, iters = 1000;
            const uint32_t seed = 123;
            float ms = 0;
            for (int rep = 0; rep < 3; ++rep) {
                CK(hipEventRecord(e0));
                if (mode == 0) rate<0><<<grid, 1024>>>(d, iters, seed, dc);
                else rate<1><<<grid, 1024>>>(d, iters, seed, dc);
                CK(hipGetLastError());
                CK(hipEventRecord(e1));
                CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms, e0, e1));
            }
            CK(hipMemcpy(hc, dc, 16, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h, d, (size_t)grid * 1024 * 8, hipMemcpyDeviceToHost));
            const double per_lane = (double)iters * UNROLL * (mode == 1 ? 2 : 1);
            const unsigned long long v = ((unsigned long long)seed << 29) | 1ull;
            unsigned long long got = 0;
            for (size_t k = 0; k < (size_t)grid * 1024; ++k) got += h[k];
            const unsigned long long want = (unsigned long long)grid * 1024ull * (unsigned long long)per_lane * v;
            const double ghz = (double)hc[0] / (double)hc[1] * 0.1;
            const double lanes = (double)grid * 1024 * per_lane;
            printf("%-40s %d WG/CU: %7.3f ms  %6.2f T adds/s  %5.2f adds/clk/CU  sums %s  (clock %.2f GHz)\n", names[mode], wg, ms,
                   lanes / ms / 1e9, lanes / (ms * 1e-3) / cus / (ghz * 1e9), got == want ? "exact" : "WRONG", ghz);
        }
    return 0;
}
