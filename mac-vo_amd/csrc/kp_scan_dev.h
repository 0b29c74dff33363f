// Workgroup-wide scan shared by the selector kernels that compact 64-pixel candidate words in order (kp_select.hip, kp_gradient.hip).
#pragma once
#include <hip/hip_runtime.h>

// workgroup exclusive scan of one int per thread; returns the exclusive prefix and the total
template <int NT>
__device__ __forceinline__ int block_exclusive_scan(int v, int* wave_tot /*[NT/64] LDS*/, int& total) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if ((tid & 63) >= o) incl += t;
    }
    __syncthreads();  // protect wave_tot reuse
    if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int t = wave_tot[w];
        if (w < (tid >> 6)) off += t;
        total += t;
    }
    return off + incl - v;
}
