// Wave and block reductions shared by the kernel files (every file but fit_kernels.hip, whose DPP sums are its own).
// A reduction's ORDER is part of its name: "equal inputs give equal bits" holds because every call site of a name adds in the
// same order, so a different order is a different function with a different name - never an edit to one of these.
// Reductions that are NOT these, on purpose: the ascending butterflies (1, 2, 4, ..) of expr_kernels.hip and joints_body.h, the
// quad sum of kp_loss_kernels.hip, the DPP / readlane minima of scan_kernels.hip and the fit kernel's DPP row sums.
// One site keeps the descending loop written out, because folding it moved an instruction of its kernel (profiles/helper_fold.md):
// the unsigned byte sum of bf_views_prepare_kernel (views_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

// The sum of v over the wave's 64 lanes by the DESCENDING xor butterfly (32, 16, .. 1), on every lane.  The order is the contract:
// lane l ends with (((((v_l + v_l^32) + ..^16) + ..^8) + ..^4) + ..^2) + ..^1, the same bits on all lanes.
__device__ __forceinline__ float bf_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The sum over a block of 256 threads from its four waves' sums: bf_block_sum_256(bf_wave_sum(a), s4), called by all threads.
// Lane 0 of each wave stores the wave's sum into s4, one barrier, the four waves as (0 + 1) + (2 + 3); every thread gets the result.
// (It takes the wave's sum, not `a`: with bf_wave_sum nested inside it the compiler placed one instruction of every caller differently.)
__device__ __forceinline__ float bf_block_sum_256(float wave_total, float *s4) {
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// wave-wide minimum / maximum of an int by the same butterfly (exact, so the order is free; all lanes get it)
__device__ __forceinline__ int bf_wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int bf_wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
