// What openpose_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct OpConv {
    const float *x, *w, *bias;
    float *y;
    int ldx, cin, ldo, cout, coutp, k, relu;
};
struct OpConvLaunch {
    OpConv g[2];
    int n, H, W;
};

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_op_input_kernel(int n, int H, int W, int Hs, int Ws, int Hp, int Wp, double scale, const uint8_t *src, float4 *out);
extern "C" __global__ void bf_op_conv128_kernel(OpConvLaunch L);
extern "C" __global__ void bf_op_conv64_kernel(OpConvLaunch L);
extern "C" __global__ void bf_op_conv7_kernel(OpConvLaunch L);
extern "C" __global__ void bf_op_pool_kernel(int n, int H, int W, int C, const float4 *x, float4 *y);
extern "C" __global__ void bf_op_up8_kernel(int n, int h, int w, int hq, int wq, const float *out, float *up);
extern "C" __global__ void bf_op_maps_kernel(int n, int H, int W, int h, int w, double sy2, double sx2, const float *up, double *heat, double *paf);
extern "C" __global__ void bf_op_gauss_kernel(int n, int H, int W, int axis, int src_c, const double *src, double *dst);
extern "C" __global__ void bf_op_peaks_kernel(int n, int H, int W, const double *bl, const double *heat, int cap, int *count, int *peaks, double *scores);
extern "C" __global__ void bf_op_pairs_kernel(int npairs, int H, int W, const double *paf, const int *jobs, double *score, int *above);
#pragma GCC visibility pop
