// What hmr_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct HmrConv {
    const float *x, *w, *bias, *res;
    float *y;
    int n, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, ldo, relu;
};

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_hmr_resize_kernel(int n, int H, int W, double scale_y, double scale_x, const uint8_t *src, uint8_t *resized, float *out, float3 mean,
                                                float3 stdv);
extern "C" __global__ void bf_hmr_conv_kernel(HmrConv p);
extern "C" __global__ void bf_hmr_maxpool_kernel(int n, int H, int W, int C, int Ho, int Wo, const float *x, float *y);
extern "C" __global__ void bf_hmr_avgpool_kernel(int n, const float *x, float *xc);
extern "C" __global__ void bf_hmr_init_state_kernel(int n, const float *mean, float *xc);
#pragma GCC visibility pop
