// Host-side pieces shared by the OpenPose body (openpose_api.hip) and hand (openpose_hand_api.hip) estimators: the convolution
// descriptor of openpose_kernels.hip, a packed layer, the launch of one or two convolutions.  (Their grow-only device buffers: bf_grow, bf_host.h.)
#pragma once
#include "bf_host.h"
#include "openpose_kernels.h"

struct OpLayer { size_t w, b; int cin, cout, coutp, k; };       // packed [k*k*cin][coutp] then the bias [coutp]; cin padded to 4

// appends a layer of cin -> cout, k x k to L at float offset *at
inline void op_add_layer(std::vector<OpLayer> &L, size_t *at, int cin, int cout, int k) {
    const int cp = (cin + 3) / 4 * 4, co = (cout + 3) / 4 * 4;
    OpLayer l{*at, *at + (size_t)k * k * cp * co, cp, cout, co, k};
    *at = l.b + co;
    L.push_back(l);
}

inline OpConv conv_of(const float *wts, const OpLayer &l, const float *x, int ldx, float *y, int ldo, int relu) {
    OpConv c;
    c.x = x; c.w = wts + l.w; c.bias = wts + l.b; c.y = y;
    c.ldx = ldx; c.cin = l.cin; c.ldo = ldo; c.cout = l.cout; c.coutp = l.coutp; c.k = l.k; c.relu = relu;
    return c;
}

// one launch of one or two convolutions of the same n x H x W grid (BN = 64 tiles when no output has more than 64 channels)
inline int launch_conv(hipStream_t s, int n, int H, int W, const OpConv &a, const OpConv *b = nullptr) {
    OpConvLaunch L;
    L.g[0] = a; L.g[1] = b ? *b : a; L.n = n; L.H = H; L.W = W;
    const long long M = (long long)n * H * W;
    const int maxc = b ? std::max(a.cout, b->cout) : a.cout;
    const int bn = maxc <= 64 ? 64 : 128;
    const dim3 grid((unsigned)((M + 127) / 128), (unsigned)((maxc + bn - 1) / bn), b ? 2 : 1);
    if (bn == 64) hipLaunchKernelGGL(bf_op_conv64_kernel, grid, dim3(256), 0, s, L);
    else if (a.k == 7) hipLaunchKernelGGL(bf_op_conv7_kernel, grid, dim3(256), 0, s, L);
    else hipLaunchKernelGGL(bf_op_conv128_kernel, grid, dim3(256), 0, s, L);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// MaxPool2d(2, 2) of n x H x W x C (C a multiple of 4) from x into y
inline int launch_pool(hipStream_t s, int n, int H, int W, int C, const float *x, float *y) {
    const long long total = (long long)n * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(bf_op_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n, H, W, C, (const float4 *)x, (float4 *)y);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

inline unsigned op_blocks(long long total) { return (unsigned)((total + 255) / 256); }
