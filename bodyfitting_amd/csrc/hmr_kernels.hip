// HMR forward pass (reference models/hmr.py, smplify/body_fitting.py:57-68): the run_hmr image pipeline, the ResNet-50 convolutions
// as one implicit-GEMM kernel on the exact-fp32 MFMA, the pools and the regressor's state.  Host side: hmr_api.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hmr_kernels.h"
#include "resize_axis.h"

#define HMR_RES 224
#define HMR_FEAT 2048
#define HMR_NSTATE 157          // pose 144 + shape 10 + cam 3
#define HMR_XC (HMR_FEAT + HMR_NSTATE)

// cv2.resize(image, (224, 224)) with the default INTER_LINEAR (run_hmr passes INTER_CUBIC as the positional `dst`, so the flag never
// reaches the interpolation argument), OpenCV's 8-bit fixed-point path: per axis the source coordinate (d + 0.5) * scale - 0.5 in
// double rounded to float, floored; 11-bit coefficients rint((1 - f) * 2048), rint(f * 2048).  Columns clamp the coordinate AND the
// weight at the borders, rows clamp only the row index.  Horizontal pass: an int sum per row; vertical pass as VResizeLinear<uchar>:
// (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.  Then /255 and Normalize(IMG_NORM_MEAN, IMG_NORM_STD) in fp32.
// One thread per output pixel (all three channels); out[n][224][224][3] NHWC.  The numpy restatement is bodyfitting_amd/hmr.py.
// The axis itself is resize_axis.h's.
extern "C" __global__ __launch_bounds__(256) void bf_hmr_resize_kernel(int n, int H, int W, double scale_y, double scale_x,
                                                                       const uint8_t *__restrict__ src, uint8_t *__restrict__ resized,
                                                                       float *__restrict__ out, float3 mean, float3 stdv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * HMR_RES * HMR_RES) return;
    const int b = i / (HMR_RES * HMR_RES), r = i % (HMR_RES * HMR_RES), dy = r / HMR_RES, dx = r % HMR_RES;
    int x0, x1, a0, a1, y0, y1, b0, b1;
    bf_resize_axis(dx, scale_x, W, 1, &x0, &x1, &a0, &a1);
    bf_resize_axis(dy, scale_y, H, 0, &y0, &y1, &b0, &b1);
    const bool edge = x0 == W - 1;            // (sx + 1 >= width: OpenCV's tail loop, S[sx] * 2048 without the second tap)
    const uint8_t *img = src + (size_t)b * H * W * 3;
    const float m[3] = {mean.x, mean.y, mean.z}, sd[3] = {stdv.x, stdv.y, stdv.z};
    for (int c = 0; c < 3; ++c) {
        const uint8_t *r0 = img + (size_t)y0 * W * 3, *r1 = img + (size_t)y1 * W * 3;
        const int h0 = edge ? r0[x0 * 3 + c] * 2048 : r0[x0 * 3 + c] * a0 + r0[x1 * 3 + c] * a1;
        const int h1 = edge ? r1[x0 * 3 + c] * 2048 : r1[x0 * 3 + c] * a0 + r1[x1 * 3 + c] * a1;
        const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        const uint8_t u = (uint8_t)v;
        if (resized) resized[(size_t)i * 3 + c] = u;
        out[(size_t)i * 3 + c] = ((float)u / 255.f - m[c]) / sd[c];
    }
}

// y[m][n] = relu?( sum_k A[m][k] W[k][n] + bias[n] + res[m][n] ): a convolution as an implicit GEMM over NHWC activations.
// M = n * Ho * Wo output pixels, N = Cout, K = kh * kw * Cin in (ky, kx, ci) order - the packed weight is [K][Cout].  Rows of y and
// res are `ldo` floats apart (Cout for a feature map; the regressor writes into a wider state row).  A 64 x 64 output tile per
// workgroup of four waves, each wave one 32 x 32 block on v_mfma_f32_32x32x2_f32, K staged through LDS 16 at a time.  Every output is
// a k-ordered fp32 fma chain from 0 whatever the tile, batch size or position, so a batch equals its single images bit for bit;
// out-of-range rows, columns, k and the spatial padding are zeros in LDS.
#define HC_BM 64
#define HC_BN 64
#define HC_BK 16

typedef float hmr_f32x16 __attribute__((ext_vector_type(16)));

extern "C" __global__ __launch_bounds__(256) void bf_hmr_conv_kernel(HmrConv p) {
    __shared__ float As[HC_BK][HC_BM + 4];
    __shared__ float Bs[HC_BK][HC_BN + 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int HoWo = p.Ho * p.Wo, M = p.n * HoWo, K = p.Cin * p.kh * p.kw;
    const int m0 = blockIdx.x * HC_BM, n0 = blockIdx.y * HC_BN;
    // the A rows this thread stages: (t >> 4) + 16 j, k = t & 15
    const int akk = t & 15;
    int a_pix[4], a_iy[4], a_ix[4];
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + (t >> 4) + 16 * j;
        if (m < M) {
            const int b = m / HoWo, r = m % HoWo, oy = r / p.Wo, ox = r % p.Wo;
            a_pix[j] = b * p.H * p.W;
            a_iy[j] = oy * p.stride - p.pad;
            a_ix[j] = ox * p.stride - p.pad;
        } else {
            a_pix[j] = -1; a_iy[j] = 0; a_ix[j] = 0;
        }
    }
    const int bn = t & 63, bk = t >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32, li = lane & 31, lk = lane >> 5;
    hmr_f32x16 acc = {};
    for (int k0 = 0; k0 < K; k0 += HC_BK) {
        const int k = k0 + akk;
        int ci = 0, kx = 0, ky = 0;
        if (k < K) { ci = k % p.Cin; const int q = k / p.Cin; kx = q % p.kw; ky = q / p.kw; }
        for (int j = 0; j < 4; ++j) {
            float v = 0.f;
            const int iy = a_iy[j] + ky, ix = a_ix[j] + kx;
            if (k < K && a_pix[j] >= 0 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                v = p.x[((size_t)a_pix[j] + (size_t)iy * p.W + ix) * p.Cin + ci];
            As[akk][(t >> 4) + 16 * j] = v;
        }
        for (int j = 0; j < 4; ++j) {
            const int kb = k0 + bk + 4 * j, nn = n0 + bn;
            Bs[bk + 4 * j][bn] = (kb < K && nn < p.Cout) ? p.w[(size_t)kb * p.Cout + nn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < HC_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + lk][wm + li], Bs[kk + lk][wn + li], acc, 0, 0, 0);
        __syncthreads();
    }
    const int nn = n0 + wn + li;
    if (nn >= p.Cout) return;
    const float bias = p.bias ? p.bias[nn] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (m >= M) continue;
        const size_t o = (size_t)m * p.ldo + nn;
        float v = acc[r] + bias;
        if (p.res) v += p.res[o];
        if (p.relu) v = fmaxf(v, 0.f);
        p.y[o] = v;
    }
}

// MaxPool2d(3, stride 2, padding 1) on NHWC (padding is -inf, as torch pads a max pool)
extern "C" __global__ __launch_bounds__(256) void bf_hmr_maxpool_kernel(int n, int H, int W, int C, int Ho, int Wo,
                                                                        const float *__restrict__ x, float *__restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * Ho * Wo * C) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((size_t)Wo * Ho));
    float v = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * 2 - 1 + dx;
            if (ix < 0 || ix >= W) continue;
            v = fmaxf(v, x[(((size_t)b * H + iy) * W + ix) * C + c]);
        }
    }
    y[i] = v;
}

// AvgPool2d(7) over the 7 x 7 layer-4 map -> xc[b][0:2048] (the feature part of the regressor's input row of HMR_XC floats)
extern "C" __global__ __launch_bounds__(256) void bf_hmr_avgpool_kernel(int n, const float *__restrict__ x, float *__restrict__ xc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * HMR_FEAT) return;
    const int b = i / HMR_FEAT, c = i % HMR_FEAT;
    float s = 0.f;
    for (int q = 0; q < 49; ++q) s += x[((size_t)b * 49 + q) * HMR_FEAT + c];
    xc[(size_t)b * HMR_XC + c] = s / 49.f;
}

// the regressor's starting state (init_pose, init_shape, init_cam) -> xc[b][2048:2205]
extern "C" __global__ __launch_bounds__(256) void bf_hmr_init_state_kernel(int n, const float *__restrict__ mean, float *__restrict__ xc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * HMR_NSTATE) return;
    const int b = i / HMR_NSTATE, j = i % HMR_NSTATE;
    xc[(size_t)b * HMR_XC + HMR_FEAT + j] = mean[j];
}
