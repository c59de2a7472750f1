// The reference's OpenPose body estimator (openpose/body.py Body.__call__, openpose/model.py bodypose_model) on gfx950: the cv2
// INTER_CUBIC image pipeline, the network's convolutions as one implicit-GEMM kernel on the exact-fp32 MFMA, the map resizes and
// the scale accumulation, scipy's Gaussian filter, the peak test and the limb scoring.  Host side: openpose_api.hip; the numpy
// restatements every kernel here is held to: bodyfitting_amd/openpose.py.
//
// Compiled with -ffp-contract=off: every float and double operation rounds as the source writes it (OpenCV's and numpy's
// arithmetic has no fused multiply-adds).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "openpose_device.h"
#include "openpose_kernels.h"

#define OP_NPAF 38
#define OP_NHEAT 19
#define OP_NOUT 57
#define OP_NPART 18
#define OP_GR 12                  // scipy's radius int(4 * sigma + 0.5) for sigma = 3

// body.py:73-75 for one scale: cv2.resize(img, fx=s, fy=s, INTER_CUBIC) on uint8 BGR through OpenCV's fixed-point path (coefficients
// saturate_cast<short>(c * 2048), an int horizontal sum per source row, then (sum_k h_k * b_k + 2^21) >> 22 saturated to uchar),
// padRightDownCorner with 128, then / 256 - 0.5.  out[n][Hp][Wp][4] NHWC, channel 3 zero.  One thread per padded pixel.
extern "C" __global__ __launch_bounds__(256) void bf_op_input_kernel(int n, int H, int W, int Hs, int Ws, int Hp, int Wp, double scale,
                                                                     const uint8_t *__restrict__ src, float4 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * Hp * Wp) return;
    const int x = (int)(i % Wp), y = (int)((i / Wp) % Hp), b = (int)(i / ((long long)Wp * Hp));
    float v[3] = {0.f, 0.f, 0.f};
    if (y < Hs && x < Ws) {
        int xi[4], yi[4], xa[4], ya[4];
        float cx[4], cy[4];
        op_axis(x, scale, W, xi, cx);
        op_axis(y, scale, H, yi, cy);
        for (int j = 0; j < 4; ++j) { xa[j] = (int)rintf(cx[j] * 2048.f); ya[j] = (int)rintf(cy[j] * 2048.f); }
        const uint8_t *img = src + (size_t)b * H * W * 3;
        for (int c = 0; c < 3; ++c) {
            int acc = 0;
            for (int r = 0; r < 4; ++r) {
                const uint8_t *row = img + (size_t)yi[r] * W * 3;
                int h = 0;
                for (int j = 0; j < 4; ++j) h += row[xi[j] * 3 + c] * xa[j];
                acc += h * ya[r];
            }
            const int u = min(max((acc + (1 << 21)) >> 22, 0), 255);
            v[c] = (float)u / 256.f - 0.5f;
        }
    } else {
        for (int c = 0; c < 3; ++c) v[c] = 128.f / 256.f - 0.5f;
    }
    out[i] = make_float4(v[0], v[1], v[2], 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Convolution, stride 1, 'same' padding (k / 2), NHWC: y[m][n] = relu?(sum_k A[m][k] W[k][n] + bias[n]) as an implicit GEMM with
// M = n * H * W pixels, N = cout, K = k * k * cin in (ky, kx, ci) order, the packed weight [K][coutp] (coutp = cout rounded up to 4,
// zero columns).  Input pixel rows are `ldx` floats apart and output rows `ldo` apart, so a layer can read a channel slice of a
// wider buffer and write into one (the stage concat).  cin and ldx are multiples of 4 and the slice 16-byte aligned: A and B are
// staged with 16-byte loads.  Up to two independent convolutions of the same pixel grid run as one launch (blockIdx.z): the L1 and
// L2 branches of a stage.
//
// Tiles: BM = 128 pixels x BN (128 or 64) channels per workgroup of four waves, K through LDS 16 at a time, double-buffered - the
// next slice is read from global memory into registers while the MFMAs run on the current one, one barrier per slice.  Each
// wave owns (BM / WM) x (BN / WN) outputs as 32 x 32 blocks of v_mfma_f32_32x32x2_f32.  Every output is a k-ordered fp32 chain
// from 0 whatever the tile, batch size or position, so a batch equals its single images bit for bit; out-of-range rows, columns,
// k and the spatial padding are zeros.
#define OC_BM 128
#define OC_BK 16
typedef float op_f32x16 __attribute__((ext_vector_type(16)));

template <int BN, int WM>
__device__ __forceinline__ void op_conv_body(const OpConvLaunch &L) {
    constexpr int WN = 4 / WM, MI = OC_BM / WM / 32, NI = BN / WN / 32;
    constexpr int BLOADS = BN / 64;                              // float4 B loads per thread per slice
    __shared__ __attribute__((aligned(16))) float As[2][OC_BK][OC_BM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[2][OC_BK][BN + 4];
    const OpConv p = L.g[blockIdx.z];
    const int n0 = blockIdx.y * BN;
    if (n0 >= p.cout) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int HW = L.H * L.W, M = L.n * HW, K = p.cin * p.k * p.k, pad = p.k >> 1;
    const int m0 = blockIdx.x * OC_BM;
    // A staging: float4 kq (k = 4 kq .. 4 kq + 3 of the slice) of rows r0 and r0 + 64
    const int kq = t & 3, r0 = t >> 2;
    int a_base[2], a_y[2], a_x[2];
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + r0 + 64 * j;
        if (m < M) {
            const int b = m / HW, r = m - b * HW, oy = r / L.W;
            a_base[j] = b * HW; a_y[j] = oy; a_x[j] = r - oy * L.W;
        } else {
            a_base[j] = -1; a_y[j] = 0; a_x[j] = 0;
        }
    }
    // B staging: float4 column group bn4, rows bk + 64 / (BN / 4) * j
    const int bn4 = t % (BN / 4), bk = t / (BN / 4);
    constexpr int BROWS = 256 / (BN / 4);
    float4 ra[2], rb[BLOADS];
    auto load = [&](int k0) {
        const int k = k0 + 4 * kq;
        int ci = 0, ky = 0, kx = 0;
        if (k < K) { const int tap = k / p.cin; ci = k - tap * p.cin; ky = tap / p.k; kx = tap - ky * p.k; }
        for (int j = 0; j < 2; ++j) {
            const int iy = a_y[j] + ky - pad, ix = a_x[j] + kx - pad;
            ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < K && a_base[j] >= 0 && iy >= 0 && iy < L.H && ix >= 0 && ix < L.W)
                ra[j] = *(const float4 *)(p.x + ((size_t)a_base[j] + (size_t)iy * L.W + ix) * p.ldx + ci);
        }
        for (int j = 0; j < BLOADS; ++j) {
            const int kb = k0 + bk + BROWS * j, nn = n0 + 4 * bn4;
            rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kb < K && nn < p.coutp) rb[j] = *(const float4 *)(p.w + (size_t)kb * p.coutp + nn);
        }
    };
    auto store = [&](int buf) {
        for (int j = 0; j < 2; ++j) {
            const int row = r0 + 64 * j;
            As[buf][4 * kq + 0][row] = ra[j].x;
            As[buf][4 * kq + 1][row] = ra[j].y;
            As[buf][4 * kq + 2][row] = ra[j].z;
            As[buf][4 * kq + 3][row] = ra[j].w;
        }
        for (int j = 0; j < BLOADS; ++j) *(float4 *)&Bs[buf][bk + BROWS * j][4 * bn4] = rb[j];
    };
    const int wm = (wave % WM) * (OC_BM / WM), wn = (wave / WM) * (BN / WN), li = lane & 31, lk = lane >> 5;
    op_f32x16 acc[MI][NI];
    for (int i = 0; i < MI; ++i)
        for (int j = 0; j < NI; ++j) acc[i][j] = op_f32x16{};
    load(0);
    store(0);
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < K; k0 += OC_BK) {
        const bool more = k0 + OC_BK < K;
        if (more) load(k0 + OC_BK);
#pragma unroll
        for (int kk = 0; kk < OC_BK; kk += 2) {
            float a[MI], bv[NI];
            for (int i = 0; i < MI; ++i) a[i] = As[cur][kk + lk][wm + 32 * i + li];
            for (int j = 0; j < NI; ++j) bv[j] = Bs[cur][kk + lk][wn + 32 * j + li];
            for (int i = 0; i < MI; ++i)
                for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    for (int j = 0; j < NI; ++j) {
        const int nn = n0 + wn + 32 * j + li;
        if (nn >= p.cout) continue;
        const float bias = p.bias[nn];
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m >= M) continue;
                float v = acc[i][j][r] + bias;
                if (p.relu) v = fmaxf(v, 0.f);
                p.y[(size_t)m * p.ldo + nn] = v;
            }
    }
}

extern "C" __global__ __launch_bounds__(256) void bf_op_conv128_kernel(OpConvLaunch L) { op_conv_body<128, 2>(L); }
extern "C" __global__ __launch_bounds__(256) void bf_op_conv64_kernel(OpConvLaunch L) { op_conv_body<64, 4>(L); }
// the stages' 7 x 7 layers: the same code under its own name, so a kernel trace times them apart
extern "C" __global__ __launch_bounds__(256) void bf_op_conv7_kernel(OpConvLaunch L) { op_conv_body<128, 2>(L); }

// MaxPool2d(2, 2) on NHWC with C a multiple of 4 (H, W even: the padded input is a multiple of 8)
extern "C" __global__ __launch_bounds__(256) void bf_op_pool_kernel(int n, int H, int W, int C, const float4 *__restrict__ x,
                                                                    float4 *__restrict__ y) {
    const int C4 = C / 4, Ho = H / 2, Wo = W / 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * Ho * Wo * C4) return;
    const int c = (int)(i % C4);
    const long long q = i / C4;
    const int ox = (int)(q % Wo), oy = (int)((q / Wo) % Ho), b = (int)(q / ((long long)Wo * Ho));
    const float4 *base = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C4 + c;
    const float4 a0 = base[0], a1 = base[C4], a2 = base[(size_t)W * C4], a3 = base[(size_t)W * C4 + C4];
    float4 v;
    v.x = fmaxf(fmaxf(a0.x, a1.x), fmaxf(a2.x, a3.x));
    v.y = fmaxf(fmaxf(a0.y, a1.y), fmaxf(a2.y, a3.y));
    v.z = fmaxf(fmaxf(a0.z, a1.z), fmaxf(a2.z, a3.z));
    v.w = fmaxf(fmaxf(a0.w, a1.w), fmaxf(a2.w, a3.w));
    y[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// body.py:88-102 for one scale, as OpenCV runs each resize - a horizontal pass per source row, then a vertical one, each
// ((S0 a0 + S1 a1) + S2 a2) + S3 a3 in float - in two kernels of one output element per thread.
// bf_op_up8_kernel: the float cv2.resize(fx=8, fy=8, INTER_CUBIC) of the network output out[b][hq][wq][57] (paf 0:38, heat 38:57),
// only its [h][w] crop (the resized image without the padding) -> up[b][h][w][57].
extern "C" __global__ __launch_bounds__(256) void bf_op_up8_kernel(int n, int h, int w, int hq, int wq, const float *__restrict__ out,
                                                                   float *__restrict__ up) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * h * w * OP_NOUT) return;
    const int c = (int)(i % OP_NOUT);
    const long long q = i / OP_NOUT;
    const int x = (int)(q % w), y = (int)((q / w) % h), b = (int)(q / ((long long)w * h));
    int rx[4], ry[4];
    float cx[4], cy[4];
    op_axis(x, 0.125, wq, rx, cx);
    op_axis(y, 0.125, hq, ry, cy);
    const float *o = out + (size_t)b * hq * wq * OP_NOUT + c;
    float v = 0.f;
    for (int r = 0; r < 4; ++r) {
        const float *row = o + (size_t)ry[r] * wq * OP_NOUT;
        float hh = row[(size_t)rx[0] * OP_NOUT] * cx[0];
        hh = hh + row[(size_t)rx[1] * OP_NOUT] * cx[1];
        hh = hh + row[(size_t)rx[2] * OP_NOUT] * cx[2];
        hh = hh + row[(size_t)rx[3] * OP_NOUT] * cx[3];
        v = r == 0 ? hh * cy[0] : v + hh * cy[r];
    }
    up[i] = v;
}

// bf_op_maps_kernel: the cubic resize of up[b][h][w][57] to the original [H][W] (sy2 / sx2 = 1 / (H / h), 1 / (W / w), cv2's scale
// for a dsize), then heatmap_avg += heatmap_avg + heatmap / 4 and paf_avg += paf / 4 in double (heatmap / 4 in float, as numpy
// divides a float32 array).  heat[b][H][W][19], paf[b][H][W][38].
extern "C" __global__ __launch_bounds__(256) void bf_op_maps_kernel(int n, int H, int W, int h, int w, double sy2, double sx2,
                                                                    const float *__restrict__ up, double *__restrict__ heat,
                                                                    double *__restrict__ paf) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * H * W * OP_NOUT) return;
    const int c = (int)(i % OP_NOUT);
    const long long q = i / OP_NOUT;
    const int x = (int)(q % W), y = (int)((q / W) % H), b = (int)(q / ((long long)W * H));
    int rx[4], ry[4];
    float cx[4], cy[4];
    op_axis(x, sx2, w, rx, cx);
    op_axis(y, sy2, h, ry, cy);
    const float *o = up + (size_t)b * h * w * OP_NOUT + c;
    float v = 0.f;
    for (int r = 0; r < 4; ++r) {
        const float *row = o + (size_t)ry[r] * w * OP_NOUT;
        float hh = row[(size_t)rx[0] * OP_NOUT] * cx[0];
        hh = hh + row[(size_t)rx[1] * OP_NOUT] * cx[1];
        hh = hh + row[(size_t)rx[2] * OP_NOUT] * cx[2];
        hh = hh + row[(size_t)rx[3] * OP_NOUT] * cx[3];
        v = r == 0 ? hh * cy[0] : v + hh * cy[r];
    }
    const float quarter = v / 4.f;
    if (c < OP_NPAF) {
        double *d = paf + q * OP_NPAF + c;
        *d = *d + (double)quarter;
    } else {
        double *d = heat + q * OP_NHEAT + (c - OP_NPAF);
        const double old = *d;
        *d = old + (old + (double)quarter);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// scipy.ndimage.gaussian_filter(heatmap_avg[:, :, part], sigma=3) for the 18 parts: correlate1d along axis 0, then axis 1, with
// NI_Correlate1D's symmetric summation - out = x[i] w0, then out += (x[i - j] + x[i + j]) w_j for j = 12 .. 1 - and mode
// 'reflect' (d c b a | a b c d | d c b a; one reflection suffices for lines of 13 or more).  The weights are
// _gaussian_kernel1d(3, 0, 12) as numpy computes them (exp, then / sum), w_0 first.
__constant__ double op_gauss_w[OP_GR + 1] = {
    0x1.105a329f98197p-3, 0x1.01a25f86eb137p-3, 0x1.b42a57d56c0bep-4, 0x1.4a614d1afd337p-4, 0x1.bfde9c12bec92p-5,
    0x1.0fa58939b528fp-5, 0x1.26defcaeb0202p-6, 0x1.1e6bccad344bap-7, 0x1.f1e9915139406p-9, 0x1.8345966f69518p-10,
    0x1.0d8a5ad43c165p-11, 0x1.4fbe39149e277p-13, 0x1.763a210dfb306p-15};

// src[b][H][W][src_c] channels 0..17 -> dst[b][H][W][18]; axis 0 runs along y, 1 along x
extern "C" __global__ __launch_bounds__(256) void bf_op_gauss_kernel(int n, int H, int W, int axis, int src_c, const double *__restrict__ src,
                                                                     double *__restrict__ dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * H * W * OP_NPART) return;
    const int c = (int)(i % OP_NPART);
    const long long q = i / OP_NPART;
    const int x = (int)(q % W), y = (int)((q / W) % H), b = (int)(q / ((long long)W * H));
    const double *img = src + (size_t)b * H * W * src_c + c;
    auto at = [&](int yy, int xx) { return img[((size_t)yy * W + xx) * src_c]; };
    double v = at(y, x) * op_gauss_w[0];
    for (int j = OP_GR; j >= 1; --j) {
        const double s = axis == 0 ? at(op_reflect(y - j, H), x) + at(op_reflect(y + j, H), x)
                                   : at(y, op_reflect(x - j, W)) + at(y, op_reflect(x + j, W));
        v = v + s * op_gauss_w[j];
    }
    dst[i] = v;
}

// body.py:113-121: a peak where the filtered map is > 0.1 and >= its four neighbours (0 outside the image); appended as (x, y, part)
// with the unfiltered heatmap_avg value as its score.  The host puts each view's list into np.nonzero's order.
extern "C" __global__ __launch_bounds__(256) void bf_op_peaks_kernel(int n, int H, int W, const double *__restrict__ bl,
                                                                     const double *__restrict__ heat, int cap, int *__restrict__ count,
                                                                     int *__restrict__ peaks, double *__restrict__ scores) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * H * W * OP_NPART) return;
    const int c = (int)(i % OP_NPART);
    const long long q = i / OP_NPART;
    const int x = (int)(q % W), y = (int)((q / W) % H), b = (int)(q / ((long long)W * H));
    const double v = bl[i];
    if (!(v > 0.1)) return;
    const size_t row = (size_t)W * OP_NPART;
    if (y > 0 && !(v >= bl[i - row])) return;
    if (y < H - 1 && !(v >= bl[i + row])) return;
    if (x > 0 && !(v >= bl[i - OP_NPART])) return;
    if (x < W - 1 && !(v >= bl[i + OP_NPART])) return;
    const int slot = atomicAdd(count + b, 1);
    if (slot >= cap) return;
    int *pk = peaks + ((size_t)b * cap + slot) * 3;
    pk[0] = x; pk[1] = y; pk[2] = c;
    scores[(size_t)b * cap + slot] = heat[q * OP_NHEAT + c];
}

// body.py:143-163 for one (limb k, candidate pair): job = (k, ax, ay, bx, by) -> score_with_dist_prior and the number of the 100
// samples above thre2 (criterion1 is count > 80, criterion2 score > 0).  np.linspace as numpy computes it (arange * step + start,
// the last sample = stop), Python's round (half to even), the builtin sequential sum; all in double.  paf[H][W][38] of one view.
__constant__ int op_map_idx[19][2] = {{12, 13}, {20, 21}, {14, 15}, {16, 17}, {22, 23}, {24, 25}, {0, 1}, {2, 3}, {4, 5}, {6, 7},
                                      {8, 9}, {10, 11}, {28, 29}, {30, 31}, {34, 35}, {32, 33}, {36, 37}, {18, 19}, {26, 27}};

extern "C" __global__ __launch_bounds__(64) void bf_op_pairs_kernel(int npairs, int H, int W, const double *__restrict__ paf,
                                                                    const int *__restrict__ jobs, double *__restrict__ score,
                                                                    int *__restrict__ above) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const int *jb = jobs + 5 * i;
    const int k = jb[0], ax = jb[1], ay = jb[2], bx = jb[3], by = jb[4];
    const int vx = bx - ax, vy = by - ay;
    double norm = __dsqrt_rn((double)((long long)vx * vx + (long long)vy * vy));
    if (norm == 0.0) norm = 0.1;
    const double ux = (double)vx / norm, uy = (double)vy / norm;
    const double dx = (double)vx, dy = (double)vy, stx = dx / 99, sty = dy / 99;
    const int cx = op_map_idx[k][0], cy = op_map_idx[k][1];
    double sum = 0.0;
    int cnt = 0;
    for (int s = 0; s < 100; ++s) {
        double px, py;
        if (s == 99) { px = (double)bx; py = (double)by; }
        else {
            px = (stx == 0.0 ? (double)s / 99 * dx : (double)s * stx) + (double)ax;
            py = (sty == 0.0 ? (double)s / 99 * dy : (double)s * sty) + (double)ay;
        }
        const int xi = (int)rint(px), yi = (int)rint(py);
        const double *pp = paf + ((size_t)yi * W + xi) * OP_NPAF;
        const double m = pp[cx] * ux + pp[cy] * uy;
        sum = s == 0 ? m : sum + m;
        cnt += m > 0.05;
    }
    const double prior = 0.5 * (double)H / norm - 1.0;
    score[i] = sum / 100 + (prior < 0.0 ? prior : 0.0);
    above[i] = cnt;
}
