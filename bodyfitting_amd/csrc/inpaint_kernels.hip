// The reference's texture inpainting (models/inpaint.py Inpainter, LBAMModel(4, 3); smplify/texture_fitting.py:191-214
// TextureFitting.inpaint) on gfx950: the input preparation, the encoder's attention convolutions, the reverse-attention chain and
// the decoder's transposed convolutions as implicit GEMMs on the exact-fp32 MFMA with fused epilogues and a fixed-order split-K
// reduction; the hole mask (face test, OpenCV's filled-contour rule); cv2.erode / dilate with a rectangle and the post-processing.
// Host side: inpaint_api.hip; the restatements every kernel here is held to: bodyfitting_amd/inpaint.py, tests/inpaint_cases.py.
//
// Compiled with -ffp-contract=off: every element-wise float and double operation rounds as the source writes it (torch's CPU
// kernels and numpy have no fused multiply-adds there); the one fma below is written out, as the BLAS behind numpy's `@` does it.
#include "inpaint.h"

#define IP_BM 128
#define IP_BK 16
typedef float ip_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------------------
// Inpainter.__call__'s preparation (inpaint.py:17-37) of uint8 [n][H][W][3] image and mask (255 = hole), per pixel:
// x = (image / 255 * known, known_0), known = 1 - (mask / 255 >= 0.5); mk = (known, 0); rmk = (1 - known, 0) - the encoder's
// input, the mask conv's input and the reverse chain's input, NHWC with 4 floats per pixel.  The divisions are correctly rounded
// (no fast math), so known pixels come out as the reference's float32(v / 255).
extern "C" __global__ __launch_bounds__(256) void bf_ip_prepare_kernel(long long npx, const uint8_t *__restrict__ img,
                                                                       const uint8_t *__restrict__ msk, float4 *__restrict__ x,
                                                                       float4 *__restrict__ mk, float4 *__restrict__ rmk) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    float v[3], k[3];
    for (int c = 0; c < 3; ++c) {
        const float im = (float)img[i * 3 + c] / 255.f;
        float m = (float)msk[i * 3 + c] / 255.f;
        m = m >= 0.5f ? 1.f : 0.f;
        k[c] = 1.f - m;
        v[c] = im * k[c];
    }
    x[i] = make_float4(v[0], v[1], v[2], k[0]);
    mk[i] = make_float4(k[0], k[1], k[2], 0.f);
    rmk[i] = make_float4(1.f - k[0], 1.f - k[1], 1.f - k[2], 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The epilogues (GaussActivation, MaskUpdate, LeakyReLU(0.2), tanh) in the reference's float32 operation order
__device__ __forceinline__ float ip_gauss(const IpConv &p, float x) {
    const float d = x - p.gmu, d2 = d * d;
    return x < p.gmu ? p.ga * expf(-p.gs1 * d2) : 1.f + (p.ga - 1.f) * expf(-p.gs2 * d2);
}
__device__ __forceinline__ float ip_leaky(float v) { return v > 0.f ? v : v * 0.2f; }
__device__ __forceinline__ float ip_mupdate(float v) { return powf(fmaxf(v, 0.f), 0.8f); }

// output pixel q (NHWC row of the layer's output grid), channel nn; c = the conv of x, g = the conv of xm
__device__ __forceinline__ void ip_epilogue(const IpConv &p, size_t q, int nn, float c, float g) {
    switch (p.epi) {
    case IP_EPI_RAW:
        p.y0[q * p.ld0 + nn] = c;
        if (p.y1) p.y1[q * p.ld1 + nn] = g;
        break;
    case IP_EPI_ENC: {
        const float a = ip_gauss(p, g);
        if (p.y0) p.y0[q * p.ld0 + nn] = ip_leaky(c * a);
        if (p.y1) p.y1[q * p.ld1 + nn] = ip_mupdate(g);
        break;
    }
    case IP_EPI_REV:
        p.y0[q * p.ld0 + nn] = ip_gauss(p, c);
        if (p.y1) p.y1[q * p.ld1 + nn] = ip_mupdate(c);
        break;
    case IP_EPI_DEC:
        p.y0[q * p.ld0 + nn] = ip_leaky(c * p.aux0[q * p.ldaux + nn]);
        break;
    default: {
        const float o = (tanhf(c) + 1.f) / 2.f, k = p.aux1[q * 4 + nn];
        p.y0[q * p.ld0 + nn] = o * (1.f - k) + p.aux0[q * 4 + nn] * k;
        break;
    }
    }
}

// GEMM row m of phase `phase` -> the output pixel it writes
__device__ __forceinline__ size_t ip_out_pixel(const IpConv &p, int m, int phase) {
    if (!p.deconv) return (size_t)m;
    const int HW = p.Hi * p.Wi, b = m / HW, r = m - b * HW, j = r / p.Wi, i = r - j * p.Wi;
    return ((size_t)b * p.Ho + 2 * j + (phase >> 1)) * p.Wo + 2 * i + (phase & 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The implicit GEMM (the structure of op_conv_body in openpose_kernels.hip): BM = 128 GEMM rows x BN output channels per workgroup
// of four waves, K through LDS 16 at a time, double-buffered - the next slice is read from global memory into registers while the
// MFMAs run on the current one, one barrier per slice.  Each wave owns (BM / WM) x (BN / WN) outputs of each operand as 32 x 32
// blocks of v_mfma_f32_32x32x2_f32.  Every output (or split partial) is a k-ordered fp32 chain from 0 over its K range whatever the
// tile, batch or position, and the split count depends on the per-image layer shape only, so a batch equals its single images bit
// for bit.  Out-of-range rows, columns, k and the spatial padding are zeros.  blockIdx.z = phase * splits + split.
template <int BN, int WM, bool DUAL, bool DECONV>
__device__ __forceinline__ void ip_gemm_body(const IpConv &p) {
    constexpr int WN = 4 / WM, MI = IP_BM / WM / 32, NI = BN / WN / 32, NG = DUAL ? 2 : 1;
    constexpr int BLOADS = BN / 64;                              // float4 B loads per thread, operand and slice
    // LDS: the double-buffered A and B slices, and after the K loop the accumulator tile (the epilogue's staging)
    constexpr int A_FL = NG * 2 * IP_BK * (IP_BM + 4), B_FL = NG * 2 * IP_BK * (BN + 4), T_LD = BN + 1, T_FL = NG * IP_BM * T_LD;
    __shared__ __attribute__((aligned(16))) float smem[A_FL + B_FL > T_FL ? A_FL + B_FL : T_FL];
    auto As = reinterpret_cast<float(*)[2][IP_BK][IP_BM + 4]>(smem);
    auto Bs = reinterpret_cast<float(*)[2][IP_BK][BN + 4]>(smem + A_FL);
    const int n0 = blockIdx.y * BN;
    if (n0 >= p.cout) return;
    const int phase = DECONV ? (int)blockIdx.z / p.splits : 0, sp = (int)blockIdx.z - phase * p.splits;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int gh = DECONV ? p.Hi : p.Ho, gw = DECONV ? p.Wi : p.Wo;
    const int HWg = gh * gw, M = p.n * HWg, K = p.cin * (DECONV ? 4 : 16);
    const int kb0 = sp * p.kper, kb1 = min(K, kb0 + p.kper);
    const int m0 = blockIdx.x * IP_BM;
    const float *xg[2] = {p.x, DUAL ? p.xm : p.x};
    const int ldg[2] = {p.ldx, DUAL ? p.ldxm : p.ldx};
    const float *wg[2] = {p.w + (size_t)phase * K * p.coutp, DUAL ? p.wm : p.w};
    // A staging: float4 kq (k = 4 kq .. 4 kq + 3 of the slice) of rows r0 and r0 + 64; the tap origin of each row
    const int kq = t & 3, r0 = t >> 2;
    int a_base[2], a_y[2], a_x[2];
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + r0 + 64 * j;
        if (m < M) {
            const int b = m / HWg, r = m - b * HWg, oy = r / gw, ox = r - oy * gw;
            a_base[j] = b * p.Hi * p.Wi;
            a_y[j] = DECONV ? oy : 2 * oy - 1;
            a_x[j] = DECONV ? ox : 2 * ox - 1;
        } else {
            a_base[j] = -1; a_y[j] = 0; a_x[j] = 0;
        }
    }
    const int py = phase >> 1, px = phase & 1;
    const int bn4 = t % (BN / 4), bk = t / (BN / 4);
    constexpr int BROWS = 256 / (BN / 4);
    float4 ra[NG][2], rb[NG][BLOADS];
    auto load = [&](int k0) {
        const int k = k0 + 4 * kq;
        int ci = 0, dy = 0, dx = 0;
        if (k < kb1) {
            const int tap = k / p.cin;
            ci = k - tap * p.cin;
            if (DECONV) {
                const int ty = tap >> 1, tx = tap & 1;                 // inpaint.py DY: (0, -1) for even rows, (1, 0) for odd
                dy = py ? 1 - ty : -ty;
                dx = px ? 1 - tx : -tx;
            } else {
                dy = tap >> 2; dx = tap & 3;
            }
        }
        for (int j = 0; j < 2; ++j) {
            const int iy = a_y[j] + dy, ix = a_x[j] + dx;
            const bool ok = k < kb1 && a_base[j] >= 0 && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
            for (int g = 0; g < NG; ++g) {
                ra[g][j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) ra[g][j] = *(const float4 *)(xg[g] + ((size_t)a_base[j] + (size_t)iy * p.Wi + ix) * ldg[g] + ci);
            }
        }
        for (int j = 0; j < BLOADS; ++j) {
            const int kb = k0 + bk + BROWS * j, nn = n0 + 4 * bn4;
            for (int g = 0; g < NG; ++g) {
                rb[g][j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kb < kb1 && nn < p.coutp) rb[g][j] = *(const float4 *)(wg[g] + (size_t)kb * p.coutp + nn);
            }
        }
    };
    auto store = [&](int buf) {
        for (int g = 0; g < NG; ++g) {
            for (int j = 0; j < 2; ++j) {
                const int row = r0 + 64 * j;
                As[g][buf][4 * kq + 0][row] = ra[g][j].x;
                As[g][buf][4 * kq + 1][row] = ra[g][j].y;
                As[g][buf][4 * kq + 2][row] = ra[g][j].z;
                As[g][buf][4 * kq + 3][row] = ra[g][j].w;
            }
            for (int j = 0; j < BLOADS; ++j) *(float4 *)&Bs[g][buf][bk + BROWS * j][4 * bn4] = rb[g][j];
        }
    };
    const int wm = (wave % WM) * (IP_BM / WM), wn = (wave / WM) * (BN / WN), li = lane & 31, lk = lane >> 5;
    ip_f32x16 acc[NG][MI][NI];
    for (int g = 0; g < NG; ++g)
        for (int i = 0; i < MI; ++i)
            for (int j = 0; j < NI; ++j) acc[g][i][j] = ip_f32x16{};
    load(kb0);
    store(0);
    __syncthreads();
    int cur = 0;
    for (int k0 = kb0; k0 < kb1; k0 += IP_BK) {
        const bool more = k0 + IP_BK < kb1;
        if (more) load(k0 + IP_BK);
#pragma unroll
        for (int kk = 0; kk < IP_BK; kk += 2) {
            for (int g = 0; g < NG; ++g) {
                float a[MI], bv[NI];
                for (int i = 0; i < MI; ++i) a[i] = As[g][cur][kk + lk][wm + 32 * i + li];
                for (int j = 0; j < NI; ++j) bv[j] = Bs[g][cur][kk + lk][wn + 32 * j + li];
                for (int i = 0; i < MI; ++i)
                    for (int j = 0; j < NI; ++j) acc[g][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[j], acc[g][i][j], 0, 0, 0);
            }
        }
        if (more) store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // the epilogue runs once per element from the staged tile (not unrolled over the accumulators: GaussActivation, pow and tanh
    // inlined 64 times cost registers and scratch), a row's channels on consecutive lanes
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    smem[(g * IP_BM + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk) * T_LD + wn + 32 * j + li] = acc[g][i][j][r];
    __syncthreads();
    const size_t plane = (size_t)M * p.coutp, gstride = plane * p.splits * (DECONV ? 4 : 1);
    float *part = p.part + ((size_t)phase * p.splits + sp) * plane;
#pragma unroll 1
    for (int e = t; e < IP_BM * BN; e += 256) {
        const int row = e / BN, col = e - row * BN, m = m0 + row, nn = n0 + col;
        if (m >= M || nn >= p.cout) continue;
        const float c = smem[row * T_LD + col], g = DUAL ? smem[(IP_BM + row) * T_LD + col] : 0.f;
        if (p.splits > 1) {
            part[(size_t)m * p.coutp + nn] = c;
            if (DUAL) part[gstride + (size_t)m * p.coutp + nn] = g;
        } else {
            ip_epilogue(p, ip_out_pixel(p, m, phase), nn, c, g);
        }
    }
}

extern "C" __global__ __launch_bounds__(256) void bf_ip_enc_kernel(IpConv p) { ip_gemm_body<64, 4, true, false>(p); }
extern "C" __global__ __launch_bounds__(256) void bf_ip_rev128_kernel(IpConv p) { ip_gemm_body<128, 2, false, false>(p); }
extern "C" __global__ __launch_bounds__(256) void bf_ip_rev64_kernel(IpConv p) { ip_gemm_body<64, 4, false, false>(p); }
extern "C" __global__ __launch_bounds__(256) void bf_ip_dec128_kernel(IpConv p) { ip_gemm_body<128, 2, false, true>(p); }
extern "C" __global__ __launch_bounds__(256) void bf_ip_dec64_kernel(IpConv p) { ip_gemm_body<64, 4, false, true>(p); }

// the split-K reduction: per (phase, GEMM row, channel) the partials of splits 0, 1, ... added in that order, then the epilogue
extern "C" __global__ __launch_bounds__(256) void bf_ip_reduce_kernel(IpConv p, int dual) {
    const int phases = p.deconv ? 4 : 1;
    const int M = p.n * (p.deconv ? p.Hi * p.Wi : p.Ho * p.Wo);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)phases * M * p.cout) return;
    const int nn = (int)(i % p.cout);
    const long long rest = i / p.cout;
    const int m = (int)(rest % M), phase = (int)(rest / M);
    const size_t plane = (size_t)M * p.coutp, gstride = plane * p.splits * phases;
    const float *part = p.part + (size_t)phase * p.splits * plane + (size_t)m * p.coutp + nn;
    float c = part[0], g = dual ? part[gstride] : 0.f;
    for (int s = 1; s < p.splits; ++s) {
        c += part[s * plane];
        if (dual) g += part[gstride + s * plane];
    }
    ip_epilogue(p, ip_out_pixel(p, m, phase), nn, c, g);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// TextureFitting.inpaint's face test (texture_fitting.py:196-204), one thread per face: the 63 samples (dims @ face) of the float32
// pixel-space UV triangle uv[f][3][2], in float64 as fma(d2, u2, fma(d1, u1, d0 * u0)) - what numpy's matmul computes through its
// BLAS - truncated to int; numpy's indexing of img[y, x] (a negative index wraps, one out of [-size, size) raises: *err = 1); a
// sample is grey when all three channels lie strictly between 118 and 138; sel[f] = more than 63 / 6 grey samples.
extern "C" __global__ __launch_bounds__(256) void bf_ip_faces_kernel(int n_faces, int H, int W, const uint8_t *__restrict__ img,
                                                                     const float *__restrict__ uv, uint8_t *__restrict__ sel,
                                                                     int *__restrict__ err) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces) return;
    double u[3], v[3];
    for (int k = 0; k < 3; ++k) { u[k] = (double)uv[f * 6 + 2 * k]; v[k] = (double)uv[f * 6 + 2 * k + 1]; }
    int grey = 0;
    bool bad = false;
    for (int r = 1; r < 64; ++r) {
        const int a = r >> 4, b = (r >> 2) & 3, c = r & 3;
        const double s = (double)(a + b + c);
        const double d0 = (double)a / s, d1 = (double)b / s, d2 = (double)c / s;
        int x = (int)fma(d2, u[2], fma(d1, u[1], d0 * u[0]));
        int y = (int)fma(d2, v[2], fma(d1, v[1], d0 * v[0]));
        if (x < -W || x >= W || y < -H || y >= H) { bad = true; continue; }
        if (x < 0) x += W;
        if (y < 0) y += H;
        const uint8_t *q = img + ((size_t)y * W + x) * 3;
        grey += q[0] > 118 && q[0] < 138 && q[1] > 118 && q[1] < 138 && q[2] > 118 && q[2] < 138;
    }
    if (bad) *err = 1;
    sel[f] = grey * 6 > 63;
}

// OpenCV 4.1.2 clipLine(Size2l, Point2l&, Point2l&) -> inside
__device__ bool ip_clip_line(int W, int H, long long &x1, long long &y1, long long &x2, long long &y2) {
    const long long right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (x2 - x1) / (y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (x2 - x1) / (y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (y2 - y1) / (x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (y2 - y1) / (x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

__device__ __forceinline__ void ip_set(uint8_t *mask, int H, int W, long long x, long long y) {
    if (x < 0 || x >= W || y < 0 || y >= H) return;            // clipping keeps every pixel inside; this guards the memory alone
    uint8_t *q = mask + ((size_t)y * W + x) * 3;
    q[0] = 255; q[1] = 255; q[2] = 255;
}

// OpenCV's Line(img, p1, p2, color, 8): the 8-connected LineIterator (leftToRight) over the clipped segment
__device__ void ip_line8(uint8_t *mask, int H, int W, long long x1, long long y1, long long x2, long long y2) {
    if (x1 < 0 || x1 >= W || x2 < 0 || x2 >= W || y1 < 0 || y1 >= H || y2 < 0 || y2 >= H)
        if (!ip_clip_line(W, H, x1, y1, x2, y2)) return;
    long long dx = x2 - x1, dy = y2 - y1;
    if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }
    const long long sy = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    const bool ymaj = dy > dx;
    const long long dmaj = ymaj ? dy : dx, dmin = ymaj ? dx : dy;
    const long long majx = ymaj ? 0 : 1, majy = ymaj ? sy : 0, mnx = ymaj ? 1 : 0, mny = ymaj ? 0 : sy;
    long long err = dmaj - 2 * dmin, x = x1, y = y1;
    for (long long i = 0; i <= dmaj; ++i) {
        ip_set(mask, H, W, x, y);
        const bool step = err < 0;
        err += -2 * dmin + (step ? 2 * dmaj : 0);
        x += majx + (step ? mnx : 0);
        y += majy + (step ? mny : 0);
    }
}

// cv2.drawContours(mask, [face.astype(int32)], 0, 255, -1) of every selected face (texture_fitting.py:204-205), one thread per face:
// CollectPolyEdges' Line over the closed contour p0 p1 p2 p0 (from p0 -> p0) and its 16.16 edges, FillEdgeCollection's spans
// (x_left + 0xFFFF) >> 16 .. x_right >> 16 on rows y0 <= y < y1 of the two active edges, clipped.  Every writer stores 255 to
// all three channels, so overlapping faces give the same bytes in any order.  inpaint.py fill_triangle is the restatement.
extern "C" __global__ __launch_bounds__(256) void bf_ip_fill_kernel(int n_faces, int H, int W, const float *__restrict__ uv,
                                                                    const uint8_t *__restrict__ sel, uint8_t *__restrict__ mask) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces || !sel[f]) return;
    long long px[4], py[4];
    for (int k = 0; k < 3; ++k) { px[k] = (int)uv[f * 6 + 2 * k]; py[k] = (int)uv[f * 6 + 2 * k + 1]; }
    px[3] = px[0]; py[3] = py[0];
    long long ey0[3], ey1[3], ex[3], edx[3];
    int ne = 0;
    long long x0 = px[0], y0 = py[0];
    for (int k = 0; k < 4; ++k) {
        const long long x1 = px[k], y1 = py[k];
        ip_line8(mask, H, W, x0, y0, x1, y1);
        if (y0 != y1 && ne < 3) {
            const bool down = y0 < y1;
            ey0[ne] = down ? y0 : y1;
            ey1[ne] = down ? y1 : y0;
            ex[ne] = (down ? x0 : x1) * 65536;
            edx[ne] = (x1 * 65536 - x0 * 65536) / (y1 - y0);        // C's truncating division, as OpenCV's int64
            ++ne;
        }
        x0 = x1; y0 = y1;
    }
    if (ne < 2) return;
    long long ymin = ey0[0], ymax = ey1[0];
    for (int e = 1; e < ne; ++e) { ymin = min(ymin, ey0[e]); ymax = max(ymax, ey1[e]); }
    ymax = min(ymax, (long long)H);
    for (long long y = max(ymin, 0LL); y < ymax; ++y) {
        long long xs[2];
        int na = 0;
        for (int e = 0; e < ne; ++e)
            if (ey0[e] <= y && y < ey1[e] && na < 2) xs[na++] = ex[e] + (y - ey0[e]) * edx[e];
        if (na != 2) continue;
        long long x1 = (min(xs[0], xs[1]) + 65535) >> 16, x2 = max(xs[0], xs[1]) >> 16;
        if (x1 < W && x2 >= 0) {
            x1 = max(x1, 0LL);
            x2 = min(x2, (long long)W - 1);
            for (long long x = x1; x <= x2; ++x) ip_set(mask, H, W, x, y);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cv2.erode (op 0) / cv2.dilate (op 1) with np.ones((k, k)) on uint8 [n][H][W][C], anchor at the centre, pixels outside the image
// ignored (OpenCV's default border value for morphology): one output byte per thread, the k x k window read directly
extern "C" __global__ __launch_bounds__(256) void bf_ip_morph_kernel(int op, int k, int n, int H, int W, int C,
                                                                     const uint8_t *__restrict__ in, uint8_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * H * W * C) return;
    const int c = (int)(i % C);
    const long long q = i / C;
    const int x = (int)(q % W), y = (int)((q / W) % H);
    const long long b = q / ((long long)W * H);
    const int r = k / 2;
    const int y0 = max(y - r, 0), y1 = min(y - r + k - 1, H - 1), x0 = max(x - r, 0), x1 = min(x - r + k - 1, W - 1);
    int v = op ? 0 : 255;
    for (int yy = y0; yy <= y1; ++yy) {
        const uint8_t *row = in + ((b * H + yy) * W) * C + c;
        for (int xx = x0; xx <= x1; ++xx) {
            const int s = row[(size_t)xx * C];
            v = op ? max(v, s) : min(v, s);
        }
    }
    out[i] = (uint8_t)v;
}

// texture_fitting.py:207-209: img = (out * 255).astype(uint8) (float32, truncated), mask = 1 - (img == 255)
extern "C" __global__ __launch_bounds__(256) void bf_ip_quantize_kernel(long long count, const float *__restrict__ out,
                                                                        uint8_t *__restrict__ img, uint8_t *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t v = (uint8_t)(int)(out[i] * 255.f);
    img[i] = v;
    mask[i] = v == 255 ? 0 : 1;
}

// texture_fitting.py:213-214 in uint8: mask * img + (mask_d - mask) * img2 + (1 - mask_d) * img
extern "C" __global__ __launch_bounds__(256) void bf_ip_combine_kernel(long long count, const uint8_t *__restrict__ img,
                                                                       const uint8_t *__restrict__ img2, const uint8_t *__restrict__ mask,
                                                                       const uint8_t *__restrict__ mask_d, uint8_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t m = mask[i], md = mask_d[i], a = img[i], b = img2[i];
    out[i] = (uint8_t)(m * a + (uint8_t)(md - m) * b + (uint8_t)(1 - md) * a);
}
