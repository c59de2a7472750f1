// The reference's OpenPose hand estimator (openpose/hand.py Hand.__call__) on gfx950, around the body estimator's convolution and
// pool kernels (openpose_kernels.hip): the per-crop input resize, the per-crop map resizes and the scale accumulation, scipy's
// Gaussian filter on each crop's 21 parts, and the component pick - skimage's 8-connected labelling, numpy's sum per component,
// np.argmax, util.npmax - as one workgroup per (crop, part).  Host side: openpose_hand_api.hip; the numpy restatements every kernel
// here is held to: bodyfitting_amd/openpose_hand.py.
//
// Every crop has its own size, so each kernel reads a per-crop descriptor (OhBox) and runs over a grid of (the largest crop's
// elements, crops).  Compiled with -ffp-contract=off, as openpose_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "openpose_device.h"
#include "openpose_hand.h"

#define OH_GR 12
#define OH_THRE 0.05

// hand.py:35-38 for every crop of one scale: the crop of its view, cv2.resize(fx=fy=scale, INTER_CUBIC) on uint8 (the fixed-point
// path of bf_op_input_kernel, taps clamped to the crop), padRightDownCorner with 128, / 256 - 0.5.  out[n][Hp][Wp][4], channel 3 zero.
extern "C" __global__ __launch_bounds__(256) void bf_oh_input_kernel(int n, int Hp, int Wp, int H, int W, const OhBox *__restrict__ boxes,
                                                                     const uint8_t *__restrict__ views, float4 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * Hp * Wp) return;
    const int x = (int)(i % Wp), y = (int)((i / Wp) % Hp), b = (int)(i / ((long long)Wp * Hp));
    const OhBox B = boxes[b];
    float v[3] = {0.f, 0.f, 0.f};
    if (y < B.rh && x < B.rw) {
        int xi[4], yi[4], xa[4], ya[4];
        float cx[4], cy[4];
        op_axis(x, B.inv, B.bw, xi, cx);
        op_axis(y, B.inv, B.bh, yi, cy);
        for (int j = 0; j < 4; ++j) { xa[j] = (int)rintf(cx[j] * 2048.f); ya[j] = (int)rintf(cy[j] * 2048.f); }
        const uint8_t *img = views + (size_t)B.view * H * W * 3;
        for (int c = 0; c < 3; ++c) {
            int acc = 0;
            for (int r = 0; r < 4; ++r) {
                const uint8_t *row = img + (size_t)(B.y + yi[r]) * W * 3;
                int h = 0;
                for (int j = 0; j < 4; ++j) h += row[(B.x + xi[j]) * 3 + c] * xa[j];
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

// hand.py:48-49 per crop: the float x8 cubic resize of the network output out[b][hq][wq][22], only its [rh][rw] crop ->
// up[b * up_stride ..][rh][rw][22].  Grid (elements of the largest crop, crops); the sums in bf_op_up8_kernel's order.
extern "C" __global__ __launch_bounds__(256) void bf_oh_up8_kernel(int hq, int wq, long long up_stride, const OhBox *__restrict__ boxes,
                                                                   const float *__restrict__ out, float *__restrict__ up) {
    const int b = blockIdx.y;
    const OhBox B = boxes[b];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B.rh * B.rw * OH_NMAP) return;
    const int c = (int)(i % OH_NMAP);
    const long long q = i / OH_NMAP;
    const int x = (int)(q % B.rw), y = (int)(q / B.rw);
    int rx[4], ry[4];
    float cx[4], cy[4];
    op_axis(x, 0.125, wq, rx, cx);
    op_axis(y, 0.125, hq, ry, cy);
    const float *o = out + (size_t)b * hq * wq * OH_NMAP + c;
    float v = 0.f;
    for (int r = 0; r < 4; ++r) {
        const float *row = o + (size_t)ry[r] * wq * OH_NMAP;
        float hh = row[(size_t)rx[0] * OH_NMAP] * cx[0];
        hh = hh + row[(size_t)rx[1] * OH_NMAP] * cx[1];
        hh = hh + row[(size_t)rx[2] * OH_NMAP] * cx[2];
        hh = hh + row[(size_t)rx[3] * OH_NMAP] * cx[3];
        v = r == 0 ? hh * cy[0] : v + hh * cy[r];
    }
    up[b * up_stride + i] = v;
}

// hand.py:51-54 per crop: the cubic resize of up[rh][rw][22] to the crop's [bh][bw], then heatmap_avg += heatmap / 4 in double (the
// quotient in float, as numpy divides a float32 array).  heat: the crops' [bh][bw][22] laid end to end (OhBox::px).
extern "C" __global__ __launch_bounds__(256) void bf_oh_maps_kernel(long long up_stride, const OhBox *__restrict__ boxes,
                                                                    const float *__restrict__ up, double *__restrict__ heat) {
    const int b = blockIdx.y;
    const OhBox B = boxes[b];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B.bh * B.bw * OH_NMAP) return;
    const int c = (int)(i % OH_NMAP);
    const long long q = i / OH_NMAP;
    const int x = (int)(q % B.bw), y = (int)(q / B.bw);
    int rx[4], ry[4];
    float cx[4], cy[4];
    op_axis(x, B.sx2, B.rw, rx, cx);
    op_axis(y, B.sy2, B.rh, ry, cy);
    const float *o = up + b * up_stride + c;
    float v = 0.f;
    for (int r = 0; r < 4; ++r) {
        const float *row = o + (size_t)ry[r] * B.rw * OH_NMAP;
        float hh = row[(size_t)rx[0] * OH_NMAP] * cx[0];
        hh = hh + row[(size_t)rx[1] * OH_NMAP] * cx[1];
        hh = hh + row[(size_t)rx[2] * OH_NMAP] * cx[2];
        hh = hh + row[(size_t)rx[3] * OH_NMAP] * cx[3];
        v = r == 0 ? hh * cy[0] : v + hh * cy[r];
    }
    const float quarter = v / 4.f;
    double *d = heat + B.px * OH_NMAP + i;
    *d = *d + (double)quarter;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// scipy.ndimage.gaussian_filter(heatmap_avg[:, :, part], sigma=3) for parts 0 .. 20 of every crop: bf_op_gauss_kernel's
// NI_Correlate1D restatement (the weights below are its table), on each crop at its own size (13 or more on a side: one reflection).
// src: the crops' [bh][bw][src_c] end to end, channels 0 .. 20 read; dst: [bh][bw][21] end to end.  Grid (largest crop, crops).
__constant__ double oh_gauss_w[OH_GR + 1] = {
    0x1.105a329f98197p-3, 0x1.01a25f86eb137p-3, 0x1.b42a57d56c0bep-4, 0x1.4a614d1afd337p-4, 0x1.bfde9c12bec92p-5,
    0x1.0fa58939b528fp-5, 0x1.26defcaeb0202p-6, 0x1.1e6bccad344bap-7, 0x1.f1e9915139406p-9, 0x1.8345966f69518p-10,
    0x1.0d8a5ad43c165p-11, 0x1.4fbe39149e277p-13, 0x1.763a210dfb306p-15};

extern "C" __global__ __launch_bounds__(256) void bf_oh_gauss_kernel(int axis, int src_c, const OhBox *__restrict__ boxes,
                                                                     const double *__restrict__ src, double *__restrict__ dst) {
    const int b = blockIdx.y;
    const OhBox B = boxes[b];
    const int H = B.bh, W = B.bw;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)H * W * OH_NPART) return;
    const int c = (int)(i % OH_NPART);
    const long long q = i / OH_NPART;
    const int x = (int)(q % W), y = (int)(q / W);
    const double *img = src + B.px * src_c + c;
    auto at = [&](int yy, int xx) { return img[((size_t)yy * W + xx) * src_c]; };
    double v = at(y, x) * oh_gauss_w[0];
    for (int j = OH_GR; j >= 1; --j) {
        const double s = axis == 0 ? at(op_reflect(y - j, H), x) + at(op_reflect(y + j, H), x)
                                   : at(y, op_reflect(x - j, W)) + at(y, op_reflect(x + j, W));
        v = v + s * oh_gauss_w[j];
    }
    dst[B.px * OH_NPART + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The component pick, hand.py:60-74, one workgroup of 256 threads per (crop, part) on N = bh * bw pixels, with global scratch
// (a crop can be as large as its view):
//   parent[N]  union-find forest, -1 off the mask; a pixel only ever points to a smaller raster index, so each root is its
//              component's first pixel, and skimage's label of a component is 1 + the rank of its root
//   aux[N]     at a root: the running count of its pixels, then its first slot in the gather (or, labelling only, its label)
//   pos[N]     a pixel's place among its component's pixels in raster order
//   cl[N]      the roots in raster order (cl[label - 1])
//   gath[N]    the unblurred map gathered component by component, each in raster order: map_ori[label_img == i]
//   csum[N]    per component np.sum of its gather
// Every phase ends with a device-scope fence and a barrier: the union step links roots with global atomics.
#define OH_T 256

struct OhScratch {
    int *parent, *aux, *pos, *cl;
    double *gath, *csum;
};

__device__ __forceinline__ void oh_phase_end() {
    __threadfence();
    __syncthreads();
}

__device__ __forceinline__ int oh_find(int *parent, int p) {
    int q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (q != p) {
        p = q;
        q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return p;
}

// link the trees of a and b under the smaller root
__device__ void oh_unite(int *parent, int a, int b) {
    while (true) {
        a = oh_find(parent, a);
        b = oh_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + b, a);
        if (old == b) return;                                   // b was still a root: hooked
        b = old;                                                // b was hooked meanwhile: join its new parent to a
    }
}

// parent[] holds p on the mask, -1 off it -> every pixel of the mask points at its root
__device__ void oh_label(int H, int W, int *parent) {
    const int N = H * W, t = threadIdx.x;
    for (int p = t; p < N; p += OH_T) {
        if (parent[p] < 0) continue;
        const int y = p / W, x = p - y * W;
        if (x > 0 && parent[p - 1] >= 0) oh_unite(parent, p, p - 1);
        if (y > 0) {
            const int u = p - W;
            if (x > 0 && parent[u - 1] >= 0) oh_unite(parent, p, u - 1);
            if (parent[u] >= 0) oh_unite(parent, p, u);
            if (x < W - 1 && parent[u + 1] >= 0) oh_unite(parent, p, u + 1);
        }
    }
    oh_phase_end();
    for (int p = t; p < N; p += OH_T)
        if (parent[p] >= 0) __hip_atomic_store(parent + p, oh_find(parent, p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    oh_phase_end();
}

// block-wide exclusive scan of (a, b) over one chunk of 256 -> this thread's prefixes; totals added to *ta / *tb (uniform)
__device__ void oh_scan2(int a, int b, int *pa, int *pb, int *ta, int *tb) {
    __shared__ int wa[OH_T / 64], wb[OH_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sa = a, sb = b;
    for (int d = 1; d < 64; d <<= 1) {
        const int ua = __shfl_up(sa, d), ub = __shfl_up(sb, d);
        if (lane >= d) { sa += ua; sb += ub; }
    }
    if (lane == 63) { wa[wave] = sa; wb[wave] = sb; }
    __syncthreads();
    int oa = *ta, ob = *tb, na = 0, nb = 0;
    for (int w = 0; w < OH_T / 64; ++w) {
        if (w < wave) { oa += wa[w]; ob += wb[w]; }
        na += wa[w]; nb += wb[w];
    }
    *pa = oa + sa - a;
    *pb = ob + sb - b;
    __syncthreads();
    *ta += na;
    *tb += nb;
}

// every pixel's place in its component (raster order within the component) and each root's pixel count in aux[root]
__device__ void oh_positions(int N, const OhScratch &S) {
    __shared__ int s_root[OH_T / 64][64], s_cnt[OH_T / 64][64], s_n[OH_T / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int p = t; p < N; p += OH_T)
        if (S.parent[p] >= 0 && S.parent[p] == p) S.aux[p] = 0;
    __syncthreads();
    for (int base = 0; base < N; base += OH_T) {
        const int p = base + t;
        const int r = p < N ? S.parent[p] : -1;
        if (!__syncthreads_or(r >= 0)) continue;
        int lrank = 0, wcnt = 0, nl = 0;
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lr = __shfl(r, leader);
            const unsigned long long m = __ballot(r == lr);
            if (r == lr) { lrank = __popcll(m & lt); wcnt = __popcll(m); }
            if (lane == 0) { s_root[wave][nl] = lr; s_cnt[wave][nl] = __popcll(m); }
            ++nl;
            todo &= ~m;
        }
        if (lane == 0) s_n[wave] = nl;
        __syncthreads();
        int off = 0, cur = 0;
        bool last = r >= 0 && lrank == wcnt - 1;
        if (r >= 0) {
            for (int w = 0; w < OH_T / 64; ++w) {
                if (w == wave) continue;
                for (int k = 0; k < s_n[w]; ++k)
                    if (s_root[w][k] == r) {
                        if (w < wave) off += s_cnt[w][k];
                        else last = false;
                    }
            }
            cur = S.aux[r];
            S.pos[p] = cur + off + lrank;
        }
        __syncthreads();
        if (last) S.aux[r] = cur + off + lrank + 1;
        __syncthreads();
    }
    oh_phase_end();
}

// the roots in raster order: cl[k] = the root of label k + 1; at each root aux = its first gather slot (ranks: its label).  -> K
__device__ int oh_rank_roots(int N, const OhScratch &S, bool ranks_only) {
    int tk = 0, tn = 0;
    for (int base = 0; base < N; base += OH_T) {
        const int p = base + threadIdx.x;
        const bool root = p < N && S.parent[p] == p;
        const int cnt = root && !ranks_only ? S.aux[p] : 0;
        int k, off;
        oh_scan2(root ? 1 : 0, cnt, &k, &off, &tk, &tn);
        if (root) {
            S.cl[k] = p;
            S.aux[p] = ranks_only ? k + 1 : off;
        }
    }
    oh_phase_end();
    return tk;
}

// np.sum of a contiguous float64 run of n <= 8192: numpy's pairwise summation (leaves of at most 128 with eight partial sums,
// halves rounded down to multiples of 8), iterative: each frame holds a pending right half and the sum of its left half
__device__ double oh_leaf(const double *a, int n) {
    if (n < 8) {
        double r = -0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - n % 8; i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

__device__ double oh_pairwise(const double *a, int n) {
    int rlo[8], rn[8];                                           // rn < 0: the right half is being summed
    double ls[8];
    int top = 0, lo = 0;
    while (true) {
        while (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            rlo[top] = lo + n2; rn[top] = n - n2; ++top;
            n = n2;
        }
        double v = oh_leaf(a + lo, n);
        while (top > 0 && rn[top - 1] < 0) { --top; v = ls[top] + v; }
        if (top == 0) return v;
        ls[top - 1] = v;
        lo = rlo[top - 1]; n = rn[top - 1]; rn[top - 1] = -1;
    }
}

// np.sum of a gathered run of any length: 8192-element buffers summed pairwise, the buffer sums added in order (one thread)
__device__ double oh_sum_serial(const double *a, int n) {
    double s = -0.0;
    for (int b = 0; b < n; b += 8192) s = s + oh_pairwise(a + b, min(8192, n - b));
    return s;
}

template <bool LABEL_ONLY>
__device__ void oh_pick(int H, int W, const double *heat, const OhScratch &S, int *peak, double *score, int *found, int *labels,
                        int *count) {
    const int N = H * W, t = threadIdx.x;
    oh_label(H, W, S.parent);
    if (LABEL_ONLY) {
        const int K = oh_rank_roots(N, S, true);
        for (int p = t; p < N; p += OH_T) labels[p] = S.parent[p] >= 0 ? S.aux[S.parent[p]] : 0;
        if (t == 0) *count = K;
        return;
    }
    oh_positions(N, S);
    const int K = oh_rank_roots(N, S, false);
    for (int p = t; p < N; p += OH_T) {
        const int r = S.parent[p];
        const int slot = r >= 0 ? S.aux[r] + S.pos[p] : -1;
        if (slot >= 0 && slot < N) S.gath[slot] = heat[(size_t)p * OH_NMAP];
    }
    oh_phase_end();
    int total = 0;                                               // the mask's pixel count
    for (int p = t; p < N; p += OH_T) total += S.parent[p] >= 0;
    __shared__ int s_tot;
    __shared__ double s_bs[OH_T];
    if (t == 0) s_tot = 0;
    __syncthreads();
    atomicAdd(&s_tot, total);
    __syncthreads();
    total = s_tot;
    auto comp = [&](int k, int *off, int *n) {
        *off = S.aux[S.cl[k]];
        *n = (k + 1 < K ? S.aux[S.cl[k + 1]] : total) - *off;
    };
    // components of up to 8192 pixels: one thread each; larger ones: one thread per buffer, the buffer sums added in order
    for (int k = t; k < K; k += OH_T) {
        int off, n;
        comp(k, &off, &n);
        if (n <= 8192) S.csum[k] = oh_pairwise(S.gath + off, n);
    }
    for (int k = 0; k < K; ++k) {
        int off, n;
        comp(k, &off, &n);
        if (n <= 8192) continue;
        const int nb = (n + 8191) / 8192;
        double s = 0.0;
        for (int b0 = 0; b0 < nb; b0 += OH_T) {
            const int b = b0 + t;
            if (b < nb) s_bs[t] = oh_pairwise(S.gath + off + (size_t)b * 8192, min(8192, n - b * 8192));
            __syncthreads();
            if (t == 0) {
                for (int j = 0; j < min(OH_T, nb - b0); ++j) s = (b0 + j == 0) ? s_bs[0] : s + s_bs[j];
            }
            __syncthreads();
        }
        if (t == 0) S.csum[k] = s;
    }
    oh_phase_end();
    // np.argmax over the component sums (the first label on a tie), then util.npmax over the map zeroed off that component: the
    // first raster occurrence of the maximum (a zeroed pixel when the component is all negative)
    __shared__ double s_v[OH_T];
    __shared__ int s_i[OH_T];
    double bv = 0.0;
    int bi = -1;
    for (int k = t; k < K; k += OH_T) {
        const double v = S.csum[k];
        if (bi < 0 || v > bv) { bv = v; bi = k; }
    }
    s_v[t] = bv; s_i[t] = bi;
    __syncthreads();
    for (int w = OH_T / 2; w > 0; w >>= 1) {
        if (t < w) {
            const double v = s_v[t + w];
            const int i = s_i[t + w];
            if (i >= 0 && (s_i[t] < 0 || v > s_v[t] || (v == s_v[t] && i < s_i[t]))) { s_v[t] = v; s_i[t] = i; }
        }
        __syncthreads();
    }
    const int R = S.cl[s_i[0]];
    __syncthreads();
    bv = 0.0; bi = -1;
    for (int p = t; p < N; p += OH_T) {
        const double v = S.parent[p] == R ? heat[(size_t)p * OH_NMAP] : 0.0;
        if (bi < 0 || v > bv) { bv = v; bi = p; }
    }
    s_v[t] = bv; s_i[t] = bi;
    __syncthreads();
    for (int w = OH_T / 2; w > 0; w >>= 1) {
        if (t < w) {
            const double v = s_v[t + w];
            const int i = s_i[t + w];
            if (i >= 0 && (s_i[t] < 0 || v > s_v[t] || (v == s_v[t] && i < s_i[t]))) { s_v[t] = v; s_i[t] = i; }
        }
        __syncthreads();
    }
    if (t == 0) {
        const int p = s_i[0];
        peak[0] = p % W; peak[1] = p / W;
        *score = s_v[0];
        *found = 1;
    }
}

// grid (21 parts, crops): bl the blurred maps [bh][bw][21] end to end, heat the maps [bh][bw][22] end to end; px0 the first crop's
// OhBox::px (scratch is laid out from it); peaks[crop][21][2] = (x, y), scores / found [crop][21]
extern "C" __global__ __launch_bounds__(OH_T) void bf_oh_pick_kernel(const OhBox *__restrict__ boxes, long long px0, const double *bl,
                                                                   const double *heat, int *iscr, double *dscr, int *peaks,
                                                                   double *scores, int *found) {
    const int part = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const OhBox B = boxes[b];
    const int N = B.bh * B.bw;
    const size_t base = (size_t)(B.px - px0) * OH_NPART + (size_t)part * N;
    OhScratch S;
    S.parent = iscr + 4 * base; S.aux = S.parent + N; S.pos = S.aux + N; S.cl = S.pos + N;
    S.gath = dscr + 2 * base; S.csum = S.gath + N;
    const double *blp = bl + B.px * OH_NPART + part;
    int any = 0;
    for (int p = t; p < N; p += OH_T) {
        const bool fg = blp[(size_t)p * OH_NPART] > OH_THRE;
        S.parent[p] = fg ? p : -1;
        any |= fg;
    }
    const size_t o = (size_t)b * OH_NPART + part;
    if (!__syncthreads_or(any)) {
        if (t == 0) { peaks[2 * o] = 0; peaks[2 * o + 1] = 0; scores[o] = 0.0; found[o] = 0; }
        return;
    }
    __threadfence();
    __syncthreads();
    oh_pick<false>(B.bh, B.bw, heat + B.px * OH_NMAP + part, S, peaks + 2 * o, scores + o, found + o, nullptr, nullptr);
}

// test hook: skimage.measure.label(binary, connectivity=2) of n images [H][W] -> labels, counts[n]; one workgroup per image
extern "C" __global__ __launch_bounds__(OH_T) void bf_oh_label_kernel(int H, int W, const uint8_t *binary, int *iscr, int *labels,
                                                                    int *counts) {
    const int b = blockIdx.x, N = H * W;
    OhScratch S;
    S.parent = iscr + (size_t)4 * N * b; S.aux = S.parent + N; S.pos = S.aux + N; S.cl = S.pos + N;
    S.gath = nullptr; S.csum = nullptr;
    for (int p = threadIdx.x; p < N; p += OH_T) S.parent[p] = binary[(size_t)b * N + p] ? p : -1;
    __threadfence();
    __syncthreads();
    oh_pick<true>(H, W, nullptr, S, nullptr, nullptr, nullptr, labels + (size_t)b * N, counts + b);
}
