// GeneBody view preparation (reference apps/genebody_fitting.py:119-131, utils/io_utils.py:97-101): the mask bounding box and the
// fused crop, mask, resize and sum of every view of a frame.  Host side: views_api.hip; numpy restatement: bodyfitting_amd/genebody.py.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include "views_kernels.h"
#include "wave_ops.h"
#include "resize_axis.h"

#define VW_THREADS 256

// per view (top, left, bottom, right) = (INT_MAX, INT_MAX, -1, -1): what the atomics of bf_views_bbox_kernel reduce into
extern "C" __global__ __launch_bounds__(VW_THREADS) void bf_views_bbox_init_kernel(int n, int *__restrict__ bbox) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * 4) bbox[i] = (i & 3) < 2 ? INT_MAX : -1;
}

// np.where(mask != 0) -> min / max row and column, per view.  masks: n views of H * W bytes, view v at v * stride (stride a multiple of
// 16, the bytes past H * W are not read as pixels).  Grid (blocks per view, n); each thread streams 16-byte chunks, skips all-zero
// ones, and walks the bytes of the others with an incremental (row, column); one wave reduction, one LDS step across the four waves,
// then one atomicMin / atomicMax per value per workgroup.
extern "C" __global__ __launch_bounds__(VW_THREADS) void bf_views_bbox_kernel(int H, int W, long long stride,
                                                                               const uint8_t *__restrict__ masks, int *__restrict__ bbox) {
    const int v = blockIdx.y;
    const long long hw = (long long)H * W, chunks = stride >> 4;
    const uint4 *src = reinterpret_cast<const uint4 *>(masks + (long long)v * stride);
    int top = INT_MAX, left = INT_MAX, bottom = -1, right = -1;
    for (long long c = (long long)blockIdx.x * VW_THREADS + threadIdx.x; c < chunks; c += (long long)gridDim.x * VW_THREADS) {
        const uint4 q = src[c];
        if ((q.x | q.y | q.z | q.w) == 0) continue;
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
        const long long p0 = c << 4;
        int r = (int)(p0 / W), x = (int)(p0 - (long long)r * W);
        for (int k = 0; k < 16; ++k) {
            if (p0 + k >= hw) break;
            if ((w4[k >> 2] >> ((k & 3) * 8)) & 0xff) {
                top = min(top, r); bottom = max(bottom, r);
                left = min(left, x); right = max(right, x);
            }
            if (++x == W) { x = 0; ++r; }
        }
    }
    __shared__ int red[4][VW_THREADS / 64];
    top = bf_wave_min(top); left = bf_wave_min(left); bottom = bf_wave_max(bottom); right = bf_wave_max(right);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = top; red[1][wave] = left; red[2][wave] = bottom; red[3][wave] = right; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VW_THREADS / 64; ++w) {
            top = min(top, red[0][w]); left = min(left, red[1][w]); bottom = max(bottom, red[2][w]); right = max(right, red[3][w]);
        }
        if (bottom >= 0) {
            atomicMin(bbox + v * 4 + 0, top);
            atomicMin(bbox + v * 4 + 1, left);
            atomicMax(bbox + v * 4 + 2, bottom);
            atomicMax(bbox + v * 4 + 3, right);
        }
    }
}

// VResizeLinear<uchar>: (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
__device__ __forceinline__ uint8_t vw_vert(int b0, int b1, int h0, int h1) {
    return (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// img = (img * (msk > 128)[..., None])[top:bottom, left:right] resized to L x L, the mask crop resized to L x L for mask views, and
// the integer sum of the resized RGB bytes (np.mean(img) > 10 <=> sum > 30 L^2).  Grid (ceil(L * L / 256), n): one thread per output
// pixel, all three channels; one atomicAdd per workgroup into sums[v] (zeroed by the caller on the stream).
extern "C" __global__ __launch_bounds__(VW_THREADS) void bf_views_prepare_kernel(int L, int W, const VwJob *__restrict__ jobs,
                                                                                  const uint8_t *__restrict__ crops,
                                                                                  const uint8_t *__restrict__ masks,
                                                                                  uint8_t *__restrict__ out_images,
                                                                                  uint8_t *__restrict__ out_masks,
                                                                                  unsigned long long *__restrict__ sums) {
    const int v = blockIdx.y;
    const VwJob j = jobs[v];
    const int i = blockIdx.x * VW_THREADS + threadIdx.x;
    unsigned int s = 0;
    if (i < L * L) {
        const int dy = i / L, dx = i % L;
        int x0, x1, a0, a1, y0, y1, b0, b1;
        // any crop size -> L: OpenCV's scale 1 / (L / n_src) in double
        bf_resize_axis(dx, 1.0 / ((double)L / (double)j.cw), j.cw, 1, &x0, &x1, &a0, &a1);
        bf_resize_axis(dy, 1.0 / ((double)L / (double)j.ch), j.ch, 0, &y0, &y1, &b0, &b1);
        const bool edge = x0 == j.cw - 1;     // OpenCV's tail loop: S[sx] * 2048 without the second tap
        const uint8_t *m0 = masks + j.msk_off + (long long)y0 * W, *m1 = masks + j.msk_off + (long long)y1 * W;
        const uint8_t *r0 = crops + j.img_off + (long long)y0 * W * 3, *r1 = crops + j.img_off + (long long)y1 * W * 3;
        const bool k00 = m0[x0] > 128, k01 = m0[x1] > 128, k10 = m1[x0] > 128, k11 = m1[x1] > 128;
        uint8_t *o = out_images + ((long long)v * L * L + i) * 3;
        for (int c = 0; c < 3; ++c) {
            const int p00 = k00 ? r0[x0 * 3 + c] : 0, p01 = k01 ? r0[x1 * 3 + c] : 0;
            const int p10 = k10 ? r1[x0 * 3 + c] : 0, p11 = k11 ? r1[x1 * 3 + c] : 0;
            const int h0 = edge ? p00 * 2048 : p00 * a0 + p01 * a1;
            const int h1 = edge ? p10 * 2048 : p10 * a0 + p11 * a1;
            const uint8_t u = vw_vert(b0, b1, h0, h1);
            o[c] = u;
            s += u;
        }
        if (j.mask_slot >= 0) {
            const int h0 = edge ? m0[x0] * 2048 : m0[x0] * a0 + m0[x1] * a1;
            const int h1 = edge ? m1[x0] * 2048 : m1[x0] * a0 + m1[x1] * a1;
            out_masks[(long long)j.mask_slot * L * L + i] = vw_vert(b0, b1, h0, h1);
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ unsigned int red[VW_THREADS / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < VW_THREADS / 64; ++w) t += red[w];
        atomicAdd(sums + v, t);
    }
}
