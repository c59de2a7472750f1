// The stand-alone silhouette loss for gfx950 (bf_silhouette_loss): reference smplify/loss.py:85-130 `multview_mask_loss` on vertices
// the CALLER holds, with its gradient.  One frame, M views that are their own cameras (MaskIO: F = 1, view_index = identity,
// weight = 1), three launches:
//
//   bf_sil_project_kernel   thread = sampled vertex x view: bf_mask_project_one on verts[s * stride] - uv, inside flag, binary term
//                           and its d/duv; zeroes the vertex's fixed-point sums
//   bf_sil_contour_kernel   bf_mask_contour_body in its fixed-point-sum mode (MaskIO::acc: 64-bit integer atomics, exact and so
//                           order-free): nearest inside vertex of every contour point, the contour term's block sums; the
//                           distance form per view as torch.cdist chooses it
//   bf_sil_finish_kernel    thread = vertex: the views in view order - fixed-point sums back to float, + the binary term's d/duv,
//                           back through the view's projection (bf_mask_gather_kernel's closing step) - into dverts[n_verts,3] in
//                           full, zeros at unsampled vertices included; its last block reduces the block sums to view_terms[M,2]
//                           and the loss, in an order that depends on the view's own sizes alone
// The per-vertex and per-contour-point arithmetic is loss_bodies.h's, shared with the fused fit: the two paths cannot drift apart.
//
// Two more for the device route (bf_silhouette_create_dev, bf_silhouette_loss_dev), where masks and cameras are device arrays:
//   bf_sil_ingest_kernel    masks in the caller's type -> the object's 0 / 1 bytes, a "has foreground" flag per view and one "holds
//                           a value other than 0 / 1" flag
//   bf_sil_rows_kernel      thread = row element: the 3 x 4 rows K [R|t] of every view, the host loop's expression in double
#include "bf_internal.h"
#include "loss_bodies.h"
#include "silhouette_kernels.h"

#define BF_CDIST_DIRECT_ROWS 25       // torch.cdist (use_mm_for_euclid_dist_if_necessary): the matmul form only beyond 25 rows

// grid (ceil(Ns/256), M).  verts[n_verts][3] as the caller holds them, read with the call's stride; proj[M][12] = K [R|t] rows
extern "C" __global__ void __launch_bounds__(256)
bf_sil_project_kernel(MaskIO K, const float *__restrict__ verts, const float *__restrict__ proj, float *__restrict__ uvi,
                      float *__restrict__ duvb, float *__restrict__ loss_part) {
    __shared__ float sred[4];
    const int s = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    float lval = 0.f;
    if (s < K.ns) {
        const float *X = verts + (size_t)s * K.sstride * 3;
        lval = bf_mask_project_one(K, X[0], X[1], X[2], proj, 0, m, s, uvi, duvb);
    }
    const float tot = bf_block_sum_256(bf_wave_sum(lval), sred);
    if (threadIdx.x == 0) loss_part[(size_t)m * K.part_stride + blockIdx.x] = tot;
}

// grid (ceil(16 Cmax/256), M): sixteen lanes per contour point (loss_bodies.h); K.acc is set, so nothing but the sums and the
// block's share of the contour term is written.  The cdist form is torch.cdist's as torch chooses it (loss.py:110 leaves the
// compute mode at its default): the expanded form for a view with MORE THAN 25 inside vertices, direct (a - b)^2 sums up to
// there (the other operand, one contour point, has one row).  The fused fit never meets the second case; a caller's handful of
// vertices does.  The view's inside vertices are counted by the whole block, a tile at a time, until they exceed 25.
extern "C" __global__ void __launch_bounds__(256)
bf_sil_contour_kernel(MaskIO K, const float *__restrict__ uvi, float *__restrict__ loss_part) {
    __shared__ float4 tile[256];
    __shared__ float sred[4];
    if (K.cdist) {
        const float4 *rec = (const float4 *)uvi + (size_t)blockIdx.y * K.ns;
        int inside = 0;                                        // (the same on every thread)
        for (int base = 0; base < K.ns && inside <= BF_CDIST_DIRECT_ROWS; base += 256) {
            const int s = base + (int)threadIdx.x;
            inside += __syncthreads_count(s < K.ns && rec[s].z > 0.5f);
        }
        if (inside <= BF_CDIST_DIRECT_ROWS) K.cdist = 0;
    }
    bf_mask_contour_body<256>(blockIdx.x, blockIdx.y, 0, tile, sred, K, uvi, (int *)nullptr, (float *)nullptr, loss_part);
}

// grid (vertex blocks + 1), 256 threads; vertex blocks = ceil(n_verts/256), or 0 when dverts is null.  The LAST block reduces:
// wave w takes views w, w + 4, ...: a view's terms = its block sums, lane l adding every 64th in ascending order, the lanes merged
// by the xor butterfly (the same sum on every lane) - nothing in it depends on another view.  terms[0] = loss = terms[1 .. 1 + 2M)
// added in memory order; terms[1 + 2m] = view m's contour term, terms[2 + 2m] = its binary term.
extern "C" __global__ void __launch_bounds__(256)
bf_sil_finish_kernel(MaskIO K, const float *__restrict__ proj, const float *__restrict__ uvi, const float *__restrict__ duvb,
                     const float *__restrict__ loss_part, float *__restrict__ terms, float *__restrict__ dverts) {
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        if (!terms) return;
        const int lane = tid & 63, wave = tid >> 6;
        for (int m = wave; m < K.n_masks; m += 4) {
            const float *p = loss_part + (size_t)m * K.part_stride;
            const int nc = (K.contour_count[m] * 16 + 255) / 256;          // (16 lanes per contour point)
            float b = 0.f, c = 0.f;
            for (int i = lane; i < K.proj_blocks; i += 64) b += p[i];
            for (int i = lane; i < nc; i += 64) c += p[K.proj_blocks + i];
            b = bf_wave_sum(b); c = bf_wave_sum(c);
            if (lane == 0) { terms[1 + 2 * (size_t)m] = c; terms[2 + 2 * (size_t)m] = b; }
        }
        __threadfence_block();
        __syncthreads();
        if (tid == 0) {
            float tot = 0.f;
            for (size_t i = 0; i < 2 * (size_t)K.n_masks; ++i) tot += terms[1 + i];
            terms[0] = tot;
        }
        return;
    }
    const int v = blockIdx.x * 256 + tid;
    if (v >= K.nv) return;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    const int s = v / K.sstride;
    if (s * K.sstride == v) {
        for (int m = 0; m < K.n_masks; ++m) {
            const size_t o = (size_t)m * K.ns + s;
            const float tu = duvb[o * 2] + bf_acc_float(K.acc[o * 2]), tv = duvb[o * 2 + 1] + bf_acc_float(K.acc[o * 2 + 1]);
            const float4 r = ((const float4 *)uvi)[o];
            const float *P = proj + (size_t)m * 12;
            const float q0 = tu * r.w, q1 = tv * r.w, q2 = -(tu * r.x + tv * r.y) * r.w;
            // (the view's share first, then onto the sum: the share's bits do not depend on the views before it)
            const float h0 = P[0] * q0 + P[4] * q1 + P[8] * q2;
            const float h1 = P[1] * q0 + P[5] * q1 + P[9] * q2;
            const float h2 = P[2] * q0 + P[6] * q1 + P[10] * q2;
            g0 += h0; g1 += h1; g2 += h2;
        }
    }
    float *o = dverts + (size_t)v * 3;
    o[0] = g0; o[1] = g1; o[2] = g2;
}

// grid ceil(ceil(npix / 4) / 256), 256 threads; thread = four consecutive pixels of masks[M][H][W] (float32, or one byte per pixel:
// uint8 / bool), read element by element - the array is aligned to its element and no further - and stored as ONE word of the
// object's bytes bin[ceil(npix / 4) * 4] (1 = foreground; the bytes behind npix are written as 0).  flags[M + 1], zeroed by the
// caller: flags[m] |= 1 when view m has a foreground pixel, flags[M] |= 1 when a pixel is neither 0 nor 1 (a NaN is neither).  A
// block whose pixels lie in one view raises that view's flag once, through LDS; a block across views (small images) per thread.
extern "C" __global__ void __launch_bounds__(256)
bf_sil_ingest_kernel(const void *__restrict__ masks, int is_float, unsigned long long npix, unsigned plane, unsigned *__restrict__ bin,
                     int *__restrict__ flags, int n_views) {
    __shared__ int any_fg, any_bad;
    if (threadIdx.x == 0) { any_fg = 0; any_bad = 0; }
    __syncthreads();
    const unsigned long long block_first = (unsigned long long)blockIdx.x * 1024u;
    const unsigned long long block_last = min(block_first + 1023u, npix - 1);
    const bool one_view = block_first / plane == block_last / plane;
    const unsigned long long first = block_first + (unsigned long long)threadIdx.x * 4u;
    if (first < npix) {
        unsigned word = 0;
        bool bad = false;
        for (unsigned j = 0; j < 4; ++j) {
            const unsigned long long i = first + j;
            if (i >= npix) break;
            bool fg;
            if (is_float) {
                const float x = ((const float *)masks)[i];
                fg = x == 1.f;
                bad |= !(fg || x == 0.f);
            } else {
                const unsigned char x = ((const unsigned char *)masks)[i];
                fg = x == 1;
                bad |= x > 1;
            }
            if (fg) {
                word |= 1u << (8 * j);
                if (one_view) any_fg = 1;          // (a race on purpose, here and for any_bad: every writer stores 1, the read is behind the barrier)
                else atomicOr(&flags[i / plane], 1);
            }
        }
        bin[first / 4] = word;
        if (bad) any_bad = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (any_fg) atomicOr(&flags[block_first / plane], 1);
        if (any_bad) atomicOr(&flags[n_views], 1);
    }
}

// grid ceil(12 M / 256), 256 threads; thread = one element of rows[M][3][4] = K [R|t] from K[M][3][3] and w2c[M][4][4] (rows 0..2).
extern "C" __global__ void __launch_bounds__(256)
bf_sil_rows_kernel(const float *__restrict__ K, const float *__restrict__ w2c, int n_views, float *__restrict__ rows) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_views * 12) return;
    const int i = e / 12, r = (e % 12) / 4, c = e % 4;
    const float *k = K + (size_t)i * 9 + r * 3, *w = w2c + (size_t)i * 16 + c;
    // bf_silhouette_loss' host expression, summed left to right.  A product of two float32 values is exact in double (24 + 24 bits
    // of significand in 53), so a * b + c rounds once whether the compiler fuses it or not: these are the host loop's bits.
    rows[e] = (float)((double)k[0] * w[0] + (double)k[1] * w[4] + (double)k[2] * w[8]);
}
