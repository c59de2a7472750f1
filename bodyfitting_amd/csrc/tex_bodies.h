// The per-vertex / per-face / per-pixel arithmetic of the rasteriser, shared by tex_kernels.hip (the fused texture-fitting loop) and
// nr_kernels.hip (the stand-alone neural_renderer.Renderer): one body each, so the two paths cannot drift apart.
// (The VALUES follow neural_renderer's float32 operation order - projection.py:6-42, rasterize_cuda_kernel.cu:38-63,110-137,209-240 -
// because a render has to agree with it pixel for pixel: an edge test that rounds the other way hands a pixel to the neighbouring face.
// Both files are compiled without fused multiply-adds for the same reason.)
#pragma once
#include "bf_internal.h"
#include "tex_kernels.h"

#define BF_TEX_TILE 8
#define BF_TEX_REC 20            // floats per face record
#define BF_TEX_GATHER_MAX 4096   // faces whose pixel box is larger go through the per-pixel atomic path of the backward pass

// neural_renderer/projection.py:6-42, zero distortion: world (a, b, c) -> (u, v in [-1,1], z)
__device__ __forceinline__ void tex_project(const TexView &V, float a, float b, float c, float out[3]) {
    if (V.orig < 0.f) { out[0] = a; out[1] = b; out[2] = c; return; }      // already normalised device coordinates (UV-space render)
    // vertices @ R^T + t : (a R00 + b R01) + c R02, then + t  (row-vector times matrix, k ascending)
    const float x = ((a * V.R[0] + b * V.R[1]) + c * V.R[2]) + V.t[0];
    const float y = ((a * V.R[3] + b * V.R[4]) + c * V.R[5]) + V.t[1];
    const float z = ((a * V.R[6] + b * V.R[7]) + c * V.R[8]) + V.t[2];
    const float x_ = x / (z + 1e-9f), y_ = y / (z + 1e-9f);
    float u = (x_ * V.K[0] + y_ * V.K[1]) + V.K[2];
    float w = (x_ * V.K[3] + y_ * V.K[4]) + V.K[5];
    w = V.orig - w;
    u = 2.f * (u - V.orig / 2.f) / V.orig;
    w = 2.f * (w - V.orig / 2.f) / V.orig;
    out[0] = u; out[1] = w; out[2] = z;
}

struct TexTri { float x[3], y[3], z[3]; };       // a face's corners: normalised device coordinates + depth

__device__ __forceinline__ TexTri tex_tri(const float *f9) {
    TexTri t;
#pragma unroll
    for (int c = 0; c < 3; ++c) { t.x[c] = f9[3 * c]; t.y[c] = f9[3 * c + 1]; t.z[c] = f9[3 * c + 2]; }
    return t;
}

// the face shows its back when its signed area is negative: (c2 - c0) x (c1 - c0) compared as two products
__device__ __forceinline__ bool tex_back_facing(const TexTri &t) {
    return (t.y[2] - t.y[0]) * (t.x[1] - t.x[0]) < (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
}

// A pixel centre (xp, yp) lies outside the face when it is on the wrong side of one of the three directed edges a -> b.
__device__ __forceinline__ bool tex_outside(const TexTri &t, float xp, float yp) {
    bool out = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3;
        out = out || (yp - t.y[a]) * (t.x[b] - t.x[a]) < (xp - t.x[a]) * (t.y[b] - t.y[a]);
    }
    return out;
}

// Rows of the inverse of [[x0 x1 x2], [y0 y1 y2], [1 1 1]] over pixel-space corners: row k gives corner k's barycentric weight as
// a x + b y + c.  Row k is the cofactor row of the two OTHER corners taken cyclically, a = k + 1, b = k + 2.
__device__ __forceinline__ void tex_barycentric_rows(const float px[3], const float py[3], float rows[9]) {
    float cof[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        cof[3 * k] = py[a] - py[b];
        cof[3 * k + 1] = px[b] - px[a];
        cof[3 * k + 2] = px[a] * py[b] - px[b] * py[a];
    }
    const float det = px[2] * cof[6] + px[0] * cof[0] + px[1] * cof[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) rows[k] = cof[k] / det;
}

// weights of pixel (xi, yi) clamped to [0, 1] and renormalised; returns the interpolated depth 1 / sum(w_k / z_k)
__device__ __forceinline__ float tex_weights(const float rows[9], const TexTri &t, int xi, int yi, float w[3]) {
    float total = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w[k] = fminf(fmaxf(rows[3 * k] * xi + rows[3 * k + 1] * yi + rows[3 * k + 2], 0.f), 1.f);
        total += w[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] /= total;
    return 1.f / (w[0] / t.z[0] + w[1] / t.z[1] + w[2] / t.z[2]);
}

// face record (BF_TEX_REC floats): nine projected coordinates (x0 y0 z0 x1 y1 z1 x2 y2 z2) | nine entries of the inverted
// triangle | the pixel box that holds every pixel the face can own: x0 | x1 << 16, y0 | y1 << 16 (empty: x1 < x0)
// Record i from its nine projected coordinates f.  pass 0: the record + count the tiles of the box; pass 1: write the record into
// their lists (cursor = running start).
__device__ __forceinline__ void tex_face_record(int i, const float f[9], int is, int tiles, float *__restrict__ frec, int *__restrict__ tile_count,
                                                int *__restrict__ cursor, int *__restrict__ tile_list, int pass, int cap) {
    float *rec = frec + (size_t)i * BF_TEX_REC;
    if (pass == 0) { rec[18] = __int_as_float(1); rec[19] = __int_as_float(1); }          // (empty box until shown otherwise)
    const TexTri tri = tex_tri(f);
    if (tex_back_facing(tri)) return;                                                      // never drawn
    float px[3], py[3];                                                                    // corners in pixel units of the super-sampled image
#pragma unroll
    for (int n = 0; n < 3; ++n) { px[n] = 0.5f * (tri.x[n] * is + is - 1); py[n] = 0.5f * (tri.y[n] * is + is - 1); }
    // pixels whose centre can pass the three edge tests lie inside the triangle's pixel-space bounding box (one pixel of slack)
    const float xmin = fminf(px[0], fminf(px[1], px[2])), xmax = fmaxf(px[0], fmaxf(px[1], px[2]));
    const float ymin = fminf(py[0], fminf(py[1], py[2])), ymax = fmaxf(py[0], fmaxf(py[1], py[2]));
    if (!(xmax >= -1.f && ymax >= -1.f && xmin <= (float)is && ymin <= (float)is)) return;       // (also drops NaN boxes)
    const int x0 = max((int)floorf(fmaxf(xmin, 0.f)) - 1, 0), x1 = min((int)ceilf(fminf(xmax, (float)is)) + 1, is - 1);
    const int y0 = max((int)floorf(fmaxf(ymin, 0.f)) - 1, 0), y1 = min((int)ceilf(fminf(ymax, (float)is)) + 1, is - 1);
    if (pass == 0) {
        float rows[9];
        tex_barycentric_rows(px, py, rows);
#pragma unroll
        for (int k = 0; k < 9; ++k) { rec[k] = f[k]; rec[9 + k] = rows[k]; }
        rec[18] = __int_as_float(x0 | (x1 << 16)); rec[19] = __int_as_float(y0 | (y1 << 16));
    }
    for (int ty = y0 / BF_TEX_TILE; ty <= y1 / BF_TEX_TILE; ++ty)
        for (int tx = x0 / BF_TEX_TILE; tx <= x1 / BF_TEX_TILE; ++tx) {
            const int tile = ty * tiles + tx;
            if (pass == 0) atomicAdd(tile_count + tile + 1, 1);
            else { const int slot = atomicAdd(cursor + tile, 1); if (slot < cap) tile_list[slot] = i; }      // (cap: the host re-runs the pass with a larger list when the total said so)
        }
}

// The z-buffer of one pixel: lane = pixel (xi, yi) of a tile, the wave walks the tile's list entries [s0, s1) staged through
// `stage` (the wave's own [64][19] floats of LDS) 64 at a time and keeps the lexicographic (depth, record index) minimum - the
// reference's strict `<` in face order - so the result does not depend on the order of the list.
struct TexHit { float depth, w[3]; int face; };       // face = -1: nothing drawn, depth = far

__device__ __forceinline__ TexHit tex_tile_nearest(float (*stage)[19], int lane, const float *__restrict__ frec, const int *__restrict__ tile_list,
                                                   int s0, int s1, int is, int xi, int yi, float near, float far) {
    const float yp = (2.f * yi + 1 - is) / is, xp = (2.f * xi + 1 - is) / is;
    TexHit h;
    h.depth = far; h.w[0] = h.w[1] = h.w[2] = 0.f; h.face = -1;
    for (int base = s0; base < s1; base += 64) {
        const int n = min(64, s1 - base);
        __builtin_amdgcn_wave_barrier();
        if (lane < n) {
            const int fn = tile_list[base + lane];
            const float *src = frec + (size_t)fn * BF_TEX_REC;
#pragma unroll
            for (int k = 0; k < 18; ++k) stage[lane][k] = src[k];
            stage[lane][18] = __int_as_float(fn);
        }
        __builtin_amdgcn_wave_barrier();
        for (int j = 0; j < n; ++j) {
            const float *face = stage[j];
            const int fn = __float_as_int(face[18]);
            const TexTri tri = tex_tri(face);
            if (tex_outside(tri, xp, yp)) continue;
            float w[3];
            const float zp = tex_weights(face + 9, tri, xi, yi, w);
            if (zp <= near || far <= zp) continue;
            if (zp < h.depth || (zp == h.depth && h.face >= 0 && fn < h.face)) {      // first strictly nearer face in face order
                h.depth = zp; h.face = fn; h.w[0] = w[0]; h.w[1] = w[1]; h.w[2] = w[2];
            }
        }
    }
    return h;
}

// Texture sampling of one pixel: position inside the face's ts^3 texture cube = barycentric weight x (ts - 1), perspective-corrected by
// depth / corner depth and kept inside the cube; the colour is the trilinear blend of the 8 texels around it.  idx / wt: their
// indices and weights, corner bit k set = the upper texel along axis k.
__device__ __forceinline__ void tex_corners(const float w[3], float depth, const float *__restrict__ frec, int ts, int idx[8], float wt[8]) {
    int cell[3];
    float hi[3], lo[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float pos = fminf(fmaxf(w[k] * (ts - 1) * (depth / frec[3 * k + 2]), 0.f), ts - 1 - 1e-4f);
        cell[k] = (int)pos;
        hi[k] = pos - cell[k];
        lo[k] = 1.f - hi[k];
    }
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int u0 = corner & 1, u1 = (corner >> 1) & 1, u2 = corner >> 2;
        idx[corner] = (cell[0] + u0) * ts * ts + (cell[1] + u1) * ts + (cell[2] + u2);
        wt[corner] = (u0 ? hi[0] : lo[0]) * (u1 ? hi[1] : lo[1]) * (u2 ? hi[2] : lo[2]);
    }
}

// dL/drgb of one super-sampled pixel, through the pooling and the flip
__device__ __forceinline__ void tex_pixel_grad(int yi, int xi, int is, int out, int aa, const float *__restrict__ grad_image, float g[3]) {
    const int yf = is - 1 - yi, oy = aa ? yf >> 1 : yf, ox = aa ? xi >> 1 : xi;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = grad_image[((size_t)c * out + oy) * out + ox] * (aa ? 0.25f : 1.f);
}

// the same for a one-channel map (depth, alpha)
__device__ __forceinline__ float tex_pixel_grad1(int yi, int xi, int is, int out, int aa, const float *__restrict__ grad_map) {
    const int yf = is - 1 - yi, oy = aa ? yf >> 1 : yf, ox = aa ? xi >> 1 : xi;
    return grad_map[(size_t)oy * out + ox] * (aa ? 0.25f : 1.f);
}

// backward_pixel_map's signed distance of pixel d1 from an edge's end point, in normalised device units (rasterize_cuda_kernel.cu:404-405):
// `num / den * off * 2. / is` - float32 up to the literal 2., double from there, rounded back - pushed away from 0 by rasterizer_eps = 1e-3
__device__ __forceinline__ float tex_edge_dist(float num, float den, float off, int is) {
    const float d = (float)((double)(num / den * off) * 2. / (double)is);
    return 0.f < d ? d + 1e-3f : d - 1e-3f;
}

// the crossing of line d0 with the edge (a0, a1) -> (b0, b1), first coordinate along the line index (rasterize_cuda_kernel.cu:317,421,424)
__device__ __forceinline__ float tex_edge_cross(float a0, float a1, float b0, float b1, float d0) {
    return (b1 - a1) / (b0 - a0) * (d0 - a0) + a1;
}

// float -> int as the reference's target converts it: NaN -> 0, saturating (here: to [lo, hi], which the callers clamp to anyway)
__device__ __forceinline__ int tex_to_int(float v, int lo, int hi) {
    return v != v ? 0 : (int)fminf(fmaxf(v, (float)lo), (float)hi);
}
