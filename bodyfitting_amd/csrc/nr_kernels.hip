// neural_renderer.Renderer as a stand-alone object (thirdparty/neural_renderer/neural_renderer/renderer.py:11-346), for gfx950: what
// the fused texture-fitting kernels of tex_kernels.hip leave out - directional light, fill-back, the alpha output, a texture VJP of an
// arbitrary rgb cotangent per render.  Compiled with -ffp-contract=off like tex_kernels.hip; the rasteriser's arithmetic is the ONE
// copy in tex_bodies.h, and the projection, compose and depth kernels are tex_kernels.hip's own (tex_kernels.h).
//
// Records.  A render draws nrec face records: nrec = NF, or 2 NF with fill_back (renderer.py:176-178).  Record k is face f = k mod NF;
// for k >= NF its corners are reversed and texel (a, b, c) of the record is texel (c, b, a) of cube f - `textures.permute((0, 1, 4,
// 3, 2, 5))` without the doubled copy.  The z-buffer keeps the lexicographic (depth, record index) minimum, i.e. the reference's
// strict `<` over the concatenated list.
//
//   bf_nr_face_kernel            bf_tex_face_kernel per record + the record's light row (lighting.py:5-57) from the world-space corners
//   bf_nr_raster_kernel          bf_tex_raster_kernel with texel x light before the sampling weight, and the back records' axis exchange
//   bf_nr_alpha_kernel           forward_alpha_map + flip + 2 x 2 pooling (rasterize.py:181-184,312-325)
//   bf_nr_backward_kernel        backward_textures for any dL/drgb, gathered: one wave owns BOTH records of a face, adds the pixels they
//                                own into the face's cube in LDS and stores it - every texel of every cube written once, no clearing pass
//   bf_nr_backward_large_kernel  records whose pixel box exceeds BF_TEX_GATHER_MAX: per pixel, global atomicAdd (runs after the gather)
#include "bf_internal.h"
#include "nr_kernels.h"
#include "tex_bodies.h"

// lighting.py:33-52 for one face from its world-space corners c0, c1, c2 (3 floats each), float32, in this order:
//   light = 0; ambient != 0: light += ambient * color_ambient; directional != 0: v10 = c0 - c1, v12 = c2 - c1, n = v10 x v12,
//   n /= max(|n|, 1e-5) (F.normalize), cos = max((n0 d0 + n1 d1) + n2 d2, 0), light += directional * (color_directional * cos)
__device__ __forceinline__ void nr_face_light(const NrLight &L, const float *c0, const float *c1, const float *c2, float light[3]) {
    light[0] = light[1] = light[2] = 0.f;
    if (L.ambient != 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) light[c] += L.ambient * L.color_ambient[c];
    }
    if (L.directional != 0.f) {
        float a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] = c0[c] - c1[c]; b[c] = c2[c] - c1[c]; }
        float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const float len = fmaxf(sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), 1e-5f);
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = n[c] / len;
        const float cosv = fmaxf((n[0] * L.direction[0] + n[1] * L.direction[1]) + n[2] * L.direction[2], 0.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) light[c] += L.directional * (L.color_directional[c] * cosv);
    }
}

// texel index inside cube f of a record's texel index: back records read (c, b, a) for (a, b, c)
__device__ __forceinline__ int nr_texel(int idx, int ts, bool back) {
    if (!back) return idx;
    const int a = idx / (ts * ts), r = idx - a * ts * ts, b = r / ts, c = r - b * ts;
    return (c * ts + b) * ts + a;
}

// thread = record k in [0, nrec).  verts: world space (what the light sees), pv: projected.  light[nrec][3] (written in pass 0, also
// for records that are never drawn), or NULL with L.on = 0.
extern "C" __global__ void __launch_bounds__(256)
bf_nr_face_kernel(int nf, int nrec, const int *__restrict__ faces, const float *__restrict__ pv, const float *__restrict__ verts, NrLight L, int is,
                  int tiles, float *__restrict__ frec, float *__restrict__ light, int *__restrict__ tile_count, int *__restrict__ cursor,
                  int *__restrict__ tile_list, int pass, int cap) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nrec) return;
    const bool back = k >= nf;
    const int fn = back ? k - nf : k;
    int vid[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) vid[c] = faces[(size_t)fn * 3 + (back ? 2 - c : c)];
    float f[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *v = pv + (size_t)vid[c] * 3;
        f[c * 3] = v[0]; f[c * 3 + 1] = v[1]; f[c * 3 + 2] = v[2];
    }
    if (pass == 0 && L.on) {
        float l[3];
        nr_face_light(L, verts + (size_t)vid[0] * 3, verts + (size_t)vid[1] * 3, verts + (size_t)vid[2] * 3, l);
        light[(size_t)k * 3] = l[0]; light[(size_t)k * 3 + 1] = l[1]; light[(size_t)k * 3 + 2] = l[2];
    }
    tex_face_record(k, f, is, tiles, frec, tile_count, cursor, tile_list, pass, cap);
}

// grid (tiles * tiles / 4), 256 threads: wave = tile, lane = pixel (8 x 8).  pix[is][is] = (w0, w1, w2, depth, record) per pixel;
// rgb[is][is][3] with the background filled in, skipped when textures is NULL (silhouette / depth renders).  light NULL: lightoff.
extern "C" __global__ void __launch_bounds__(256)
bf_nr_raster_kernel(int is, int tiles, int nf, const float *__restrict__ frec, const float *__restrict__ light, const int *__restrict__ tile_start,
                    const int *__restrict__ tile_list, const float *__restrict__ textures, int ts, float near, float far, float bg0, float bg1,
                    float bg2, float *__restrict__ pix, float *__restrict__ rgb, int cap) {
    __shared__ float s_f[4][64][19];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, tile = blockIdx.x * 4 + wv;
    if (tile >= tiles * tiles) return;                     // (wave-uniform)
    const int ty = tile / tiles, tx = tile - ty * tiles;
    const int yi = ty * BF_TEX_TILE + (lane >> 3), xi = tx * BF_TEX_TILE + (lane & 7);
    const int s0 = min(tile_start[tile], cap), s1 = min(tile_start[tile + 1], cap);
    const TexHit hit = tex_tile_nearest(s_f[wv], lane, frec, tile_list, s0, s1, is, xi, yi, near, far);
    if (yi >= is || xi >= is) return;
    const size_t o = (size_t)yi * is + xi;
    float *pp = pix + o * 5;
    pp[0] = hit.w[0]; pp[1] = hit.w[1]; pp[2] = hit.w[2]; pp[3] = hit.depth; pp[4] = __int_as_float(hit.face);
    if (!textures) return;
    float px[3] = {bg0, bg1, bg2};
    if (hit.face >= 0) {
        const bool back = hit.face >= nf;
        const int fn = back ? hit.face - nf : hit.face;
        int idx[8];
        float wt[8];
        tex_corners(hit.w, hit.depth, frec + (size_t)hit.face * BF_TEX_REC, ts, idx, wt);
        const float *tex = textures + (size_t)fn * ts * ts * ts * 3;
        float l[3] = {1.f, 1.f, 1.f};
        if (light) { l[0] = light[(size_t)hit.face * 3]; l[1] = light[(size_t)hit.face * 3 + 1]; l[2] = light[(size_t)hit.face * 3 + 2]; }
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const int at = nr_texel(idx[corner], ts, back) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] += wt[corner] * (light ? tex[at + k] * l[k] : tex[at + k]);      // textures * light, then the sampling weight
        }
        // forward_background: rgb * mask + (1 - mask) * background with mask = 1
        px[0] = acc[0] * 1.f + 0.f * bg0; px[1] = acc[1] * 1.f + 0.f * bg1; px[2] = acc[2] * 1.f + 0.f * bg2;
    }
    rgb[o * 3] = px[0]; rgb[o * 3 + 1] = px[1]; rgb[o * 3 + 2] = px[2];
}

// alpha[y][x] (out x out) from pix[is][is][5]'s record (1 where one was drawn): the same flip and 2 x 2 mean as the colours
extern "C" __global__ void __launch_bounds__(256)
bf_nr_alpha_kernel(int out, int aa, const float *__restrict__ pix, float *__restrict__ alpha) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= out * out) return;
    const int y = i / out, x = i - y * out, is = aa ? out * 2 : out;
    auto at = [&](int yy, int xx) { return __float_as_int(pix[((size_t)(is - 1 - yy) * is + xx) * 5 + 4]) >= 0 ? 1.f : 0.f; };
    alpha[i] = aa ? (at(2 * y, 2 * x) + at(2 * y, 2 * x + 1) + at(2 * y + 1, 2 * x) + at(2 * y + 1, 2 * x + 1)) * 0.25f : at(y, x);
}

// one owned pixel's contribution to cube[] (LDS or global): (sampling weight x light) x dL/drgb at the record's exchanged texel
template <class Add>
__device__ __forceinline__ void nr_pixel_vjp(const float *__restrict__ pp, const float *__restrict__ rec, const float *__restrict__ light, int k,
                                             bool back, int ts, const float g[3], Add add) {
    const float w[3] = {pp[0], pp[1], pp[2]};
    int idx[8];
    float wt[8];
    tex_corners(w, pp[3], rec, ts, idx, wt);
    float l[3] = {1.f, 1.f, 1.f};
    if (light) { l[0] = light[(size_t)k * 3]; l[1] = light[(size_t)k * 3 + 1]; l[2] = light[(size_t)k * 3 + 2]; }
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int at = nr_texel(idx[corner], ts, back) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) add(at + c, (light ? wt[corner] * l[c] : wt[corner]) * g[c]);
    }
}

// grid nf, one wave per FACE: its front record and (nrec = 2 nf) its back record.  Dynamic LDS: ts^3 * 3 floats.  A record with a box
// above BF_TEX_GATHER_MAX pixels adds nothing here and is left to bf_nr_backward_large_kernel.
extern "C" __global__ void __launch_bounds__(64)
bf_nr_backward_kernel(int nf, int nrec, int is, int out, int aa, const float *__restrict__ pix, const float *__restrict__ frec,
                      const float *__restrict__ light, int ts, const float *__restrict__ grad_image, float *__restrict__ grad_tex) {
    extern __shared__ float cube[];
    const int fn = blockIdx.x, lane = threadIdx.x, n = ts * ts * ts * 3;
    for (int i = lane; i < n; i += 64) cube[i] = 0.f;
    __builtin_amdgcn_wave_barrier();
    for (int k = fn; k < nrec; k += nf) {
        const float *rec = frec + (size_t)k * BF_TEX_REC;
        const int bx = __float_as_int(rec[18]), by = __float_as_int(rec[19]);
        const int x0 = bx & 0xffff, x1 = bx >> 16, y0 = by & 0xffff, y1 = by >> 16, W = x1 - x0 + 1, H = y1 - y0 + 1;
        if (!(W > 0 && H > 0 && W * H <= BF_TEX_GATHER_MAX)) continue;
        for (int p = lane; p < W * H; p += 64) {
            const int yi = y0 + p / W, xi = x0 + p % W;
            const float *pp = pix + ((size_t)yi * is + xi) * 5;
            if (__float_as_int(pp[4]) != k) continue;
            float g[3];
            tex_pixel_grad(yi, xi, is, out, aa, grad_image, g);
            nr_pixel_vjp(pp, rec, light, k, k >= nf, ts, g, [&](int at, float v) { atomicAdd(cube + at, v); });
        }
    }
    __builtin_amdgcn_wave_barrier();
    float *gt = grad_tex + (size_t)fn * n;
    for (int i = lane; i < n; i += 64) gt[i] = cube[i];
}

// the records the gather kernel left out (box above BF_TEX_GATHER_MAX pixels): per pixel, atomicAdd as the reference does
extern "C" __global__ void __launch_bounds__(256)
bf_nr_backward_large_kernel(int nf, int is, int out, int aa, const float *__restrict__ pix, const float *__restrict__ frec,
                            const float *__restrict__ light, int ts, const float *__restrict__ grad_image, float *__restrict__ grad_tex) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= is * is) return;
    const float *pp = pix + (size_t)i * 5;
    const int k = __float_as_int(pp[4]);
    if (k < 0) return;
    const float *rec = frec + (size_t)k * BF_TEX_REC;
    const int bx = __float_as_int(rec[18]), by = __float_as_int(rec[19]);
    if (((bx >> 16) - (bx & 0xffff) + 1) * ((by >> 16) - (by & 0xffff) + 1) <= BF_TEX_GATHER_MAX) return;
    const int yi = i / is, xi = i - yi * is;
    float g[3];
    tex_pixel_grad(yi, xi, is, out, aa, grad_image, g);
    const bool back = k >= nf;
    float *gt = grad_tex + (size_t)(back ? k - nf : k) * ts * ts * ts * 3;
    nr_pixel_vjp(pp, rec, light, k, back, ts, g, [&](int at, float v) { atomicAdd(gt + at, v); });
}
