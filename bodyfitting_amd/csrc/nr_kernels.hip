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
#include "wave_ops.h"
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

// ---- the geometry gradient: backward_pixel_map + backward_depth_map (cuda/rasterize_cuda_kernel.cu:245-503,543-592), the light's and
// the projection's reverse (lighting.py:41-52, projection.py:19-42) ----
//   bf_nr_unlit_kernel      per super-sampled pixel the texture sample WITHOUT the light, sum(wt * texel): what dL/dlight multiplies
//   bf_nr_geometry_kernel   one wave per record: the soft-edge walks (lanes share a walk's pixels), then the depth terms and dL/dlight
//                           gathered over the record's pixel box; every row of grad_frec / grad_lrec written once, fixed order
//   bf_nr_fold_kernel       one thread per vertex: its incident (record, corner) rows in table order, then the projection's reverse;
//                           per block a fixed-order tree of dp and dp (x) v
//   bf_nr_fold_view_kernel  the same body with the view read from device memory
//   bf_nr_fold_sum_kernel   the blocks' partial sums in block order -> grad_R[9], grad_t[3]
extern "C" __global__ void __launch_bounds__(256)
bf_nr_unlit_kernel(int is, int nf, const float *__restrict__ pix, const float *__restrict__ frec, const float *__restrict__ textures, int ts,
                   float *__restrict__ unlit) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= is * is) return;
    const float *pp = pix + (size_t)i * 5;
    const int k = __float_as_int(pp[4]);
    float acc[3] = {0.f, 0.f, 0.f};
    if (k >= 0) {
        const bool back = k >= nf;
        const float w[3] = {pp[0], pp[1], pp[2]};
        int idx[8];
        float wt[8];
        tex_corners(w, pp[3], frec + (size_t)k * BF_TEX_REC, ts, idx, wt);
        const float *tex = textures + (size_t)(back ? k - nf : k) * ts * ts * ts * 3;
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const int at = nr_texel(idx[corner], ts, back) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wt[corner] * tex[at + c];
        }
    }
    unlit[(size_t)i * 3] = acc[0]; unlit[(size_t)i * 3 + 1] = acc[1]; unlit[(size_t)i * 3 + 2] = acc[2];
}

// one line d0 of one edge along one axis: axis 0 walks columns (d0 = x, d1 = y), axis 1 rows (d0 = y, d1 = x)
struct NrLine { float p00, p10, cross; int d0, axis; };

__device__ __forceinline__ size_t nr_line_pixel(const NrLine &ln, int d1, int is) {
    return ln.axis == 0 ? (size_t)d1 * is + ln.d0 : (size_t)ln.d0 * is + d1;
}

// diff_grad of pixel o against the reference pixel's (alpha, rgb): (alpha - alpha_ref) g_alpha, then the three colour terms, float32
__device__ __forceinline__ float nr_diff_grad(const NrGeo &G, size_t o, float a_ref, const float rgb_ref[3]) {
    const int yi = (int)(o / G.is), xi = (int)(o - (size_t)yi * G.is);
    float diff = 0.f;
    if (G.g_alpha) {
        const float a = __float_as_int(G.pix[o * 5 + 4]) >= 0 ? 1.f : 0.f;
        diff += (a - a_ref) * tex_pixel_grad1(yi, xi, G.is, G.out, G.aa, G.g_alpha);
    }
    if (G.g_rgb) {
        float g[3];
        tex_pixel_grad(yi, xi, G.is, G.out, G.aa, G.g_rgb, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) diff += (G.rgbmap[o * 3 + c] - rgb_ref[c]) * g[c];
    }
    return diff;
}

// pixels d1 in [from, to] of a line, dealt to the lanes: acc0 / acc1 -= diff_grad / dist for the edge's two end points.  own >= 0: only
// pixels whose record is `own` (the "in" walk)
__device__ __forceinline__ void nr_walk(const NrGeo &G, const NrLine &ln, int from, int to, int own, int lane, float a_ref, const float rgb_ref[3],
                                        float &acc0, float &acc1) {
    const float fd0 = (float)ln.d0;
    for (int d1 = from + lane; d1 <= to; d1 += 64) {
        const size_t o = nr_line_pixel(ln, d1, G.is);
        if (own >= 0 && __float_as_int(G.pix[o * 5 + 4]) != own) continue;
        const float diff = nr_diff_grad(G, o, a_ref, rgb_ref);
        if (diff <= 0.f) continue;
        const float off = (float)d1 - ln.cross;
        if (ln.p10 != fd0) acc0 -= diff / tex_edge_dist(ln.p10 - ln.p00, ln.p10 - fd0, off, G.is);
        if (ln.p00 != fd0) acc1 -= diff / tex_edge_dist(ln.p10 - ln.p00, fd0 - ln.p00, off, G.is);
    }
}

// grid nrec, one wave per record k.  grad_frec[nrec][3][3]: dL/d(the record's projected corners); grad_lrec[nrec][3][3] (NULL unless
// the render was lit with a directional term and has an rgb cotangent): dL/d(its world-space corners) through its light row.
extern "C" __global__ void __launch_bounds__(64)
bf_nr_geometry_kernel(NrGeo G, NrLight L, float *__restrict__ grad_frec, float *__restrict__ grad_lrec) {
    __shared__ float s_g[9], s_p[6];
    const int k = blockIdx.x, lane = threadIdx.x, is = G.is;
    const bool back = k >= G.nf;
    const int fn = back ? k - G.nf : k;
    int vid[3];
    float f[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        vid[c] = G.faces[(size_t)fn * 3 + (back ? 2 - c : c)];
        const float *v = G.pv + (size_t)vid[c] * 3;
        f[c * 3] = v[0]; f[c * 3 + 1] = v[1]; f[c * 3 + 2] = v[2];
    }
    const TexTri tri = tex_tri(f);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) s_g[i] = 0.f;
#pragma unroll
        for (int n = 0; n < 3; ++n) { s_p[2 * n] = 0.5f * (tri.x[n] * is + is - 1); s_p[2 * n + 1] = 0.5f * (tri.y[n] * is + is - 1); }
    }
    __builtin_amdgcn_wave_barrier();
    const bool shown = !tex_back_facing(tri);                        // (:270 - a record that shows its back gets zeros)
    if (shown && (G.g_rgb || G.g_alpha)) {
        for (int e = 0; e < 3; ++e) {
            const int i0 = e, i1 = (e + 1) % 3, i2 = (e + 2) % 3;
            for (int axis = 0; axis < 2; ++axis) {
                const float p00 = s_p[2 * i0 + axis], p01 = s_p[2 * i0 + 1 - axis], p10 = s_p[2 * i1 + axis], p11 = s_p[2 * i1 + 1 - axis];
                const float p20 = s_p[2 * i2 + axis], p21 = s_p[2 * i2 + 1 - axis];
                if (p00 == p10) continue;                            // axis-parallel: no line, or the reference's 0 / 0 at an integer coordinate
                const int direction = (axis == 0) == (p00 < p10) ? -1 : 1;
                const int d0_from = (int)fmaxf(fminf(ceilf(fminf(p00, p10)), (float)is), 0.f);
                const int d0_to = (int)fminf(fmaxf(fmaxf(p00, p10), -2.f), is - 1.f);        // ((int) truncates: (-1, 0) -> 0 as in the reference)
                float acc0 = 0.f, acc1 = 0.f;
                for (int d0 = d0_from; d0 <= d0_to; ++d0) {
                    NrLine ln{p00, p10, tex_edge_cross(p00, p01, p10, p11, (float)d0), d0, axis};
                    if (!(ln.cross > -2.f && ln.cross < is + 1.f)) continue;                 // (d1_in would be off the image)
                    const int d1_in = direction > 0 ? (int)floorf(ln.cross) : (int)ceilf(ln.cross), d1_out = d1_in + direction;
                    if (d1_in < 0 || is <= d1_in || d1_out < 0 || is <= d1_out) continue;
                    const size_t o_in = nr_line_pixel(ln, d1_in, is), o_out = nr_line_pixel(ln, d1_out, is);
                    const int k_in = __float_as_int(G.pix[o_in * 5 + 4]), k_out = __float_as_int(G.pix[o_out * 5 + 4]);
                    float rgb_in[3] = {0.f, 0.f, 0.f}, rgb_out[3] = {0.f, 0.f, 0.f};
                    if (G.g_rgb) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) { rgb_in[c] = G.rgbmap[o_in * 3 + c]; rgb_out[c] = G.rgbmap[o_out * 3 + c]; }
                    }
                    if (k_in == k) {                                 // out: from the crossing to the image border
                        const int lim = direction > 0 ? is - 1 : 0;
                        nr_walk(G, ln, max(min(d1_out, lim), 0), min(max(d1_out, lim), is - 1), -1, lane, k_in >= 0 ? 1.f : 0.f, rgb_in, acc0, acc1);
                    }
                    {                                                // in: from the crossing to the other edge, over this record's pixels
                        const float fd0 = (float)d0;
                        const float c2 = (fd0 - p00) * (fd0 - p20) < 0 ? tex_edge_cross(p00, p01, p20, p21, fd0) : tex_edge_cross(p20, p21, p10, p11, fd0);
                        const int lim = tex_to_int(direction > 0 ? ceilf(c2) : floorf(c2), -1, is);
                        nr_walk(G, ln, max(min(d1_in, lim), 0), min(max(d1_in, lim), is - 1), k, lane, k_out >= 0 ? 1.f : 0.f, rgb_out, acc0, acc1);
                    }
                }
                acc0 = bf_wave_sum(acc0); acc1 = bf_wave_sum(acc1);
                if (lane == 0) { s_g[i0 * 3 + 1 - axis] += acc0; s_g[i1 * 3 + 1 - axis] += acc1; }
            }
        }
    }
    // depth terms and dL/dlight: the pixels this record owns, gathered over its box
    float gd[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dl[3] = {0.f, 0.f, 0.f};
    const float *rec = G.frec + (size_t)k * BF_TEX_REC;
    const int bx = __float_as_int(rec[18]), by = __float_as_int(rec[19]);
    const int x0 = bx & 0xffff, x1 = bx >> 16, y0 = by & 0xffff, y1 = by >> 16, W = x1 - x0 + 1, H = y1 - y0 + 1;
    if (W > 0 && H > 0 && (G.g_depth || grad_lrec)) {
        float tmp[2] = {0.f, 0.f};
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) tmp[l] += -rec[9 + 3 * m + l] / rec[3 * m + 2];
        for (int p = lane; p < W * H; p += 64) {
            const int yi = y0 + p / W, xi = x0 + p % W;
            const size_t o = (size_t)yi * is + xi;
            const float *pp = G.pix + o * 5;
            if (__float_as_int(pp[4]) != k) continue;
            if (G.g_depth) {
                const float g = tex_pixel_grad1(yi, xi, is, G.out, G.aa, G.g_depth), depth2 = pp[3] * pp[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float z = rec[3 * c + 2];
                    gd[3 * c + 2] += g * pp[c] * depth2 / (z * z);
#pragma unroll
                    for (int l = 0; l < 2; ++l) gd[3 * c + l] += -g * tmp[l] * pp[c] * depth2 * is / 2;
                }
            }
            if (grad_lrec) {
                float g[3];
                tex_pixel_grad(yi, xi, is, G.out, G.aa, G.g_rgb, g);
#pragma unroll
                for (int c = 0; c < 3; ++c) dl[c] += G.unlit[o * 3 + c] * g[c];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) gd[i] = bf_wave_sum(gd[i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) dl[c] = bf_wave_sum(dl[c]);
    __builtin_amdgcn_wave_barrier();
    if (lane != 0) return;
#pragma unroll
    for (int i = 0; i < 9; ++i) grad_frec[(size_t)k * 9 + i] = s_g[i] + gd[i];
    if (!grad_lrec) return;
    // the reverse of nr_face_light: light = .. + directional * (color * relu(n^ . d)), n^ = n / max(|n|, 1e-5), n = (c0 - c1) x (c2 - c1)
    float out[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float *c0 = G.verts + (size_t)vid[0] * 3, *c1 = G.verts + (size_t)vid[1] * 3, *c2 = G.verts + (size_t)vid[2] * 3;
    float a[3], b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = c0[c] - c1[c]; b[c] = c2[c] - c1[c]; }
    const float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float norm = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), len = fmaxf(norm, 1e-5f);
    const float nh[3] = {n[0] / len, n[1] / len, n[2] / len};
    const float s = (nh[0] * L.direction[0] + nh[1] * L.direction[1]) + nh[2] * L.direction[2];
    if (s > 0.f) {                                                   // (relu: derivative 0 at 0)
        const float dcos = L.directional * ((dl[0] * L.color_directional[0] + dl[1] * L.color_directional[1]) + dl[2] * L.color_directional[2]);
        float dn[3] = {dcos * L.direction[0], dcos * L.direction[1], dcos * L.direction[2]};       // d / d n^
        if (norm >= 1e-5f) {                                         // (below it the denominator is the constant 1e-5)
            const float along = (nh[0] * dn[0] + nh[1] * dn[1]) + nh[2] * dn[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) dn[c] = dn[c] - nh[c] * along;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dn[c] = dn[c] / len;
        const float da[3] = {b[1] * dn[2] - b[2] * dn[1], b[2] * dn[0] - b[0] * dn[2], b[0] * dn[1] - b[1] * dn[0]};       // b x dn
        const float db[3] = {dn[1] * a[2] - dn[2] * a[1], dn[2] * a[0] - dn[0] * a[2], dn[0] * a[1] - dn[1] * a[0]};       // dn x a
#pragma unroll
        for (int c = 0; c < 3; ++c) { out[c] = da[c]; out[3 + c] = -(da[c] + db[c]); out[6 + c] = db[c]; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) grad_lrec[(size_t)k * 9 + i] = out[i];
}

// thread = vertex i.  vstart[nv + 1], ventry[]: its (record * 3 + corner) rows, ascending; rows of records >= nrec are not drawn.
// V.orig < 0 (ndc): grad_verts is the sum itself.  partial[blocks][12]: the block's sums of dp (x) v [9] | dp [3], NULL with ndc.
// (the one body of bf_nr_fold_kernel and bf_nr_fold_view_kernel: V by value or through a pointer; s_r: the block's [12][256] floats)
__device__ __forceinline__ void nr_fold(int nv, int nrec, const int *__restrict__ vstart, const int *__restrict__ ventry, const float *__restrict__ grad_frec,
                                        const float *__restrict__ grad_lrec, const float *__restrict__ verts, const TexView &V,
                                        float *__restrict__ grad_verts, float *__restrict__ partial, float (*s_r)[256]) {
    const int i = blockIdx.x * 256 + threadIdx.x, tid = threadIdx.x;
    float gn[3] = {0.f, 0.f, 0.f}, gw[3] = {0.f, 0.f, 0.f}, red[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < nv) {
        for (int e = vstart[i]; e < vstart[i + 1]; ++e) {
            const int row = ventry[e];
            if (row >= nrec * 3) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) gn[c] += grad_frec[(size_t)row * 3 + c];
            if (grad_lrec) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gw[c] += grad_lrec[(size_t)row * 3 + c];
            }
        }
        float gv[3];
        if (V.orig < 0.f) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gv[c] = gn[c] + gw[c];
        } else {
            const float a = verts[(size_t)i * 3], b = verts[(size_t)i * 3 + 1], c = verts[(size_t)i * 3 + 2];
            const float x = ((a * V.R[0] + b * V.R[1]) + c * V.R[2]) + V.t[0];
            const float y = ((a * V.R[3] + b * V.R[4]) + c * V.R[5]) + V.t[1];
            const float z = ((a * V.R[6] + b * V.R[7]) + c * V.R[8]) + V.t[2];
            const float zi = z + 1e-9f;
            const float du = gn[0] * 2.f / V.orig, dw = -(gn[1] * 2.f / V.orig);      // u = 2 (u - orig / 2) / orig; v = orig - v first
            const float dx_ = du * V.K[0] + dw * V.K[3], dy_ = du * V.K[1] + dw * V.K[4];
            const float dp[3] = {dx_ / zi, dy_ / zi, gn[2] - (dx_ * x + dy_ * y) / (zi * zi)};
            const float v[3] = {a, b, c};
#pragma unroll
            for (int j = 0; j < 3; ++j) gv[j] = ((V.R[j] * dp[0] + V.R[3 + j] * dp[1]) + V.R[6 + j] * dp[2]) + gw[j];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                red[9 + r] = dp[r];
#pragma unroll
                for (int j = 0; j < 3; ++j) red[3 * r + j] = dp[r] * v[j];
            }
        }
        grad_verts[(size_t)i * 3] = gv[0]; grad_verts[(size_t)i * 3 + 1] = gv[1]; grad_verts[(size_t)i * 3 + 2] = gv[2];
    }
    if (!partial) return;                                            // (block-uniform)
#pragma unroll
    for (int q = 0; q < 12; ++q) s_r[q][tid] = red[q];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 12; ++q) s_r[q][tid] += s_r[q][tid + s];
        }
        __syncthreads();
    }
    if (tid < 12) partial[(size_t)blockIdx.x * 12 + tid] = s_r[tid][0];
}

extern "C" __global__ void __launch_bounds__(256)
bf_nr_fold_kernel(int nv, int nrec, const int *__restrict__ vstart, const int *__restrict__ ventry, const float *__restrict__ grad_frec,
                  const float *__restrict__ grad_lrec, const float *__restrict__ verts, TexView V, float *__restrict__ grad_verts,
                  float *__restrict__ partial) {
    __shared__ float s_r[12][256];
    nr_fold(nv, nrec, vstart, ventry, grad_frec, grad_lrec, verts, V, grad_verts, partial, s_r);
}

// ... with the view where bf_tex_view_pack_kernel wrote it (4-byte aligned)
extern "C" __global__ void __launch_bounds__(256)
bf_nr_fold_view_kernel(int nv, int nrec, const int *__restrict__ vstart, const int *__restrict__ ventry, const float *__restrict__ grad_frec,
                       const float *__restrict__ grad_lrec, const float *__restrict__ verts, const TexView *__restrict__ V,
                       float *__restrict__ grad_verts, float *__restrict__ partial) {
    __shared__ float s_r[12][256];
    nr_fold(nv, nrec, vstart, ventry, grad_frec, grad_lrec, verts, *V, grad_verts, partial, s_r);
}

// one block of 64: lane q < 12 adds the blocks' partial sums in block order -> out_R[9] = grad_R, out_t[3] = grad_t (each may be NULL)
extern "C" __global__ void __launch_bounds__(64)
bf_nr_fold_sum_kernel(int blocks, const float *__restrict__ partial, float *__restrict__ out_R, float *__restrict__ out_t) {
    const int q = threadIdx.x;
    if (q >= 12) return;
    float *dst = q < 9 ? (out_R ? out_R + q : nullptr) : (out_t ? out_t + (q - 9) : nullptr);
    if (!dst) return;
    float s = 0.f;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * 12 + q];
    *dst = s;
}
