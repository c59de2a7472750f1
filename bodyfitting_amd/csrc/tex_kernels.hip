// Texture fitting (reference smplify/texture_fitting.py:240-275): the slice of neural_renderer its loop exercises, for gfx950.
// Compiled with -ffp-contract=off: the reference kernels' float32 operation order is kept literally (an edge test that
// flips on a contracted fma moves a pixel from one face to another).
//
//   bf_tex_project_kernel   neural_renderer/projection.py:6-42, zero distortion: world -> (u, v in [-1,1], z)
//   bf_tex_view_pack_kernel / bf_tex_project_view_kernel   the camera packed into device memory, and the projection reading it there
//   bf_tex_face_kernel      forward_face_index_map_cuda_kernel_1 (cuda/rasterize_cuda_kernel.cu:24-68): per face the nine projected
//                           coordinates, the back-face test, the inverted pixel-space triangle; + the 8x8-pixel tiles its bounding
//                           box touches (count pass / fill pass of the tile lists)
//   bf_tex_raster_kernel    forward_face_index_map_cuda_kernel_2 (:70-174) + forward_texture_sampling (:177-252) +
//                           forward_background (rasterize.py:181-190): one wave per tile, lane = pixel.  The reference walks ALL
//                           faces for every pixel; here a pixel walks the faces of its tile (staged through LDS 64 at a time) and
//                           keeps the lexicographic (depth, face index) minimum - the reference's strict `<` in face order - so the
//                           result does not depend on the order of the list.
//   bf_tex_compose_kernel   permute, vertical flip, 2x2 average pooling (rasterize.py:300-318) -> image[3][is][is]
//   bf_tex_loss_kernel      sum |a - b| (texture_fitting.py:266) and its derivative sign(b - a)
//   bf_tex_backward_kernel  backward_textures_cuda_kernel (:498-540) through pooling / flip / background mask: atomicAdd of
//                           sampling weight x dL/drgb into the face's texture cube (sampling indices / weights recomputed from
//                           the stored weights and depth: 20 bytes per pixel kept instead of 64)
//   bf_tex_adam_kernel      torch.optim.Adam (defaults) on every texel
//   bf_tex_load_kernel      load_textures_cuda_kernel (cuda/load_textures_cuda_kernel.cu): the per-face texture cubes of nr.load_obj
#include "bf_internal.h"
#include "tex_kernels.h"
#include "tex_bodies.h"       // the arithmetic shared with nr_kernels.hip: projection, face record, edge tests, weights, sampling corners

extern "C" __global__ void __launch_bounds__(256)
bf_tex_project_kernel(int nv, const float *__restrict__ verts, TexView V, float *__restrict__ pv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const float a = verts[i * 3], b = verts[i * 3 + 1], c = verts[i * 3 + 2];
    tex_project(V, a, b, c, pv + i * 3);
}

// the view in device memory (bf_nr_render_dev): 22 floats, thread = float.  Plain loads and stores; one block of 64.
extern "C" __global__ void __launch_bounds__(64)
bf_tex_view_pack_kernel(const float *__restrict__ d_K, const float *__restrict__ d_R, const float *__restrict__ d_t, TexView host, TexView *__restrict__ out) {
    const int i = threadIdx.x;
    float *o = (float *)out;
    if (i < 9) o[i] = d_R ? d_R[i] : host.R[i];
    else if (i < 12) o[i] = d_t ? d_t[i - 9] : host.t[i - 9];
    else if (i < 21) o[i] = d_K ? d_K[i - 12] : host.K[i - 12];
    else if (i == 21) o[i] = host.orig;
}

extern "C" __global__ void __launch_bounds__(256)
bf_tex_project_view_kernel(int nv, const float *__restrict__ verts, const TexView *__restrict__ V, float *__restrict__ pv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const float a = verts[i * 3], b = verts[i * 3 + 1], c = verts[i * 3 + 2];
    tex_project(*V, a, b, c, pv + i * 3);
}

// pass 0: the record + count the tiles of the box; pass 1: write the face into their lists (tex_bodies.h: tex_face_record)
extern "C" __global__ void __launch_bounds__(256)
bf_tex_face_kernel(int nf, const int *__restrict__ faces, const float *__restrict__ pv, int is, int tiles, float *__restrict__ frec,
                   int *__restrict__ tile_count, int *__restrict__ cursor, int *__restrict__ tile_list, int pass, int cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    float f[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *v = pv + (size_t)faces[i * 3 + c] * 3;
        f[c * 3] = v[0]; f[c * 3 + 1] = v[1]; f[c * 3 + 2] = v[2];
    }
    tex_face_record(i, f, is, tiles, frec, tile_count, cursor, tile_list, pass, cap);
}

// grid (tiles * tiles / 4), 256 threads: wave = tile, lane = pixel (8 x 8).  pix[is][is] = (w0, w1, w2, depth, face) per pixel,
// rgb[is][is][3] with the background filled in.
extern "C" __global__ void __launch_bounds__(256)
bf_tex_raster_kernel(int is, int tiles, const float *__restrict__ frec, const int *__restrict__ tile_start, const int *__restrict__ tile_list,
                     const float *__restrict__ textures, int ts, float near, float far, float bg0, float bg1, float bg2,
                     float *__restrict__ pix, float *__restrict__ rgb, int cap) {
    __shared__ float s_f[4][64][19];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, tile = blockIdx.x * 4 + wv;
    if (tile >= tiles * tiles) return;                     // (wave-uniform)
    const int ty = tile / tiles, tx = tile - ty * tiles;
    const int yi = ty * BF_TEX_TILE + (lane >> 3), xi = tx * BF_TEX_TILE + (lane & 7);
    const int s0 = min(tile_start[tile], cap), s1 = min(tile_start[tile + 1], cap);
    const TexHit hit = tex_tile_nearest(s_f[wv], lane, frec, tile_list, s0, s1, is, xi, yi, near, far);
    const float depth_min = hit.depth, wmin[3] = {hit.w[0], hit.w[1], hit.w[2]};
    const int fmin = hit.face;
    if (yi >= is || xi >= is) return;
    const size_t o = (size_t)yi * is + xi;
    float px[3] = {bg0, bg1, bg2};
    if (fmin >= 0) {
        int idx[8];
        float wt[8];
        tex_corners(wmin, depth_min, frec + (size_t)fmin * BF_TEX_REC, ts, idx, wt);
        const float *tex = textures + (size_t)fmin * ts * ts * ts * 3;
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int corner = 0; corner < 8; ++corner)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] += wt[corner] * (tex[idx[corner] * 3 + k] * 1.0f);      // (x 1: ambient light, lighting.py:33-37)
        // forward_background: rgb * mask + (1 - mask) * background with mask = 1
        px[0] = acc[0] * 1.f + 0.f * bg0; px[1] = acc[1] * 1.f + 0.f * bg1; px[2] = acc[2] * 1.f + 0.f * bg2;
    }
    rgb[o * 3] = px[0]; rgb[o * 3 + 1] = px[1]; rgb[o * 3 + 2] = px[2];
    float *pp = pix + o * 5;
    pp[0] = wmin[0]; pp[1] = wmin[1]; pp[2] = wmin[2]; pp[3] = depth_min; pp[4] = __int_as_float(fmin);
}

// image[c][y][x] (out x out) from rgb[is][is][3]: vertical flip, then (aa) the mean of the 2 x 2 block
extern "C" __global__ void __launch_bounds__(256)
bf_tex_compose_kernel(int out, int aa, const float *__restrict__ rgb, float *__restrict__ image) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * out * out) return;
    const int c = i / (out * out), r = i - c * out * out, y = r / out, x = r - y * out;
    const int is = aa ? out * 2 : out;
    auto at = [&](int yy, int xx) { return rgb[((size_t)(is - 1 - yy) * is + xx) * 3 + c]; };      // flipped row yy
    image[i] = aa ? (at(2 * y, 2 * x) + at(2 * y, 2 * x + 1) + at(2 * y + 1, 2 * x) + at(2 * y + 1, 2 * x + 1)) * 0.25f : at(y, x);
}

// depth[y][x] (out x out) from pix[is][is][5]'s depth (far where no face was drawn): the same flip and 2 x 2 mean as the colours
extern "C" __global__ void __launch_bounds__(256)
bf_tex_depth_kernel(int out, int aa, const float *__restrict__ pix, float *__restrict__ depth) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= out * out) return;
    const int y = i / out, x = i - y * out, is = aa ? out * 2 : out;
    auto at = [&](int yy, int xx) { return pix[((size_t)(is - 1 - yy) * is + xx) * 5 + 3]; };
    depth[i] = aa ? (at(2 * y, 2 * x) + at(2 * y, 2 * x + 1) + at(2 * y + 1, 2 * x) + at(2 * y + 1, 2 * x + 1)) * 0.25f : at(y, x);
}

// partial[block] = sum |a - b| over the block's elements (fixed order inside a block; the host adds the blocks in order);
// grad[i] = sign(b - a)
extern "C" __global__ void __launch_bounds__(256)
bf_tex_loss_kernel(int n, const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ grad, double *__restrict__ partial) {
    __shared__ double s[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        const float d = b[i] - a[i];
        v = (double)fabsf(d);                        // |a - b| in float32 as torch forms it; the sum in double
        grad[i] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

// backward_textures, gathered per face: one wave per face walks the face's pixel box, adds the pixels it owns into the face's
// texture cube in LDS and stores the cube (every texel of every face is written: no clearing pass, no global atomics).
// Dynamic LDS: ts^3 * 3 floats.  Faces with a box above BF_TEX_GATHER_MAX pixels store zeros and are left to
// bf_tex_backward_large_kernel.
extern "C" __global__ void __launch_bounds__(64)
bf_tex_backward_kernel(int nf, int is, int out, int aa, const float *__restrict__ pix, const float *__restrict__ frec, int ts,
                       const float *__restrict__ grad_image, float *__restrict__ grad_tex) {
    extern __shared__ float cube[];
    const int fn = blockIdx.x, lane = threadIdx.x, n = ts * ts * ts * 3;
    const float *rec = frec + (size_t)fn * BF_TEX_REC;
    for (int i = lane; i < n; i += 64) cube[i] = 0.f;
    __builtin_amdgcn_wave_barrier();
    const int bx = __float_as_int(rec[18]), by = __float_as_int(rec[19]);
    const int x0 = bx & 0xffff, x1 = bx >> 16, y0 = by & 0xffff, y1 = by >> 16, W = x1 - x0 + 1, H = y1 - y0 + 1;
    if (W > 0 && H > 0 && W * H <= BF_TEX_GATHER_MAX) {
        for (int p = lane; p < W * H; p += 64) {
            const int yi = y0 + p / W, xi = x0 + p % W;
            const float *pp = pix + ((size_t)yi * is + xi) * 5;
            if (__float_as_int(pp[4]) != fn) continue;
            float g[3];
            tex_pixel_grad(yi, xi, is, out, aa, grad_image, g);
            const float w[3] = {pp[0], pp[1], pp[2]};
            int idx[8];
            float wt[8];
            tex_corners(w, pp[3], rec, ts, idx, wt);
#pragma unroll
            for (int corner = 0; corner < 8; ++corner)
#pragma unroll
                for (int c = 0; c < 3; ++c) atomicAdd(cube + idx[corner] * 3 + c, wt[corner] * g[c]);
        }
    }
    __builtin_amdgcn_wave_barrier();
    float *gt = grad_tex + (size_t)fn * n;
    for (int i = lane; i < n; i += 64) gt[i] = cube[i];
}

// the faces the gather kernel left out (box above BF_TEX_GATHER_MAX pixels): per pixel, atomicAdd as the reference does
extern "C" __global__ void __launch_bounds__(256)
bf_tex_backward_large_kernel(int is, int out, int aa, const float *__restrict__ pix, const float *__restrict__ frec, int ts,
                             const float *__restrict__ grad_image, float *__restrict__ grad_tex) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= is * is) return;
    const float *pp = pix + (size_t)i * 5;
    const int fn = __float_as_int(pp[4]);
    if (fn < 0) return;
    const float *rec = frec + (size_t)fn * BF_TEX_REC;
    const int bx = __float_as_int(rec[18]), by = __float_as_int(rec[19]);
    if (((bx >> 16) - (bx & 0xffff) + 1) * ((by >> 16) - (by & 0xffff) + 1) <= BF_TEX_GATHER_MAX) return;
    const int yi = i / is, xi = i - yi * is;
    float g[3];
    tex_pixel_grad(yi, xi, is, out, aa, grad_image, g);
    const float w[3] = {pp[0], pp[1], pp[2]};
    int idx[8];
    float wt[8];
    tex_corners(w, pp[3], rec, ts, idx, wt);
    float *gt = grad_tex + (size_t)fn * ts * ts * ts * 3;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner)
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(gt + idx[corner] * 3 + c, wt[corner] * g[c]);
}

// torch.optim.Adam, single-tensor form
extern "C" __global__ void __launch_bounds__(256)
bf_tex_adam_kernel(size_t n, float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, const float *__restrict__ g,
                   float step_size, float bc2_sqrt, float omb1, float beta2, float omb2, float eps) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = m[i] + (gi - m[i]) * omb1;             // lerp_(grad, 1 - beta1): the weight is formed in double on the host, like torch's python float
    const float vi = v[i] * beta2 + gi * gi * omb2;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] - step_size * (mi / denom);
    m[i] = mi; v[i] = vi;
}

// ---- texture loading: load_textures_cuda_kernel (thirdparty/neural_renderer/neural_renderer/cuda/load_textures_cuda_kernel.cu), which
// nr.load_obj(..., load_texture=True) runs once per material with a texture image.  Here ONE launch covers every face: face_image[fn]
// names the face's image (-1: none - the face keeps face_fill, the 0.5 default or its material's Kd).  Thread = texel (i over
// n_faces * ts^3, as in the reference), each writes its whole texel: a wave stores 64 consecutive 12-byte texels.
// The image is the decoded file as uint8 [h][w][3], top row first; the reference's image[::-1] and / 255. happen here (the row
// index is mirrored, the byte goes through lut[256] = float32(b) / 255, the division numpy does).
// Wrapping is applied ONCE per face, to the face's own copy of its UV corners.  (The reference wraps the shared `faces` array in
// place from every thread of the face; where mod() is not idempotent - exact integers, MIRRORED_REPEAT at integer boundaries - its
// result depends on how many threads got there first.  DESIGN.md section 2.)
#define BF_TEX_REPEAT 0
#define BF_TEX_MIRRORED_REPEAT 1
#define BF_TEX_CLAMP_TO_EDGE 2
#define BF_TEX_CLAMP_TO_BORDER 3

__device__ __forceinline__ float tex_mod(float x, float y) { return x > 0.f ? fmodf(x, y) : y + fmodf(x, y); }

// one channel of the flipped, normalised image at (row y, column x) of the flipped image; indices kept inside the image (a no-op
// for every finite UV: the wrapped corners lie in [0, 1])
__device__ __forceinline__ float tex_texel(const TexImage &I, const float *lut, int y, int x, int k) {
    y = min(max(y, 0), I.h - 1);
    x = min(max(x, 0), I.w - 1);
    return lut[I.p[((size_t)(I.h - 1 - y) * I.w + x) * 3 + k]];
}

extern "C" __global__ void __launch_bounds__(256)
bf_tex_load_kernel(long long n_texels, int ts, const float *__restrict__ face_uv, const int *__restrict__ face_image,
                   const float *__restrict__ face_fill, const TexImage *__restrict__ images, const float *__restrict__ lut_g,
                   int wrapping, int bilinear, float *__restrict__ textures) {
    __shared__ float lut[256];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_texels) return;
    const int t3 = ts * ts * ts;
    const long long fn = i / t3;
    const int r = (int)(i - fn * t3);
    float *out = textures + i * 3;
    const int img = face_image[fn];
    if (img < 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = face_fill[fn * 3 + k];
        return;
    }
    if (wrapping == BF_TEX_CLAMP_TO_BORDER) {             // (the reference samples nothing and writes 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = 0.f;
        return;
    }
    // the barycentric position of the texel: computed in double, stored as float, renormalised by the float sum
    float dim0 = (float)((r / (ts * ts)) / (ts - 1.)), dim1 = (float)(((r / ts) % ts) / (ts - 1.)), dim2 = (float)((r % ts) / (ts - 1.));
    if (0 < dim0 + dim1 + dim2) {
        const float sum = dim0 + dim1 + dim2;
        dim0 /= sum; dim1 /= sum; dim2 /= sum;
    }
    float f[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float x = face_uv[fn * 6 + k];
        if (wrapping == BF_TEX_REPEAT) f[k] = tex_mod(x, 1.f);
        else if (wrapping == BF_TEX_MIRRORED_REPEAT) f[k] = tex_mod(x, 2.f) < 1 ? tex_mod(x, 1.f) : 1 - tex_mod(x, 1.f);
        else f[k] = fmaxf(fminf(x, 1.f), 0.f);
    }
    const TexImage I = images[img];
    const float pos_x = ((f[0] * dim0 + f[2] * dim1) + f[4] * dim2) * (float)(I.w - 1);
    const float pos_y = ((f[1] * dim0 + f[3] * dim1) + f[5] * dim2) * (float)(I.h - 1);
    if (bilinear) {
        const float weight_x1 = pos_x - (int)pos_x, weight_x0 = 1 - weight_x1;
        const float weight_y1 = pos_y - (int)pos_y, weight_y0 = 1 - weight_y1;
        const int x0 = (int)pos_x, y0 = (int)pos_y, x1 = min((int)pos_x + 1, I.w - 1), y1 = min((int)(pos_y + 1), I.h - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float c = 0;
            c += tex_texel(I, lut, y0, x0, k) * (weight_x0 * weight_y0);
            c += tex_texel(I, lut, y1, x0, k) * (weight_x0 * weight_y1);
            c += tex_texel(I, lut, y0, x1, k) * (weight_x1 * weight_y0);
            c += tex_texel(I, lut, y1, x1, k) * (weight_x1 * weight_y1);
            out[k] = c;
        }
    } else {
        const int xi = (int)roundf(pos_x), yi = (int)roundf(pos_y);          // (roundf: half away from zero, as CUDA's round)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = tex_texel(I, lut, yi, xi, k);
    }
}
