// What nr_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"
#include "tex_kernels.h"

// Renderer's light (neural_renderer/lighting.py:5-57).  on = 0: `lightoff` - the textures are sampled as they are.
struct NrLight { float ambient, directional, color_ambient[3], color_directional[3], direction[3]; int on; };

// What the geometry gradient reads of one taped render (device pointers).  g_*: the cotangents of the pooled outputs,
// [3][out][out] / [out][out], NULL = zero.  rgbmap[is][is][3]: the super-sampled colours with the background; unlit: without light.
struct NrGeo {
    const int *faces;
    const float *pv, *verts, *pix, *frec, *rgbmap, *unlit, *g_rgb, *g_depth, *g_alpha;
    int nf, nrec, is, out, aa;
};

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_nr_face_kernel(int nf, int nrec, const int *faces, const float *pv, const float *verts, NrLight L, int is, int tiles, float *frec,
                                             float *light, int *tile_count, int *cursor, int *tile_list, int pass, int cap);
extern "C" __global__ void bf_nr_raster_kernel(int is, int tiles, int nf, const float *frec, const float *light, const int *tile_start, const int *tile_list,
                                               const float *textures, int ts, float near, float far, float bg0, float bg1, float bg2, float *pix,
                                               float *rgb, int cap);
extern "C" __global__ void bf_nr_alpha_kernel(int out, int aa, const float *pix, float *alpha);
extern "C" __global__ void bf_nr_backward_kernel(int nf, int nrec, int is, int out, int aa, const float *pix, const float *frec, const float *light, int ts,
                                                 const float *grad_image, float *grad_tex);
extern "C" __global__ void bf_nr_backward_large_kernel(int nf, int is, int out, int aa, const float *pix, const float *frec, const float *light, int ts,
                                                       const float *grad_image, float *grad_tex);
extern "C" __global__ void bf_nr_unlit_kernel(int is, int nf, const float *pix, const float *frec, const float *textures, int ts, float *unlit);
extern "C" __global__ void bf_nr_geometry_kernel(NrGeo G, NrLight L, float *grad_frec, float *grad_lrec);
extern "C" __global__ void bf_nr_fold_kernel(int nv, int nrec, const int *vstart, const int *ventry, const float *grad_frec, const float *grad_lrec,
                                             const float *verts, TexView V, float *grad_verts, float *partial);
extern "C" __global__ void bf_nr_fold_view_kernel(int nv, int nrec, const int *vstart, const int *ventry, const float *grad_frec, const float *grad_lrec,
                                                  const float *verts, const TexView *V, float *grad_verts, float *partial);
extern "C" __global__ void bf_nr_fold_sum_kernel(int blocks, const float *partial, float *out_R, float *out_t);
#pragma GCC visibility pop
