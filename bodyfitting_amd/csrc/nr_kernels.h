// What nr_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

// Renderer's light (neural_renderer/lighting.py:5-57).  on = 0: `lightoff` - the textures are sampled as they are.
struct NrLight { float ambient, directional, color_ambient[3], color_directional[3], direction[3]; int on; };

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
#pragma GCC visibility pop
