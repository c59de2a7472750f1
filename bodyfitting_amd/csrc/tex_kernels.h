// What tex_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

struct TexView { float R[9], t[3], K[9], orig; };
struct TexImage { const unsigned char *p; int h, w; };

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_tex_project_kernel(int nv, const float *verts, TexView V, float *pv);
// the camera of a render in device memory: each of K, R, t from a device pointer (d_*, not NULL) or from `host`'s values; orig from host
extern "C" __global__ void bf_tex_view_pack_kernel(const float *d_K, const float *d_R, const float *d_t, TexView host, TexView *out);
// bf_tex_project_kernel with the view read through a pointer (4-byte aligned): the same arithmetic, the same bits
extern "C" __global__ void bf_tex_project_view_kernel(int nv, const float *verts, const TexView *V, float *pv);
extern "C" __global__ void bf_tex_face_kernel(int nf, const int *faces, const float *pv, int is, int tiles, float *frec, int *tile_count, int *cursor,
                                              int *tile_list, int pass, int cap);
extern "C" __global__ void bf_tex_raster_kernel(int is, int tiles, const float *frec, const int *tile_start, const int *tile_list, const float *textures, int ts,
                                                float near, float far, float bg0, float bg1, float bg2, float *pix, float *rgb, int cap);
extern "C" __global__ void bf_tex_compose_kernel(int out, int aa, const float *rgb, float *image);
extern "C" __global__ void bf_tex_depth_kernel(int out, int aa, const float *pix, float *depth);
extern "C" __global__ void bf_tex_loss_kernel(int n, const float *a, const float *b, float *grad, double *partial);
extern "C" __global__ void bf_tex_backward_kernel(int nf, int is, int out, int aa, const float *pix, const float *frec, int ts, const float *grad_image,
                                                  float *grad_tex);
extern "C" __global__ void bf_tex_backward_large_kernel(int is, int out, int aa, const float *pix, const float *frec, int ts, const float *grad_image,
                                                        float *grad_tex);
extern "C" __global__ void bf_tex_adam_kernel(size_t n, float *p, float *m, float *v, const float *g, float step_size, float bc2_sqrt, float omb1, float beta2,
                                              float omb2, float eps);
extern "C" __global__ void bf_tex_load_kernel(long long n_texels, int ts, const float *face_uv, const int *face_image, const float *face_fill,
                                              const TexImage *images, const float *lut_g, int wrapping, int bilinear, float *textures);
#pragma GCC visibility pop
