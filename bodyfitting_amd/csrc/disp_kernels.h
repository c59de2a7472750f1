// What disp_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_disp_face_kernel(const int *faces, int nf, int nv, const float *base, const float *disp, float *fnorm);
extern "C" __global__ void bf_disp_vertex_kernel(const int *adj_start, const int *adj, int nf, int nv, const float *base, const float *disp, const float *fnorm,
                                                 float *P, float *vnorm);
extern "C" __global__ void bf_disp_vgrad_kernel(const int *faces, const int *adj_start, const int *adj, int nf, int nv, const float *vnorm,
                                                const float *const *scan_fn, const int *cface, const float *cscale, float *dvraw, const float *P, const float *C,
                                                float *pc_partial);
extern "C" __global__ void bf_disp_fgrad_kernel(const int *faces, int nf, int nv, const float *P, const float *fnorm, const float *dvraw, float *dPf);
extern "C" __global__ void bf_disp_adam_kernel(const int *adj_start, const int *adj, int nf, int nv, const float *P, const float *C, const float *pc_partial,
                                               int n_partial, const float *dPf, float *disp, float *am, float *av, float step_size, float bc2_sqrt, float beta1,
                                               float beta2, float eps);
#pragma GCC visibility pop
