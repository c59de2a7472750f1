// What mesh_loss_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_ml_face_kernel(const int *faces, int nf, const float *verts, float *fnorm);
extern "C" __global__ void bf_ml_vertex_kernel(const int *adj_start, const int *adj, int nv, const float *fnorm, float *vnorm, float *normals);
extern "C" __global__ void bf_ml_vraw_kernel(int nv, const float *vnorm, const float *dnormals, float *dvraw);
extern "C" __global__ void bf_ml_fgrad_kernel(const int *faces, int nf, const float *P, const float *fnorm, const float *dvraw, float *dPf);
extern "C" __global__ void bf_ml_gather_kernel(const int *adj_start, const int *adj, int nv, const float *dPf, float *dverts);
extern "C" __global__ void bf_ml_lap_partial_kernel(const int *faces, int nf, const float *norms, float *partial);
extern "C" __global__ void bf_ml_lap_grad_kernel(const int *faces, const int *adj_start, const int *adj, int nf, int nv, const float *norms, float *dnorms);
extern "C" __global__ void bf_ml_pc_partial_kernel(int n, const float *P, const float *C, float *partial);
extern "C" __global__ void bf_ml_pc_grad_kernel(int n, const float *P, const float *C, const float *loss, float *dP);
extern "C" __global__ void bf_ml_normal_partial_kernel(int n, const float *fn, const float *pn, float *partial, float *dpn);
extern "C" __global__ void bf_ml_normal_gather_partial_kernel(int n, const int *ids, const float *table, int n_faces, const float *pn, float *partial, float *dpn);
extern "C" __global__ void bf_ml_scale_kernel(int n, const float *grad, const float *cotangent, int plus_zero, float *out);
extern "C" __global__ void bf_ml_finish_kernel(const float *partial, int n_partial, int root, float divisor, float *out);
#pragma GCC visibility pop
