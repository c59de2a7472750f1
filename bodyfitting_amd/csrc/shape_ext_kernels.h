// What shape_ext_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_shape_ext_pack_kernel(const float *betas, const float *expression, int nbt, int ne, int nb, float *core, float *ext);
extern "C" __global__ void bf_shape_ext_join_kernel(const float *dbeta, const float *dpsi, int nb, int L, float *rows);
extern "C" __global__ void bf_shape_ext_chain_kernel(FitTab T, float *state, const float *psi, int L, const float *JxT, float *dJ);
extern "C" __global__ void bf_shape_ext_vertex_kernel(MeshTab M, const float *state, const float *psi, int L, int n, const float *exprT, float *vraw, float *vposed);
extern "C" __global__ void bf_shape_ext_reverse_kernel(MeshTab M, const float *state, const float *dv, int L, int n, const float *extVK, float *part);
#pragma GCC visibility pop
