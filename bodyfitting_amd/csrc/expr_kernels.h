// What expr_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_expr_chain_kernel(FitTab T, float *state, const float *expr, int ne, const float *Jx, float *dJ);
extern "C" __global__ void bf_expr_vertex_kernel(MeshTab M, const float *state, const float *expr, int ne, const float *exprT, float *vraw, float *vposed);
extern "C" __global__ void bf_expr_xpart_kernel(MeshTab M, const float *vraw, float *xpart);
extern "C" __global__ void bf_expr_reverse_kernel(MeshTab M, const float *state, const float *dv, int ne, const float *exprT, float *part);
#pragma GCC visibility pop
