// What mask_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_mask_project_kernel(MaskIO K, const float *vout, const float *proj_all, float *uvi, float *duvb, float *loss_part);
extern "C" __global__ void bf_mask_contour_kernel(MaskIO K, const float *uvi, int *choice, float *cgrad, float *loss_part);
extern "C" __global__ void bf_mask_gather_kernel(MaskIO K, const float *proj_all, const float *uvi, const float *duvb, const int *choice, const float *cgrad,
                                                 float *gpart);
extern "C" __global__ void bf_mask_gsum_kernel(MaskIO K, const float *gpart, float *dvout);
extern "C" __global__ void bf_mask_loss_kernel(MaskIO K, const float *loss_part, float *loss);
extern "C" __global__ void bf_contour_kernel(const unsigned char *masks, int H, int W, int cap, int select, float *xy, int *count, unsigned *planes_global);
#pragma GCC visibility pop
