// What silhouette_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_sil_project_kernel(MaskIO K, const float *verts, const float *proj, float *uvi, float *duvb, float *loss_part);
extern "C" __global__ void bf_sil_contour_kernel(MaskIO K, const float *uvi, float *loss_part);
extern "C" __global__ void bf_sil_finish_kernel(MaskIO K, const float *proj, const float *uvi, const float *duvb, const float *loss_part, float *terms,
                                                float *dverts);
extern "C" __global__ void bf_sil_ingest_kernel(const void *masks, int is_float, unsigned long long npix, unsigned plane, unsigned *bin, int *flags,
                                                int n_views);
extern "C" __global__ void bf_sil_rows_kernel(const float *K, const float *w2c, int n_views, float *rows);
#pragma GCC visibility pop
