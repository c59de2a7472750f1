// What overlay_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_overlay_stamp_kernel(int nv, int H, int W, const float *verts, const double *cams, uint8_t *images);
#pragma GCC visibility pop
