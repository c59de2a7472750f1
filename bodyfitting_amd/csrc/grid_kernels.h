// What grid_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_grid_count_kernel(ScanDev S, int *count);
extern "C" __global__ void bf_grid_scan_kernel(int *data, int *cursor, int n);
extern "C" __global__ void bf_grid_fill_kernel(ScanDev S, int *cursor, int *tris_raw);
extern "C" __global__ void bf_grid_pack_kernel(ScanDev S, const int *tris_raw, int *tris_sorted, float4 *pack, float4 *box, int n_entries);
extern "C" __global__ void bf_face_normal_kernel(const float *verts, const int *faces, int nf, float *fn);
extern "C" __global__ void bf_inside_mesh_kernel(ScanDev S, const float *points, int n, float *sign);
extern "C" __global__ void bf_intersect_kernel(ScanDev S, const float *origins, const float *directions, int n, unsigned char *hit);
extern "C" __global__ void bf_nearest_backward_kernel(ScanDev S, int n, const int *face_ids, const float *bary, const float *dnearest, float *dpoints);
#pragma GCC visibility pop
