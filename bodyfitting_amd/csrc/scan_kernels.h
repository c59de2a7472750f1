// What scan_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_nearest_kernel(const ScanDev *scans, const float *points, int n, int *face, float *pts, float *bary, int warm, int n_frames);
extern "C" __global__ void bf_nearest_fast_kernel(const ScanDev *scans, const float *points, int n, int *face, float *pts, float *bary, int warm, int n_frames);
extern "C" __global__ void bf_nearest_quot_kernel(int n, const float *num, const float *den, float *out);
extern "C" __global__ void bf_nearest_rule_kernel(int n, const float *patches, float *dist, float *coeff, int general);
extern "C" void bf_nearest_launch(dim3 grid, hipStream_t stream, const ScanDev *scans, const float *points, int n, int *face, float *pts, float *bary, int warm);
extern "C" __global__ void bf_pc_partial_kernel(const float *P, const float *C, int n, float *partial);
extern "C" __global__ void bf_pc_grad_kernel(const float *P, const float *C, int n, const float *partial, const float *weight, float *dvout, float *loss,
                                             int accumulate, int *door, int door_target);
extern "C" __global__ void bf_dv_add_kernel(float *dvout, const float *extra, const int *verts, int n, int nv_full);
extern "C" int bf_mesh_bwd_multi_launch(const MeshTab *M, const float *posedirsT, const float *state, int n, const float *dvout, const float *vposed,
                                        const float *vraw, float *part, hipStream_t stream, const float *gpart, int n_masks, int n_sampled, int samp_stride,
                                        int part_rows, int *rows_out, const MaskFold *fold);
extern "C" __global__ void bf_door_probe_kernel(int *door);
extern "C" __global__ void bf_door_ring_kernel(int *door);
extern "C" __global__ void bf_ext_reduce_kernel(const float *part, int n_tiles, int EXT, float *ext, int ext_stride, int *door, int door_k);
extern "C" __global__ void bf_kp_loss_kernel(KpIO Q, const float *jraw, const float *state, const float *proj_all, const float *keypoints, const int *ndiv,
                                             const int *lmk_vid, const float *lmk_w, float *ext, float *dvout, float *terms, MeshTab M, const float *vraw,
                                             const float *xpart, int *door);
extern "C" __global__ void bf_kp_contour_kernel(KpIO Q, const float *jraw, const float *state, const float *proj_all, const float *keypoints, const int *ndiv,
                                                const int *lmk_vid, const float *lmk_w, float *ext, float *dvout, float *terms, MaskIO K, const float *uvi,
                                                int *choice, float *cgrad, float *loss_part, MeshTab M, const float *vraw, const float *xpart);
#pragma GCC visibility pop
