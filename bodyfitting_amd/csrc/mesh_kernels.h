// What mesh_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_pose_state_kernel(FitTab T, const float *betas, const float *orient, const float *body_pose, const float *sim, float *state,
                                                const float *packed, const float *cscale, float cscale_all);
extern "C" __global__ void bf_mesh_kernel(MeshTab M, const float *state, float *vraw, float *vout, float *xpart, float *vposed, const float *pose_off, int *door,
                                          int door_target, float *vmirror);
extern "C" __global__ void bf_mesh_span_kernel(MeshTab M, const float *state, float *vraw, float *vout, float *xpart, unsigned long long *span);
extern "C" int bf_mesh_multi_launch(const MeshTab *M, const float *state, int n, float *vraw, float *vout, float *xpart, float *vposed, float *dvzero,
                                    hipStream_t stream, const MaskProj *mproj, int *door, int door_target, hipEvent_t done, float *vmirror);
extern "C" int bf_mesh_use_multi(int npf, int n);
extern "C" size_t bf_mesh_smem_bytes(int nj, int npf, int nb);
extern "C" __global__ void bf_joints_kernel(MeshTab M, const float *state, const float *vraw, const float *xpart, float *joints, float *joints_ori, float *jraw,
                                            int *lmk_vid, float *lmk_w, BfHandOver ho);
extern "C" __global__ void bf_pack_feat_kernel(MeshTab M, const float *state, int n_frames, int kpad, int fpad, float *featT);
extern "C" __global__ void bf_poseblend_gemm_kernel(MeshTab M, const float *featT, int kpad, int fpad, int n_frames, float *pose_off);
extern "C" hipError_t bf_poseblend_launch(const MeshTab *M, const float *state, int n, float *featT, int kpad, int fpad, float *pose_off, hipStream_t stream);
extern "C" void bf_mesh_epilogue_batch_launch(const MeshTab *M, const float *state, const float *pose_off, int n, float *vraw, float *vout, float *xpart,
                                              hipStream_t stream);
extern "C" bool bf_mesh_batch32_fits(const MeshTab *M);
extern "C" hipError_t bf_mesh_batch32_launch(const MeshTab *M, const float *state, int n, float *vraw, float *vout, float *xpart, hipStream_t stream);
extern "C" __global__ void bf_mesh_epilogue_kernel(MeshTab M, const float *state, const float *pose_off, float *vraw, float *vout, float *xpart, float *vposed);
extern "C" __global__ void bf_transpose_kernel(const float *in, int rows, int cols, float *out, int in_pitch);
#pragma GCC visibility pop
