// What model_grad_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

// bf_block_scatter_kernel's destinations: block b is columns [off, off + cnt) of every row and goes to dst[b][n][cnt] (null: not wanted)
#define BF_SCATTER_MAX 8
struct BfScatter {
    float *dst[BF_SCATTER_MAX];
    int off[BF_SCATTER_MAX], cnt[BF_SCATTER_MAX];
    int n_blocks;
};

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_block_scatter_kernel(const float *rows, int n, int stride, BfScatter S);
extern "C" __global__ void bf_model_vjp_fold_kernel(MeshTab M, const float *dvertices, const float *djoints, const float *ddirect, int n_direct, const int *lmk_vid,
                                                    const float *lmk_w, float *dv, float *dchain);
extern "C" __global__ void bf_smpl_vjp_chain_kernel(FitTab T, const float *state, const float *ext, int ext_stride, const float *dchain, float *dtheta,
                                                    float *dbeta, const float *dJx, const float *Jx, int ne, const float *dexpr_mesh, float *dexpr);
extern "C" __global__ void bf_smplx_pose_assemble_kernel(FitTab T, const float *orient, const float *body_pose, const float *jaw, const float *leye,
                                                         const float *reye, const float *lh, const float *rh, float *full, float *th_root, float *th_rest);
extern "C" __global__ void bf_smplx_dyn_row_kernel(MeshTab M, const float *state, int n, int *row);
extern "C" __global__ void bf_smplx_pose_reverse_kernel(FitTab T, const float *dtheta, const float *dfull, float *out);
#pragma GCC visibility pop
