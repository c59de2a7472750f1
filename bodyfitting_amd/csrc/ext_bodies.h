// Device bodies shared by the two kernel files that take shape-space directions around the model's passes: expr_kernels.hip
// (up to BF_EXPR_MAX expression coefficients) and shape_ext_kernels.hip (the wide shape space).  The mathematics is written out
// at the head of expr_kernels.hip; the forward kernels of the two files add in the same order because they add HERE.
#pragma once
#include "bf_internal.h"

// The chain root to leaves over the levels of FitTab, a thread per joint of a level, then the state's update:
//   dGt_j = dGt_p + GR_p (dJ_j - dJ_p),  Gt_j += dGt_j,  At_j += dGt_j - GR_j dJ_j.
// s_dJ[nj * 3] and the root's s_dGt[0..2] = dJ_0 are in LDS and a barrier has passed; every thread of the workgroup calls it
// (one barrier per level).
__device__ __forceinline__ void bf_ext_chain_shift(const FitTab &T, const StateView &st, const float *s_dJ, float *s_dGt) {
    const int nj = T.nj, tid = threadIdx.x;
    for (int lev = 1; lev < T.n_levels; ++lev) {
        const int ls = T.level_start[lev], cnt = T.level_start[lev + 1] - ls;
        if (tid < cnt) {
            const int i = T.level_joints[ls + tid], p = T.parents[i];
            const float *G = st.GR + p * 9;
            const float r0 = s_dJ[i * 3] - s_dJ[p * 3], r1 = s_dJ[i * 3 + 1] - s_dJ[p * 3 + 1], r2 = s_dJ[i * 3 + 2] - s_dJ[p * 3 + 2];
#pragma unroll
            for (int a = 0; a < 3; ++a) s_dGt[i * 3 + a] = G[a * 3] * r0 + G[a * 3 + 1] * r1 + G[a * 3 + 2] * r2 + s_dGt[p * 3 + a];
        }
        __syncthreads();
    }
    if (tid < nj) {
        const float *G = st.GR + tid * 9;
        const float d0 = s_dJ[tid * 3], d1 = s_dJ[tid * 3 + 1], d2 = s_dJ[tid * 3 + 2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g = s_dGt[tid * 3 + a];
            st.Gt[tid * 3 + a] += g;
            st.At[tid * 3 + a] += g - (G[a * 3] * d0 + G[a * 3 + 1] * d1 + G[a * 3 + 2] * d2);
        }
    }
}

// visit(j, w) for the non-zero skinning weights of vertex v in joint order: the model's sparse rows (v_nnz 4 or 8), else its dense row
template <class F>
__device__ __forceinline__ void for_each_bone(const MeshTab &M, int v, F visit) {
    if (M.v_nnz) {
        const int nnz = M.v_nnz;
        for (int q = 0; q < nnz; ++q) {
            const float w = M.v_nzw[(size_t)v * nnz + q];
            if (w != 0.f) visit(M.v_nzj[(size_t)v * nnz + q], w);
        }
    } else {
        for (int j = 0; j < M.nj; ++j) {
            const float w = M.lbs_weights[(size_t)v * M.nj + j];
            if (w != 0.f) visit(j, w);
        }
    }
}

// one bone of the forward: a += w GR_j e (s_GR: the frame's global rotations in LDS, row-major)
__device__ __forceinline__ void bf_bone_rotate(const float *s_GR, int j, float w, float e0, float e1, float e2, float &a0, float &a1, float &a2) {
    const float *G = s_GR + j * 9;
    a0 += w * (G[0] * e0 + G[1] * e1 + G[2] * e2);
    a1 += w * (G[3] * e0 + G[4] * e1 + G[5] * e2);
    a2 += w * (G[6] * e0 + G[7] * e1 + G[8] * e2);
}
// one bone of the reverse: d += w GR_j^T g
__device__ __forceinline__ void bf_bone_rotate_t(const float *s_GR, int j, float w, float g0, float g1, float g2, float &d0, float &d1, float &d2) {
    const float *G = s_GR + j * 9;
    d0 += w * (G[0] * g0 + G[3] * g1 + G[6] * g2);
    d1 += w * (G[1] * g0 + G[4] * g1 + G[7] * g2);
    d2 += w * (G[2] * g0 + G[5] * g1 + G[8] * g2);
}
