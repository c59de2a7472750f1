// A wide SMPL-X shape space for gfx950 (bf_model_set_shape_space): betas beyond the tenth and up to 100 expression coefficients.
// smplx blends cat[betas, expression] against cat[shapedirs, exprdirs]; the device model keeps its ten core betas in registers, and
// every other direction goes around its passes exactly as expr_kernels.hip's do (the mathematics is written out there): a frame's
// extension coefficients are psi = [betas[10:], expression], L of them, against E[NV][3][L].
//
// expr_kernels.hip serves L <= BF_EXPR_MAX: one coefficient per lane of a wave, a register row per coefficient, every direction
// read again for every frame.  At L = 390 on 10,475 vertices the directions are 49 MB, so here
//   bf_shape_ext_pack_kernel     the caller's rows betas[n][NB] / expression[n][NE] -> the core block [n][10] the model's passes read
//                                and the extension block [n][L]
//   bf_shape_ext_chain_kernel    bf_expr_chain_kernel with the coefficients looped over: dJ = Jx psi with a lane per row of Jx^T
//   bf_shape_ext_vertex_kernel   a workgroup owns 256 vertices and walks the directions ONCE for a block of BF_EXT_FB frames: the block's
//                                coefficients in LDS, the per-frame sums e_v in registers - a direction element loaded serves every
//                                frame of the block; then bf_expr_vertex_kernel's update per frame
//   bf_shape_ext_reverse_kernel  d_v = sum_j w_vj GR_j^T dv_v formed once per (frame, vertex) into LDS; then lane = coefficient over the
//                                second copy of the directions E[v][k][l] (coalesced over l), each lane summing its tile's vertices in
//                                ascending order in registers, one sum per frame of the block.  No cross-lane step at all; the tiles
//                                are added in tile order by bf_ext_reduce_kernel, and bf_smpl_vjp_chain_kernel adds Jx^T dJ_rest
//   bf_shape_ext_join_kernel     dbeta[n][10] | dpsi[n][L] -> rows [n][NB + NE], which deliver_blocks cuts into the caller's blocks
// No float atomics; every sum has a fixed order (l ascending, j ascending, vertices ascending, tiles in tile order), so equal inputs
// give equal bits.  The forward kernels add in the order of expr_kernels.hip's, so at equal L they give its bits.
// LDS tables are sized by BF_SHAPE_EXT_MAX, BF_EXT_FB and BF_GRAD_MAX_JOINTS (bf_internal.h), which the host checks a model against.
#include "bf_internal.h"
#include "shape_ext_kernels.h"
#include "ext_bodies.h"

#define BF_EXT_THREADS 256
#define BF_EXT_TILE 256         // vertices per workgroup of the vertex delta and the reverse

// grid (n), 64 threads.  betas[n][nbt], expression[n][ne] (null: zeros) -> core[n][nb] = betas[.][:nb], ext[n][nbt - nb + ne]
extern "C" __global__ void __launch_bounds__(64)
bf_shape_ext_pack_kernel(const float *__restrict__ betas, const float *__restrict__ expression, int nbt, int ne, int nb,
                         float *__restrict__ core, float *__restrict__ ext) {
    const size_t f = blockIdx.x;
    const int nx = nbt - nb, L = nx + ne;
    for (int i = threadIdx.x; i < nb; i += 64) core[f * nb + i] = betas[f * nbt + i];
    for (int i = threadIdx.x; i < L; i += 64)
        ext[f * L + i] = i < nx ? betas[f * nbt + nb + i] : (expression ? expression[f * ne + (i - nx)] : 0.f);
}

// grid (n), 64 threads.  dbeta[n][nb], dpsi[n][L] -> rows[n][nb + L]
extern "C" __global__ void __launch_bounds__(64)
bf_shape_ext_join_kernel(const float *__restrict__ dbeta, const float *__restrict__ dpsi, int nb, int L, float *__restrict__ rows) {
    const size_t f = blockIdx.x;
    for (int i = threadIdx.x; i < nb + L; i += 64) rows[f * (nb + L) + i] = i < nb ? dbeta[f * nb + i] : dpsi[f * L + (i - nb)];
}

// grid (n), 256 threads, one workgroup per frame.  psi[n][L], JxT[L][NJ*3] -> dJ[n][NJ*3] (thread = row of Jx, l ascending); then the
// chain root to leaves over the levels of FitTab with a thread per joint: Gt_j += dGt_j, At_j += dGt_j - GR_j dJ_j.
extern "C" __global__ void __launch_bounds__(BF_EXT_THREADS)
bf_shape_ext_chain_kernel(FitTab T, float *__restrict__ state, const float *__restrict__ psi, int L, const float *__restrict__ JxT,
                          float *__restrict__ dJ) {
    constexpr int MJ = BF_GRAD_MAX_JOINTS;
    __shared__ float s_psi[BF_SHAPE_EXT_MAX], s_dJ[MJ * 3], s_dGt[MJ * 3];
    const int nj = T.nj, nj3 = nj * 3, tid = threadIdx.x, f = blockIdx.x;
    StateView st = bf_state_view(state + (size_t)f * bf_state_stride(nj, T.npf, T.nb), nj, T.npf, T.nb);
    for (int l = tid; l < L; l += BF_EXT_THREADS) s_psi[l] = psi[(size_t)f * L + l];
    __syncthreads();
    if (tid < nj3) {
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc += JxT[(size_t)l * nj3 + tid] * s_psi[l];
        s_dJ[tid] = acc;
        dJ[(size_t)f * nj3 + tid] = acc;
        if (tid < 3) s_dGt[tid] = acc;
    }
    __syncthreads();
    bf_ext_chain_shift(T, st, s_dJ, s_dGt);
}

namespace {
// frame f's global rotations into LDS (every thread of the workgroup calls it; it synchronises on both sides, so the table may be reused)
__device__ __forceinline__ void stage_rotations(const MeshTab &M, const float *__restrict__ state, int f, float *s_GR) {
    const float *GR = state + (size_t)f * bf_state_stride(M.nj, M.npf, M.nb);           // (StateView::GR: the state row's head)
    __syncthreads();
    for (int i = threadIdx.x; i < M.nj * 9; i += BF_EXT_THREADS) s_GR[i] = GR[i];
    __syncthreads();
}
}  // namespace

// grid (ceil(NV / 256), ceil(n / BF_EXT_FB)), 256 threads, thread = vertex.  For the block's frames f0 .. f0 + BF_EXT_FB (those below n):
// e_v[f] = E_v psi_f (l ascending, every E element loaded once for the block); then per frame
// vraw[f][v] += sum_j w_vj GR_j e_v (j ascending), vposed[f][v] += e_v (vposed may be null: a forward that saves nothing).
extern "C" __global__ void __launch_bounds__(BF_EXT_THREADS)
bf_shape_ext_vertex_kernel(MeshTab M, const float *__restrict__ state, const float *__restrict__ psi, int L, int n,
                           const float *__restrict__ exprT, float *__restrict__ vraw, float *__restrict__ vposed) {
    constexpr int FB = BF_EXT_FB;
    __shared__ __attribute__((aligned(16))) float s_psi[BF_SHAPE_EXT_MAX * FB];       // [l][frame of the block]; zeros past the last frame
    __shared__ float s_GR[BF_GRAD_MAX_JOINTS * 9];
    const int nv = M.nv, tid = threadIdx.x, f0 = blockIdx.y * FB, nf = min(FB, n - f0);
    for (int i = tid; i < L * FB; i += BF_EXT_THREADS) {
        const int l = i / FB, b = i - l * FB;
        s_psi[i] = b < nf ? psi[(size_t)(f0 + b) * L + l] : 0.f;
    }
    __syncthreads();
    const int v = blockIdx.x * BF_EXT_TILE + tid;
    const bool live = v < nv;
    float e0[FB], e1[FB], e2[FB];
#pragma unroll
    for (int b = 0; b < FB; ++b) e0[b] = e1[b] = e2[b] = 0.f;
    if (live) {
        const float *E = exprT + v;
        for (int l = 0; l < L; ++l, E += (size_t)3 * nv) {
            const float x0 = E[0], x1 = E[nv], x2 = E[2 * (size_t)nv];
            const float4 *c4 = reinterpret_cast<const float4 *>(s_psi + l * FB);
#pragma unroll
            for (int q = 0; q < FB / 4; ++q) {
                const float4 c = c4[q];
                e0[q * 4] += x0 * c.x; e1[q * 4] += x1 * c.x; e2[q * 4] += x2 * c.x;
                e0[q * 4 + 1] += x0 * c.y; e1[q * 4 + 1] += x1 * c.y; e2[q * 4 + 1] += x2 * c.y;
                e0[q * 4 + 2] += x0 * c.z; e1[q * 4 + 2] += x1 * c.z; e2[q * 4 + 2] += x2 * c.z;
                e0[q * 4 + 3] += x0 * c.w; e1[q * 4 + 3] += x1 * c.w; e2[q * 4 + 3] += x2 * c.w;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < FB; ++b) {
        if (b >= nf) break;                                         // (workgroup-uniform)
        stage_rotations(M, state, f0 + b, s_GR);
        if (!live) continue;
        const float x0 = e0[b], x1 = e1[b], x2 = e2[b];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for_each_bone(M, v, [&](int j, float w) { bf_bone_rotate(s_GR, j, w, x0, x1, x2, a0, a1, a2); });
        const size_t o = ((size_t)(f0 + b) * nv + v) * 3;
        vraw[o] += a0; vraw[o + 1] += a1; vraw[o + 2] += a2;
        if (vposed) { vposed[o] += x0; vposed[o + 1] += x1; vposed[o + 2] += x2; }
    }
}

// grid (ceil(NV / 256), ceil(n / BF_EXT_FB)), 256 threads.
//   1. thread = vertex of the tile: d_v[f] = sum_j w_vj GR_j^T dv[f][v] (j ascending) for the block's frames -> LDS, formed once
//   2. thread = coefficient l (l += 256 while l < L): part[f][tile][l] = sum over the tile's vertices ascending of E[v][.][l] . d_v[f],
//      E read in [v][k][l] order (the lanes of a wave read consecutive l), d_v broadcast from LDS, one register sum per frame
extern "C" __global__ void __launch_bounds__(BF_EXT_THREADS)
bf_shape_ext_reverse_kernel(MeshTab M, const float *__restrict__ state, const float *__restrict__ dv, int L, int n,
                            const float *__restrict__ extVK, float *__restrict__ part) {
    constexpr int FB = BF_EXT_FB;
    __shared__ float s_GR[BF_GRAD_MAX_JOINTS * 9];
    __shared__ float4 s_d[BF_EXT_TILE * FB];                        // [vertex of the tile][frame of the block] (d0, d1, d2, -)
    const int nv = M.nv, tid = threadIdx.x, tile = blockIdx.x, f0 = blockIdx.y * FB, nf = min(FB, n - f0);
    const int v0 = tile * BF_EXT_TILE, nvt = min(BF_EXT_TILE, nv - v0), v = v0 + tid;
    for (int b = 0; b < FB; ++b) {
        if (b >= nf) {                                              // (workgroup-uniform) a frame past the last: zeros, never stored
            s_d[tid * FB + b] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        stage_rotations(M, state, f0 + b, s_GR);
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (v < nv) {
            const size_t o = ((size_t)(f0 + b) * nv + v) * 3;
            const float g0 = dv[o], g1 = dv[o + 1], g2 = dv[o + 2];
            for_each_bone(M, v, [&](int j, float w) { bf_bone_rotate_t(s_GR, j, w, g0, g1, g2, d0, d1, d2); });
        }
        s_d[tid * FB + b] = make_float4(d0, d1, d2, 0.f);
    }
    __syncthreads();
    for (int l = tid; l < L; l += BF_EXT_THREADS) {
        float acc[FB];
#pragma unroll
        for (int b = 0; b < FB; ++b) acc[b] = 0.f;
        const float *E = extVK + (size_t)v0 * 3 * L + l;
        for (int t = 0; t < nvt; ++t, E += (size_t)3 * L) {
            const float x0 = E[0], x1 = E[L], x2 = E[2 * (size_t)L];
#pragma unroll
            for (int b = 0; b < FB; ++b) {
                const float4 d = s_d[t * FB + b];
                acc[b] += x0 * d.x + x1 * d.y + x2 * d.z;
            }
        }
#pragma unroll
        for (int b = 0; b < FB; ++b)
            if (b < nf) part[((size_t)(f0 + b) * gridDim.x + tile) * L + l] = acc[b];
    }
}
