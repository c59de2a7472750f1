// SMPL-X expression coefficients for gfx950: the kernels bf_smplx_forward_expr / bf_smplx_vjp_expr (model_grad_api.hip) add around
// the pose-state kernel, the mesh passes and the chain reverse, none of which knows the expression directions (the device model
// keeps its shape coefficients in twelve registers; the expression term is affine for fixed rotations and goes around them).
// smplx lbs(): v_shaped = v_template + S beta + E psi, J = Jt + Jd beta + Jx psi (Jx = J_regressor E); pose blend shapes do not
// depend on psi.  With e_v = E_v psi, dJ = Jx psi and GR the pose state's global rotations:
//   dGt_root = dJ_0,  dGt_j = dGt_p + GR_p (dJ_j - dJ_p),  dAt_j = dGt_j - GR_j dJ_j
//   vertex_v += sum_j w_vj (GR_j e_v + dAt_j),  posed chain joint j += dGt_j
//
//   bf_expr_chain_kernel    psi -> dJ (kept for the chain reverse); the state's Gt / At shifted in place - BEFORE the mesh pass,
//                           whose skinning reads At and so carries the sum_j w_vj dAt_j term itself
//   bf_expr_vertex_kernel   behind the mesh pass, in front of the joints pass: vraw += sum_j w_vj GR_j e_v; the saved pose-blended
//                           vertices += e_v, which is what the mesh reverse's sum w dv (x) vp rows have to see
//   bf_expr_xpart_kernel    (a model with J_regressor_extra rows) the extra joints' per-tile sums again, from the updated vertices
//   bf_expr_reverse_kernel  E_v^T (sum_j w_vj GR_j^T dv_v) per vertex, summed per 256-vertex tile in a fixed order; the tiles are
//                           added in tile order by bf_ext_reduce_kernel, and bf_smpl_vjp_chain_kernel adds Jx^T dJ_rest
// No float atomics: every sum has a fixed order, so equal inputs give equal bits.
// E arrives transposed, exprT[l][k][v]: a wave's loads of one coefficient's component are contiguous over its vertices.
// The LDS tables are sized by BF_EXPR_MAX and BF_GRAD_MAX_JOINTS (bf_internal.h), which the host checks a model against.
#include "bf_internal.h"
#include "expr_kernels.h"
#include "ext_bodies.h"

#define BF_EXPR_THREADS 256

// grid (n), one wave per frame; lane = joint, the chain walked root to leaves over the levels of FitTab.
// expr[n][ne], Jx[NJ*3][ne] -> dJ[n][NJ*3]; state: Gt_j += dGt_j, At_j += dGt_j - GR_j dJ_j.
extern "C" __global__ void __launch_bounds__(64)
bf_expr_chain_kernel(FitTab T, float *__restrict__ state, const float *__restrict__ expr, int ne, const float *__restrict__ Jx,
                     float *__restrict__ dJ) {
    constexpr int MJ = BF_GRAD_MAX_JOINTS;
    __shared__ float s_psi[BF_EXPR_MAX], s_dJ[MJ * 3], s_dGt[MJ * 3];
    const int nj = T.nj, tid = threadIdx.x, f = blockIdx.x;
    StateView st = bf_state_view(state + (size_t)f * bf_state_stride(nj, T.npf, T.nb), nj, T.npf, T.nb);
    if (tid < ne) s_psi[tid] = expr[(size_t)f * ne + tid];
    __syncthreads();
    if (tid < nj) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float acc = 0.f;
            for (int l = 0; l < ne; ++l) acc += Jx[(tid * 3 + k) * ne + l] * s_psi[l];
            s_dJ[tid * 3 + k] = acc;
            dJ[((size_t)f * nj + tid) * 3 + k] = acc;
            if (tid == 0) s_dGt[k] = acc;
        }
    }
    __syncthreads();
    bf_ext_chain_shift(T, st, s_dJ, s_dGt);
}

namespace {
// the frame's coefficients and global rotations into LDS (every thread of the workgroup calls it; it synchronises)
__device__ __forceinline__ void stage_frame(const MeshTab &M, const float *__restrict__ state, const float *__restrict__ expr, int ne, int f,
                                            float *s_psi, float *s_GR) {
    const float *GR = state + (size_t)f * bf_state_stride(M.nj, M.npf, M.nb);          // (StateView::GR: the state row's head)
    if (expr && threadIdx.x < ne) s_psi[threadIdx.x] = expr[(size_t)f * ne + threadIdx.x];
    for (int i = threadIdx.x; i < M.nj * 9; i += BF_EXPR_THREADS) s_GR[i] = GR[i];
    __syncthreads();
}
}  // namespace

// grid (ceil(NV / 256), n), 256 threads, thread = vertex.  e_v = E_v psi (l ascending);
// vraw[f][v] += sum_j w_vj GR_j e_v (j ascending), vposed[f][v] += e_v (vposed may be null: a forward that saves nothing).
extern "C" __global__ void __launch_bounds__(BF_EXPR_THREADS)
bf_expr_vertex_kernel(MeshTab M, const float *__restrict__ state, const float *__restrict__ expr, int ne, const float *__restrict__ exprT,
                      float *__restrict__ vraw, float *__restrict__ vposed) {
    __shared__ float s_psi[BF_EXPR_MAX], s_GR[BF_GRAD_MAX_JOINTS * 9];
    const int f = blockIdx.y, nv = M.nv;
    stage_frame(M, state, expr, ne, f, s_psi, s_GR);
    const int v = blockIdx.x * BF_EXPR_THREADS + threadIdx.x;
    if (v >= nv) return;
    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
    for (int l = 0; l < ne; ++l) {
        const float *E = exprT + (size_t)l * 3 * nv + v;
        const float c = s_psi[l];
        e0 += E[0] * c; e1 += E[nv] * c; e2 += E[2 * (size_t)nv] * c;
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for_each_bone(M, v, [&](int j, float w) { bf_bone_rotate(s_GR, j, w, e0, e1, e2, a0, a1, a2); });
    const size_t o = ((size_t)f * nv + v) * 3;
    vraw[o] += a0; vraw[o + 1] += a1; vraw[o + 2] += a2;
    if (vposed) { vposed[o] += e0; vposed[o + 1] += e1; vposed[o + 2] += e2; }
}

// grid (MeshTab::n_tiles, n), 128 threads; only for a model with J_regressor_extra rows.  The mesh pass forms the extra-regressor
// joints' per-tile partial sums from the vertices it writes - in front of the vertex delta - so they are formed again from the
// updated ones: xpart[f][tile][e][k] = sum over the tile's vertices ascending of j_extra[e][v] vraw[f][v][k], the layout
// bf_joints_kernel adds up in tile order.
extern "C" __global__ void __launch_bounds__(128)
bf_expr_xpart_kernel(MeshTab M, const float *__restrict__ vraw, float *__restrict__ xpart) {
    const int tile = blockIdx.x, f = blockIdx.y, nv = M.nv, ne3 = M.n_extra * 3, v0 = tile * BF_MESH_TILE, nvt = min(BF_MESH_TILE, nv - v0);
    for (int o = threadIdx.x; o < ne3; o += 128) {
        const int e = o / 3, k = o - e * 3;
        float acc = 0.f;
        for (int t = 0; t < nvt; ++t) acc += M.j_extra[(size_t)e * nv + v0 + t] * vraw[((size_t)f * nv + v0 + t) * 3 + k];
        xpart[((size_t)f * gridDim.x + tile) * ne3 + o] = acc;
    }
}

// grid (ceil(NV / 256), n), 256 threads, thread = vertex.  d_v = sum_j w_vj GR_j^T dv_v (j ascending), c_l = E_v[.][l] . d_v;
// part[f][tile][l] = the workgroup's sum of c_l: inside a wave the xor tree 1, 2, .. 32, then the four waves in wave order.
// A thread past the last vertex adds zeros (it stays for the shuffles).
extern "C" __global__ void __launch_bounds__(BF_EXPR_THREADS)
bf_expr_reverse_kernel(MeshTab M, const float *__restrict__ state, const float *__restrict__ dv, int ne, const float *__restrict__ exprT,
                       float *__restrict__ part) {
    __shared__ float s_GR[BF_GRAD_MAX_JOINTS * 9], s_red[BF_EXPR_THREADS / 64][BF_EXPR_MAX];
    const int f = blockIdx.y, nv = M.nv, tid = threadIdx.x;
    stage_frame(M, state, nullptr, 0, f, nullptr, s_GR);
    const int v = blockIdx.x * BF_EXPR_THREADS + tid;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (v < nv) {
        const size_t o = ((size_t)f * nv + v) * 3;
        const float g0 = dv[o], g1 = dv[o + 1], g2 = dv[o + 2];
        for_each_bone(M, v, [&](int j, float w) { bf_bone_rotate_t(s_GR, j, w, g0, g1, g2, d0, d1, d2); });
    }
#pragma unroll
    for (int l = 0; l < BF_EXPR_MAX; ++l) {
        if (l < ne) {                                              // (workgroup-uniform)
            float c = 0.f;
            if (v < nv) {
                const float *E = exprT + (size_t)l * 3 * nv + v;
                c = E[0] * d0 + E[nv] * d1 + E[2 * (size_t)nv] * d2;
            }
            c += __shfl_xor(c, 1); c += __shfl_xor(c, 2); c += __shfl_xor(c, 4); c += __shfl_xor(c, 8); c += __shfl_xor(c, 16);
            c += __shfl_xor(c, 32);
            if ((tid & 63) == 0) s_red[tid >> 6][l] = c;
        }
    }
    __syncthreads();
    if (tid < ne) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < BF_EXPR_THREADS / 64; ++w) tot += s_red[w][tid];
        part[((size_t)f * gridDim.x + blockIdx.x) * ne + tid] = tot;
    }
}
