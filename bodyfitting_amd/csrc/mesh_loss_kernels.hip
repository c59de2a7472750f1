// The SMPL+D stage's losses as stand-alone calls for gfx950 (mesh_loss_api.hip): what a user's own torch loop evaluates per
// iteration (reference smplify/smplify.py:236-245)
//   compute_normal_torch          utils/io_utils.py:406-428  and its vector-Jacobian product for ANY cotangent
//   point_cloud_loss_mesh_grid    smplify/loss.py:233-242    (one Frobenius norm; zero gradient where the norm is zero)
//   normal_loss_mesh_grid         smplify/loss.py:260-271    (the closest faces' normals already gathered)
//   normal_laplacian_smoothness   smplify/loss.py:273-288
// The arithmetic is mesh_normal_bodies.h's, shared with the fused stage (disp_kernels.hip), one mesh per call: one thread per face or vertex,
// incident faces walked BF_ADJ_BATCH at a time with the additions in list order, no atomics.  A scalar is reduced in one order that depends on the sizes
// alone: 256 values per block (lanes by xor-shuffle, the four waves as (0 + 1) + (2 + 3)), then ONE block over the block sums.
#include "bf_internal.h"
#include "mesh_loss_kernels.h"
#include "mesh_normal_bodies.h"
#include "wave_ops.h"

// grid ceil(NF/256): unit face normal and |n|
extern "C" __global__ void __launch_bounds__(256)
bf_ml_face_kernel(const int *__restrict__ faces, int nf, const float *__restrict__ verts, float *__restrict__ fnorm /*[nf][4]*/) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    float p[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = faces[f * 3 + c];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[c * 3 + k] = verts[v * 3 + k];
    }
    ((float4 *)fnorm)[f] = bf_face_normal(p);
}

// grid ceil(NV/256): unit vertex normal and |sum of face normals|; `normals` [nv][3] (may be NULL) is what the caller gets
extern "C" __global__ void __launch_bounds__(256)
bf_ml_vertex_kernel(const int *__restrict__ adj_start, const int *__restrict__ adj /*face*4 + corner*/, int nv,
                    const float *__restrict__ fnorm, float *__restrict__ vnorm /*[nv][4]*/, float *__restrict__ normals) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const float4 r = bf_vertex_normal(adj_start, adj, v, (const float4 *)fnorm);
    if (vnorm) ((float4 *)vnorm)[v] = r;
    if (normals) { normals[v * 3] = r.x; normals[v * 3 + 1] = r.y; normals[v * 3 + 2] = r.z; }
}

// VJP pass 1, grid ceil(NV/256): dL/d(vertex normal) -> dL/d(sum of face normals at v)
extern "C" __global__ void __launch_bounds__(256)
bf_ml_vraw_kernel(int nv, const float *__restrict__ vnorm, const float *__restrict__ dnormals, float *__restrict__ dvraw /*[nv][3]*/) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    bf_unnormalise(((const float4 *)vnorm)[v], dnormals[v * 3], dnormals[v * 3 + 1], dnormals[v * 3 + 2], dvraw + (size_t)v * 3);
}

// VJP pass 2, grid ceil(NF/256): per-face corner gradients dL/dP
extern "C" __global__ void __launch_bounds__(256)
bf_ml_fgrad_kernel(const int *__restrict__ faces, int nf, const float *__restrict__ P, const float *__restrict__ fnorm,
                   const float *__restrict__ dvraw, float *__restrict__ dPf /*[nf][9]*/) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    bf_face_corner_grads(faces, f, P, dvraw, ((const float4 *)fnorm)[f], dPf + (size_t)f * 9);
}

// VJP pass 3, grid ceil(NV/256): a vertex gathers its corners' gradients in list order
extern "C" __global__ void __launch_bounds__(256)
bf_ml_gather_kernel(const int *__restrict__ adj_start, const int *__restrict__ adj, int nv, const float *__restrict__ dPf,
                    float *__restrict__ dverts /*[nv][3]*/) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    float g[3] = {0.f, 0.f, 0.f};
    bf_corner_gather(adj_start, adj, v, dPf, g);
    dverts[v * 3] = g[0]; dverts[v * 3 + 1] = g[1]; dverts[v * 3 + 2] = g[2];
}

// normal_laplacian_smoothness, grid ceil(NF/256): block sums of |na-nb|^2 + |nc-na|^2 + |nb-nc|^2
extern "C" __global__ void __launch_bounds__(256)
bf_ml_lap_partial_kernel(const int *__restrict__ faces, int nf, const float *__restrict__ norms, float *__restrict__ partial) {
    __shared__ float s4[4];
    const int f = blockIdx.x * 256 + threadIdx.x;
    float t = 0.f;
    if (f < nf) {
        const float *a = norms + (size_t)faces[f * 3] * 3, *b = norms + (size_t)faces[f * 3 + 1] * 3, *c = norms + (size_t)faces[f * 3 + 2] * 3;
        float ab = 0.f, ca = 0.f, bc = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = a[k] - b[k], y = c[k] - a[k], z = b[k] - c[k];
            ab += x * x; ca += y * y; bc += z * z;
        }
        t = ab + ca + bc;
    }
    const float tot = bf_block_sum_256(bf_wave_sum(t), s4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// ... and its gradient for cotangent 1, grid ceil(NV/256): d/dn_v = 2 (2 n_v - n_o1 - n_o2) / NF per incident face, in list order
extern "C" __global__ void __launch_bounds__(256)
bf_ml_lap_grad_kernel(const int *__restrict__ faces, const int *__restrict__ adj_start, const int *__restrict__ adj, int nf, int nv,
                      const float *__restrict__ norms, float *__restrict__ dnorms) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    float g[3] = {0.f, 0.f, 0.f};
    bf_laplacian_gather(faces, adj_start, adj, v, [&](int u) { return bf_load_row3(norms + u * 3); }, bf_load_row3(norms + v * 3), 2.f / (float)nf, g);
    dnorms[v * 3] = g[0]; dnorms[v * 3 + 1] = g[1]; dnorms[v * 3 + 2] = g[2];
}

// point_cloud_loss_mesh_grid, grid ceil(N/256): block sums of |P - C|^2
extern "C" __global__ void __launch_bounds__(256)
bf_ml_pc_partial_kernel(int n, const float *__restrict__ P, const float *__restrict__ C, float *__restrict__ partial) {
    __shared__ float s4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float a = 0.f;
    if (i < n) a = bf_sqdist_row(P + i * 3, C + i * 3);
    const float tot = bf_block_sum_256(bf_wave_sum(a), s4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// ... and its gradient (P - C) / loss for cotangent 1, exactly zero where the loss is zero (torch's rule for the norm)
extern "C" __global__ void __launch_bounds__(256)
bf_ml_pc_grad_kernel(int n, const float *__restrict__ P, const float *__restrict__ C, const float *__restrict__ loss, float *__restrict__ dP) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float l = loss[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) dP[i * 3 + k] = l > 0.f ? (P[i * 3 + k] - C[i * 3 + k]) / l : 0.f;
}

// one row of normal_loss_mesh_grid, shared by the two kernels below: 1 - fn . pn_i, and -fn / N into dpn_i for cotangent 1 (dpn may be NULL)
static __device__ __forceinline__ float ml_normal_row(int i, int n, float f0, float f1, float f2, const float *__restrict__ pn,
                                                      float *__restrict__ dpn) {
    const float a = 1.f - (f0 * pn[i * 3] + f1 * pn[i * 3 + 1] + f2 * pn[i * 3 + 2]);
    if (dpn) { const float k = -1.f / (float)n; dpn[i * 3] = k * f0; dpn[i * 3 + 1] = k * f1; dpn[i * 3 + 2] = k * f2; }
    return a;
}

// normal_loss_mesh_grid, grid ceil(N/256): block sums of 1 - fn . pn, and the gradient -fn / N for cotangent 1 (dpn may be NULL)
extern "C" __global__ void __launch_bounds__(256)
bf_ml_normal_partial_kernel(int n, const float *__restrict__ fn, const float *__restrict__ pn, float *__restrict__ partial,
                            float *__restrict__ dpn) {
    __shared__ float s4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float a = 0.f;
    if (i < n) a = ml_normal_row(i, n, fn[i * 3], fn[i * 3 + 1], fn[i * 3 + 2], pn, dpn);
    const float tot = bf_block_sum_256(bf_wave_sum(a), s4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// ... with the closest faces' normals gathered here: row i takes table[ids[i]] of table[n_faces][3].  The same rows in the same block
// sums, so the bits are those of the kernel above on table[ids].  An id outside [0, n_faces) is not dereferenced: its row adds 0 to the
// sum (the mean still divides by N) and gets a zero gradient.
extern "C" __global__ void __launch_bounds__(256)
bf_ml_normal_gather_partial_kernel(int n, const int *__restrict__ ids, const float *__restrict__ table, int n_faces,
                                   const float *__restrict__ pn, float *__restrict__ partial, float *__restrict__ dpn) {
    __shared__ float s4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float a = 0.f;
    if (i < n) {
        const int f = ids[i];
        if (f >= 0 && f < n_faces) {
            const float *row = table + (size_t)f * 3;
            a = ml_normal_row(i, n, row[0], row[1], row[2], pn, dpn);
        } else if (dpn) {
            dpn[i * 3] = 0.f; dpn[i * 3 + 1] = 0.f; dpn[i * 3 + 2] = 0.f;
        }
    }
    const float tot = bf_block_sum_256(bf_wave_sum(a), s4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// the backward of a scalar loss, grid ceil(N/256): out = grad * cotangent[0] in float32, the cotangent read where it lies; plus_zero:
// + 0.0f behind the product (a statement of its own: never fused), so a zero is +0 whatever the cotangent's sign
extern "C" __global__ void __launch_bounds__(256)
bf_ml_scale_kernel(int n, const float *__restrict__ grad, const float *__restrict__ cotangent, int plus_zero, float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = grad[i] * cotangent[0];
    if (plus_zero) v = v + 0.0f;
    out[i] = v;
}

// ONE block: the block sums in a fixed order (thread t takes t, t + 256, ... ascending, then the block's tree) -> out[0] =
// sqrt(total) (root != 0) or total / divisor
extern "C" __global__ void __launch_bounds__(256)
bf_ml_finish_kernel(const float *__restrict__ partial, int n_partial, int root, float divisor, float *__restrict__ out) {
    __shared__ float s4[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += 256) a += partial[i];
    const float tot = bf_block_sum_256(bf_wave_sum(a), s4);
    if (threadIdx.x == 0) out[0] = root ? sqrtf(tot) : tot / divisor;
}
