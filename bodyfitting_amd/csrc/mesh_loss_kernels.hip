// The SMPL+D stage's losses as stand-alone calls for gfx950 (mesh_loss_api.hip): what a user's own torch loop evaluates per
// iteration (reference smplify/smplify.py:236-245)
//   compute_normal_torch          utils/io_utils.py:406-428  and its vector-Jacobian product for ANY cotangent
//   point_cloud_loss_mesh_grid    smplify/loss.py:233-242    (one Frobenius norm; zero gradient where the norm is zero)
//   normal_loss_mesh_grid         smplify/loss.py:260-271    (the closest faces' normals already gathered)
//   normal_laplacian_smoothness   smplify/loss.py:273-288
// The arithmetic is disp_kernels.hip's (the fused stage), one mesh per call: one thread per face or vertex, incident faces walked
// BF_ADJ_BATCH at a time with the additions in list order, no atomics.  A scalar is reduced in one order that depends on the sizes
// alone: 256 values per block (lanes by xor-shuffle, the four waves as (0 + 1) + (2 + 3)), then ONE block over the block sums.
#include "bf_internal.h"
#include "mesh_loss_kernels.h"
#include "wave_ops.h"
#ifndef BF_ADJ_BATCH
#define BF_ADJ_BATCH 8        // incident faces of a vertex walked together (disp_kernels.hip)
#endif

// through n = x / (|x| + 1e-8):  dx = dn / s - n (n . dn) / |x|, and at |x| = 0 torch's rule dx = dn / 1e-8
static __device__ __forceinline__ void ml_unnormalise(const float4 n, float g0, float g1, float g2, float *o) {
    const float len = n.w, s = len + 1e-8f, dot = n.x * g0 + n.y * g1 + n.z * g2;
    const float q = len > 0.f ? dot / len : 0.f;
    o[0] = g0 / s - n.x * q; o[1] = g1 / s - n.y * q; o[2] = g2 / s - n.z * q;
}

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
    float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    float n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    float len = sqrtf(n0 * n0 + n1 * n1 + n2 * n2), s = len + 1e-8f;
    float4 o = {n0 / s, n1 / s, n2 / s, len};
    ((float4 *)fnorm)[f] = o;
}

// grid ceil(NV/256): unit vertex normal and |sum of face normals|; `normals` [nv][3] (may be NULL) is what the caller gets
extern "C" __global__ void __launch_bounds__(256)
bf_ml_vertex_kernel(const int *__restrict__ adj_start, const int *__restrict__ adj /*face*4 + corner*/, int nv,
                    const float *__restrict__ fnorm, float *__restrict__ vnorm /*[nv][4]*/, float *__restrict__ normals) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const int i0 = adj_start[v], i1 = adj_start[v + 1];
    for (int base = i0; base < i1; base += BF_ADJ_BATCH) {            // (list entries, then normals, each level's loads in flight together)
        int a[BF_ADJ_BATCH];
        float4 n[BF_ADJ_BATCH];
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) a[e] = base + e < i1 ? adj[base + e] : -1;
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) n[e] = a[e] >= 0 ? ((const float4 *)fnorm)[a[e] >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) if (a[e] >= 0) { a0 += n[e].x; a1 += n[e].y; a2 += n[e].z; }
    }
    float len = sqrtf(a0 * a0 + a1 * a1 + a2 * a2), s = len + 1e-8f;
    float4 r = {a0 / s, a1 / s, a2 / s, len};
    if (vnorm) ((float4 *)vnorm)[v] = r;
    if (normals) { normals[v * 3] = r.x; normals[v * 3 + 1] = r.y; normals[v * 3 + 2] = r.z; }
}

// VJP pass 1, grid ceil(NV/256): dL/d(vertex normal) -> dL/d(sum of face normals at v)
extern "C" __global__ void __launch_bounds__(256)
bf_ml_vraw_kernel(int nv, const float *__restrict__ vnorm, const float *__restrict__ dnormals, float *__restrict__ dvraw /*[nv][3]*/) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    ml_unnormalise(((const float4 *)vnorm)[v], dnormals[v * 3], dnormals[v * 3 + 1], dnormals[v * 3 + 2], dvraw + (size_t)v * 3);
}

// VJP pass 2, grid ceil(NF/256): per-face corner gradients dL/dP
extern "C" __global__ void __launch_bounds__(256)
bf_ml_fgrad_kernel(const int *__restrict__ faces, int nf, const float *__restrict__ P, const float *__restrict__ fnorm,
                   const float *__restrict__ dvraw, float *__restrict__ dPf /*[nf][9]*/) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int va = faces[f * 3], vb = faces[f * 3 + 1], vc = faces[f * 3 + 2];
    float d0 = dvraw[va * 3] + dvraw[vb * 3] + dvraw[vc * 3], d1 = dvraw[va * 3 + 1] + dvraw[vb * 3 + 1] + dvraw[vc * 3 + 1],
          d2 = dvraw[va * 3 + 2] + dvraw[vb * 3 + 2] + dvraw[vc * 3 + 2];
    float g[3];
    ml_unnormalise(((const float4 *)fnorm)[f], d0, d1, d2, g);                                       // dL/d(e1 x e2)
    float e1[3] = {P[vb * 3] - P[va * 3], P[vb * 3 + 1] - P[va * 3 + 1], P[vb * 3 + 2] - P[va * 3 + 2]};
    float e2[3] = {P[vc * 3] - P[va * 3], P[vc * 3 + 1] - P[va * 3 + 1], P[vc * 3 + 2] - P[va * 3 + 2]};
    float de1[3] = {e2[1] * g[2] - e2[2] * g[1], e2[2] * g[0] - e2[0] * g[2], e2[0] * g[1] - e2[1] * g[0]};   // e2 x g
    float de2[3] = {g[1] * e1[2] - g[2] * e1[1], g[2] * e1[0] - g[0] * e1[2], g[0] * e1[1] - g[1] * e1[0]};   // g x e1
    float *o = dPf + (size_t)f * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = -de1[k] - de2[k]; o[3 + k] = de1[k]; o[6 + k] = de2[k]; }
}

// VJP pass 3, grid ceil(NV/256): a vertex gathers its corners' gradients in list order
extern "C" __global__ void __launch_bounds__(256)
bf_ml_gather_kernel(const int *__restrict__ adj_start, const int *__restrict__ adj, int nv, const float *__restrict__ dPf,
                    float *__restrict__ dverts /*[nv][3]*/) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    float g[3] = {0.f, 0.f, 0.f};
    const int i0 = adj_start[v], i1 = adj_start[v + 1];
    for (int base = i0; base < i1; base += BF_ADJ_BATCH) {
        int a[BF_ADJ_BATCH];
        float q[BF_ADJ_BATCH][3];
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) a[e] = base + e < i1 ? adj[base + e] : -1;
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) {
            const float *qp = dPf + (size_t)(a[e] >= 0 ? a[e] >> 2 : 0) * 9 + (a[e] >= 0 ? a[e] & 3 : 0) * 3;
            q[e][0] = qp[0]; q[e][1] = qp[1]; q[e][2] = qp[2];
        }
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) if (a[e] >= 0) { g[0] += q[e][0]; g[1] += q[e][1]; g[2] += q[e][2]; }
    }
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
    const float m0 = norms[v * 3], m1 = norms[v * 3 + 1], m2 = norms[v * 3 + 2];
    const float k2 = 2.f / (float)nf;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    const int i0 = adj_start[v], i1 = adj_start[v + 1];
    for (int base = i0; base < i1; base += BF_ADJ_BATCH) {
        int a[BF_ADJ_BATCH], v1[BF_ADJ_BATCH], v2[BF_ADJ_BATCH];
        float o1[BF_ADJ_BATCH][3], o2[BF_ADJ_BATCH][3];
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) a[e] = base + e < i1 ? adj[base + e] : -1;
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) {
            const int f = a[e] >> 2, c = a[e] & 3;
            v1[e] = a[e] >= 0 ? faces[f * 3 + (c + 1) % 3] : 0; v2[e] = a[e] >= 0 ? faces[f * 3 + (c + 2) % 3] : 0;
        }
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) { o1[e][k] = norms[v1[e] * 3 + k]; o2[e][k] = norms[v2[e] * 3 + k]; }
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e)
            if (a[e] >= 0) { g0 += k2 * (2.f * m0 - o1[e][0] - o2[e][0]); g1 += k2 * (2.f * m1 - o1[e][1] - o2[e][1]); g2 += k2 * (2.f * m2 - o1[e][2] - o2[e][2]); }
    }
    dnorms[v * 3] = g0; dnorms[v * 3 + 1] = g1; dnorms[v * 3 + 2] = g2;
}

// point_cloud_loss_mesh_grid, grid ceil(N/256): block sums of |P - C|^2
extern "C" __global__ void __launch_bounds__(256)
bf_ml_pc_partial_kernel(int n, const float *__restrict__ P, const float *__restrict__ C, float *__restrict__ partial) {
    __shared__ float s4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float a = 0.f;
    if (i < n) {
        const float d0 = P[i * 3] - C[i * 3], d1 = P[i * 3 + 1] - C[i * 3 + 1], d2 = P[i * 3 + 2] - C[i * 3 + 2];
        a = d0 * d0 + d1 * d1 + d2 * d2;
    }
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
