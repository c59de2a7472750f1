// SMPL+D stage for gfx950: Adam on a per-vertex displacement of the fitted mesh towards the scan
// (reference smplify/smplify.py:228-247): loss = icp + (normal_loss + laplacian) * constant_scale * 0.1 with
//   compute_normal_torch          utils/io_utils.py:406-428  (face normals / (|n|+1e-8), summed per vertex
//                                 corner by corner, normalised again)
//   point_cloud_loss_mesh_grid    smplify/loss.py:233-242    (one Frobenius norm)
//   normal_loss_mesh_grid         smplify/loss.py:260-271    (un-normalised scan face normals, smplify.py:149)
//   normal_laplacian_smoothness   smplify/loss.py:273-288
// and their hand-derived reverse.  All sums are gathers over a vertex -> (corner, face) CSR list in
// the order the reference's sparse products add them, so the stage is deterministic.
// Kernels per iteration: faces -> vertices(+P) -> [nearest, pc_partial from scan_kernels.hip] ->
// vertex gradient -> face gradient -> vertex gather + Adam.
// The arithmetic of the normals, their reverse and the walks is mesh_normal_bodies.h's, shared with the stand-alone losses
// (mesh_loss_kernels.hip); here: the frame dimension, P = base + disp, the fused block sum of |P - C|^2 and the fused Adam step.
#include "bf_internal.h"
#include "disp_kernels.h"
#include "mesh_normal_bodies.h"
#include "wave_ops.h"

// grid (ceil(NF/256), F)
extern "C" __global__ void __launch_bounds__(256)
bf_disp_face_kernel(const int *__restrict__ faces, int nf, int nv, const float *__restrict__ base,
                    const float *__restrict__ disp, float *__restrict__ fnorm /*[F][nf][4]: unit normal, |n|*/) {
    const int f = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (f >= nf) return;
    const float *b = base + (size_t)fr * nv * 3, *d = disp + (size_t)fr * nv * 3;
    float p[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v = faces[f * 3 + c];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[c * 3 + k] = b[v * 3 + k] + d[v * 3 + k];
    }
    ((float4 *)fnorm)[(size_t)fr * nf + f] = bf_face_normal(p);
}

// grid (ceil(NV/256), F): deformed vertex P, vertex normal (unit) and |sum of face normals|
extern "C" __global__ void __launch_bounds__(256)
bf_disp_vertex_kernel(const int *__restrict__ adj_start, const int *__restrict__ adj /*face*4 + corner*/, int nf, int nv,
                      const float *__restrict__ base, const float *__restrict__ disp, const float *__restrict__ fnorm,
                      float *__restrict__ P, float *__restrict__ vnorm /*[F][nv][4]*/) {
    const int v = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (v >= nv) return;
    const size_t o = ((size_t)fr * nv + v) * 3;
    P[o] = base[o] + disp[o]; P[o + 1] = base[o + 1] + disp[o + 1]; P[o + 2] = base[o + 2] + disp[o + 2];
    ((float4 *)vnorm)[(size_t)fr * nv + v] = bf_vertex_normal(adj_start, adj, v, (const float4 *)fnorm + (size_t)fr * nf);
}

// grid (ceil(NV/256), F): dL/d(sum of face normals at v) from the normal and laplacian terms
extern "C" __global__ void __launch_bounds__(256)
bf_disp_vgrad_kernel(const int *__restrict__ faces, const int *__restrict__ adj_start, const int *__restrict__ adj, int nf, int nv,
                     const float *__restrict__ vnorm, const float *const *__restrict__ scan_fn, const int *__restrict__ cface, const float *__restrict__ cscale,
                     float *__restrict__ dvraw /*[F][nv][3]*/, const float *__restrict__ P, const float *__restrict__ C,
                     float *__restrict__ pc_partial) {
    const int v = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (pc_partial) {
        // this block's share of |P - C|^2 while it is here (bf_pc_partial_kernel's sums in its order: one launch less per iteration)
        __shared__ float s_pc[4];
        float a = 0.f;
        if (v < nv) a = bf_sqdist_row(P + ((size_t)fr * nv + v) * 3, C + ((size_t)fr * nv + v) * 3);
        const float tot = bf_block_sum_256(bf_wave_sum(a), s_pc);
        if (threadIdx.x == 0) pc_partial[(size_t)fr * gridDim.x + blockIdx.x] = tot;
    }
    if (v >= nv) return;
    const float w = cscale[fr] * 0.1f;                                  // smplify.py:242
    const float4 *vn = (const float4 *)vnorm + (size_t)fr * nv;
    const float4 me = vn[v];
    // normal loss: mean_v (1 - fn_scan[closest face] . n_v)
    float g[3] = {0.f, 0.f, 0.f};
    int cf = cface[(size_t)fr * nv + v];
    if (cf >= 0) {
        const float *fn = scan_fn[fr] + (size_t)cf * 3;
        float k = -w / (float)nv;
        g[0] = k * fn[0]; g[1] = k * fn[1]; g[2] = k * fn[2];
    }
    // laplacian: mean_f (|na-nb|^2 + |nc-na|^2 + |nb-nc|^2)  ->  d/dn_v = 2 (2 n_v - n_o1 - n_o2) / NF per incident face
    bf_laplacian_gather(faces, adj_start, adj, v, [&](int u) { return vn[u]; }, me, 2.f * w / (float)nf, g);
    bf_unnormalise(me, g[0], g[1], g[2], dvraw + ((size_t)fr * nv + v) * 3);
}

// grid (ceil(NF/256), F): per-face corner gradients dL/dP from the normal terms
extern "C" __global__ void __launch_bounds__(256)
bf_disp_fgrad_kernel(const int *__restrict__ faces, int nf, int nv, const float *__restrict__ P,
                     const float *__restrict__ fnorm, const float *__restrict__ dvraw, float *__restrict__ dPf /*[F][nf][9]*/) {
    const int f = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (f >= nf) return;
    bf_face_corner_grads(faces, f, P + (size_t)fr * nv * 3, dvraw + (size_t)fr * nv * 3, ((const float4 *)fnorm)[(size_t)fr * nf + f],
                         dPf + ((size_t)fr * nf + f) * 9);
}

// grid (ceil(NV/256), F): total gradient of vertex v, then torch-semantics Adam on its 3 displacement scalars
extern "C" __global__ void __launch_bounds__(256)
bf_disp_adam_kernel(const int *__restrict__ adj_start, const int *__restrict__ adj, int nf, int nv, const float *__restrict__ P,
                    const float *__restrict__ C, const float *__restrict__ pc_partial, int n_partial,
                    const float *__restrict__ dPf, float *__restrict__ disp, float *__restrict__ am, float *__restrict__ av,
                    float step_size, float bc2_sqrt, float beta1, float beta2, float eps) {
    const int v = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (v >= nv) return;
    float tot = 0.f;
    for (int b = 0; b < n_partial; ++b) tot += pc_partial[(size_t)fr * n_partial + b];     // fixed order
    const float inorm = tot > 0.f ? 1.0f / sqrtf(tot) : 0.f;                              // (torch's rule for the norm at zero: a zero gradient)
    const size_t o = ((size_t)fr * nv + v) * 3;
    float g[3] = {(P[o] - C[o]) * inorm, (P[o + 1] - C[o + 1]) * inorm, (P[o + 2] - C[o + 2]) * inorm};
    bf_corner_gather(adj_start, adj, v, dPf + (size_t)fr * nf * 9, g);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float m = am[o + k], vv = av[o + k];
        m = m + (g[k] - m) * (1.0f - beta1);
        vv = vv * beta2 + (1.0f - beta2) * g[k] * g[k];
        am[o + k] = m; av[o + k] = vv;
        disp[o + k] = disp[o + k] - step_size * (m / (sqrtf(vv) / bc2_sqrt + eps));
    }
}
