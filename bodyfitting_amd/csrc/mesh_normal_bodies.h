// The float32 arithmetic of compute_normal_torch (utils/io_utils.py:406-428), of normal_laplacian_smoothness and point_cloud_loss_mesh_grid
// (smplify/loss.py:273-288, 233-242) and of their reverse, stated once for the fused SMPL+D stage (disp_kernels.hip: a frame dimension, a
// fused block sum, a fused Adam step around these bodies) and the stand-alone losses (mesh_loss_kernels.hip: one mesh per call).  A body
// takes pointers to ITS mesh: the stage adds its frame's offset before the call.  Compiled under the flags of the including file.
#pragma once
#include <hip/hip_runtime.h>
#ifndef BF_ADJ_BATCH
#define BF_ADJ_BATCH 8        // incident faces of a vertex walked together (a closed triangle mesh averages six)
#endif

// x / (|x| + 1e-8), and |x| in .w
__device__ __forceinline__ float4 bf_unit_normal(float n0, float n1, float n2) {
    float len = sqrtf(n0 * n0 + n1 * n1 + n2 * n2), s = len + 1e-8f;
    float4 o = {n0 / s, n1 / s, n2 / s, len};
    return o;
}

// the unit normal of the face with corners p[0..2], p[3..5], p[6..8]: e1 x e2
__device__ __forceinline__ float4 bf_face_normal(const float *p) {
    float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    float n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    return bf_unit_normal(n0, n1, n2);
}

// through n = x / (|x| + 1e-8):  dx = dn / s - n (n . dn) / |x|, and at |x| = 0 torch's rule dx = dn / 1e-8
__device__ __forceinline__ void bf_unnormalise(const float4 n, float g0, float g1, float g2, float *o) {
    const float len = n.w, s = len + 1e-8f, dot = n.x * g0 + n.y * g1 + n.z * g2;
    const float q = len > 0.f ? dot / len : 0.f;
    o[0] = g0 / s - n.x * q; o[1] = g1 / s - n.y * q; o[2] = g2 / s - n.z * q;
}

// the corner gradients o[9] = dL/d(its three corners) of face f with unit normal fn: its corners' dvraw rows summed, back through the
// normalisation to g = dL/d(e1 x e2), then through the cross product
__device__ __forceinline__ void bf_face_corner_grads(const int *faces, int f, const float *P, const float *dvraw, const float4 fn, float *o) {
    const int va = faces[f * 3], vb = faces[f * 3 + 1], vc = faces[f * 3 + 2];
    float d0 = dvraw[va * 3] + dvraw[vb * 3] + dvraw[vc * 3], d1 = dvraw[va * 3 + 1] + dvraw[vb * 3 + 1] + dvraw[vc * 3 + 1],
          d2 = dvraw[va * 3 + 2] + dvraw[vb * 3 + 2] + dvraw[vc * 3 + 2];
    float g[3];
    bf_unnormalise(fn, d0, d1, d2, g);
    float e1[3] = {P[vb * 3] - P[va * 3], P[vb * 3 + 1] - P[va * 3 + 1], P[vb * 3 + 2] - P[va * 3 + 2]};
    float e2[3] = {P[vc * 3] - P[va * 3], P[vc * 3 + 1] - P[va * 3 + 1], P[vc * 3 + 2] - P[va * 3 + 2]};
    float de1[3] = {e2[1] * g[2] - e2[2] * g[1], e2[2] * g[0] - e2[0] * g[2], e2[0] * g[1] - e2[1] * g[0]};   // e2 x g
    float de2[3] = {g[1] * e1[2] - g[2] * e1[1], g[2] * e1[0] - g[0] * e1[2], g[0] * e1[1] - g[1] * e1[0]};   // g x e1
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = -de1[k] - de2[k]; o[3 + k] = de1[k]; o[6 + k] = de2[k]; }
}

// |p - c|^2 of one row of point_cloud_loss_mesh_grid
__device__ __forceinline__ float bf_sqdist_row(const float *__restrict__ p, const float *__restrict__ c) {
    const float d0 = p[0] - c[0], d1 = p[1] - c[1], d2 = p[2] - c[2];
    return d0 * d0 + d1 * d1 + d2 * d2;
}

// THE walk over the incident (face, corner) entries adj[adj_start[v] .. adj_start[v + 1]) of vertex v (entry = face * 4 + corner, in the
// order compute_normal_torch adds them), BF_ADJ_BATCH at a time and level by level: the batch's entries, then mid(entry) of all, then
// fetch(mid) of all, then add(value) in list order for the real entries alone.  Each level's loads are in flight together - entry by
// entry the walk was a chain of dependent round trips per face.  A batch is padded with -1: mid and fetch are called for a padding
// entry too and must read something safe (nothing, or row 0); add is not.
template <class M, class T, class Mid, class Fetch, class Add>
__device__ __forceinline__ void bf_adj_walk2(const int *__restrict__ adj_start, const int *__restrict__ adj, int v, Mid mid, Fetch fetch, Add add) {
    const int i0 = adj_start[v], i1 = adj_start[v + 1];
    for (int base = i0; base < i1; base += BF_ADJ_BATCH) {
        int a[BF_ADJ_BATCH];
        M m[BF_ADJ_BATCH];
        T x[BF_ADJ_BATCH];
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) a[e] = base + e < i1 ? adj[base + e] : -1;
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) m[e] = mid(a[e]);
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) x[e] = fetch(m[e]);
#pragma unroll
        for (int e = 0; e < BF_ADJ_BATCH; ++e) if (a[e] >= 0) add(x[e]);
    }
}
// ... with one dependent level: fetch(entry)
template <class T, class Fetch, class Add>
__device__ __forceinline__ void bf_adj_walk(const int *__restrict__ adj_start, const int *__restrict__ adj, int v, Fetch fetch, Add add) {
    bf_adj_walk2<int, T>(adj_start, adj, v, [](int a) { return a; }, fetch, add);
}

struct bf_row3 { float x, y, z; };        // a float[3] row by value (the stage keeps its normals as float4 rows)
__device__ __forceinline__ bf_row3 bf_load_row3(const float *__restrict__ p) { bf_row3 r = {p[0], p[1], p[2]}; return r; }

// the unit normal of vertex v: its incident faces' unit normals fnorm[nf] summed in list order, normalised again
__device__ __forceinline__ float4 bf_vertex_normal(const int *__restrict__ adj_start, const int *__restrict__ adj, int v, const float4 *__restrict__ fnorm) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    bf_adj_walk<float4>(adj_start, adj, v, [&](int a) { return a >= 0 ? fnorm[a >> 2] : make_float4(0.f, 0.f, 0.f, 0.f); },
                        [&](const float4 &n) { a0 += n.x; a1 += n.y; a2 += n.z; });
    return bf_unit_normal(a0, a1, a2);
}

// g[3] += vertex v's corner gradients out of dPf[nf][9], in list order
__device__ __forceinline__ void bf_corner_gather(const int *__restrict__ adj_start, const int *__restrict__ adj, int v, const float *__restrict__ dPf, float *g) {
    bf_adj_walk<bf_row3>(adj_start, adj, v, [&](int a) { return bf_load_row3(dPf + (size_t)(a >= 0 ? a >> 2 : 0) * 9 + (a >= 0 ? a & 3 : 0) * 3); },
                         [&](const bf_row3 &q) { g[0] += q.x; g[1] += q.y; g[2] += q.z; });
}

// g[3] += d/dn_v of the sum over faces of |na-nb|^2 + |nc-na|^2 + |nb-nc|^2, scaled: k2 (2 n_v - n_o1 - n_o2) per incident face in list
// order, o1 and o2 the face's other corners (two dependent levels: their ids, then their normals).  row(u) loads vertex u's normal - a
// float4 row in the stage, a float[3] row as bf_row3 stand-alone - and me = row(v)
template <class Row, class Load>
__device__ __forceinline__ void bf_laplacian_gather(const int *__restrict__ faces, const int *__restrict__ adj_start, const int *__restrict__ adj, int v,
                                                    Load row, const Row me, float k2, float *g) {
    struct Ids { int v1, v2; };
    struct Rows { Row o1, o2; };
    bf_adj_walk2<Ids, Rows>(adj_start, adj, v,
        [&](int a) { const int f = a >> 2, c = a & 3; Ids i = {a >= 0 ? faces[f * 3 + (c + 1) % 3] : 0, a >= 0 ? faces[f * 3 + (c + 2) % 3] : 0}; return i; },
        [&](const Ids &i) { Rows r = {row(i.v1), row(i.v2)}; return r; },
        [&](const Rows &r) { g[0] += k2 * (2.f * me.x - r.o1.x - r.o2.x); g[1] += k2 * (2.f * me.y - r.o1.y - r.o2.y); g[2] += k2 * (2.f * me.z - r.o1.z - r.o2.z); });
}
