// Host side of bf_topo_* / bf_vertex_normals(_vjp) / bf_normal_laplacian / bf_scan_point_loss / bf_normal_loss (include/bodyfit.h):
// the SMPL+D stage's losses (smplify.py:236-245) as stateless calls on host arrays, for a user's own torch loop.  Kernels:
// mesh_loss_kernels.hip; the call's buffers come from the device's block cache; everything runs on the NULL stream, like
// bf_scan_nearest.
#include "bf_host.h"
#include "mesh_loss_kernels.h"
#include "scan_kernels.h"


struct bf_topo {
    int device = 0, nv = 0, nf = 0;
    DevBuf<int> faces, adj_start, adj;
};

namespace {
struct DrainOnExit { ~DrainOnExit() { (void)hipDeviceSynchronize(); } };
constexpr int BF_ML_MAX = 1 << 28;        // vertices, faces or points of one call: face * 4 + corner and index * 3 stay inside an int

inline unsigned blocks(int n) { return (unsigned)((n + 255) / 256); }

int bf_ml_check_count(const char *who, const char *what, int n) {
    if (n <= 0) return fail(BF_ERR_INVALID, std::string(who) + ": " + what + " must be positive");
    if (n > BF_ML_MAX) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(BF_ML_MAX) + " " + what);
    return BF_OK;
}
}  // namespace

extern "C" int bf_topo_create(int device, int n_verts, int n_faces, const int32_t *faces, bf_topo **out) {
    const char *who = "bf_topo_create";
    if (!out) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    *out = nullptr;
    if (!faces) return fail(BF_ERR_INVALID, std::string(who) + ": faces is NULL");
    BF_TRY(bf_ml_check_count(who, "n_verts", n_verts));
    BF_TRY(bf_ml_check_count(who, "n_faces", n_faces));
    const size_t n3 = (size_t)n_faces * 3;
    for (size_t i = 0; i < n3; ++i)
        if (faces[i] < 0 || faces[i] >= n_verts) return fail(BF_ERR_INVALID, std::string(who) + ": face index out of range");
    std::vector<int> host(faces, faces + n3), start, adj;
    bf_build_vertex_adjacency(host, n_verts, start, adj);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<bf_topo> t(new bf_topo);
    t->device = device; t->nv = n_verts; t->nf = n_faces;
    HIP_TRY(t->faces.upload(host));
    HIP_TRY(t->adj_start.upload(start));
    HIP_TRY(t->adj.upload(adj));
    *out = t.release();
    return BF_OK;
}

extern "C" void bf_topo_destroy(bf_topo *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

// face and vertex normals of `d_v` on the device (the forward, and the first half of the reverse)
static int bf_ml_normals_launch(const bf_topo *t, const float *d_v, float *d_fn, float *d_vn, float *d_out) {
    hipLaunchKernelGGL(bf_ml_face_kernel, dim3(blocks(t->nf)), dim3(256), 0, 0, (const int *)t->faces.p, t->nf, d_v, d_fn);
    hipLaunchKernelGGL(bf_ml_vertex_kernel, dim3(blocks(t->nv)), dim3(256), 0, 0, (const int *)t->adj_start.p, (const int *)t->adj.p, t->nv,
                       (const float *)d_fn, d_vn, d_out);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_vertex_normals(const bf_topo *t, const float *verts, float *normals) {
    if (!t || !verts || !normals) return fail(BF_ERR_INVALID, "bf_vertex_normals: bad argument");
    HIP_TRY(hipSetDevice(t->device));
    const size_t nv = (size_t)t->nv, nf = (size_t)t->nf;
    DevBuf<float> d_v, d_fn, d_n;
    DrainOnExit drain;               // (destroyed before the buffers: no kernel still uses a block when it goes back to the cache)
    HIP_TRY(d_v.upload_pooled(verts, nv * 3));
    HIP_TRY(d_fn.alloc_pooled(nf * 4)); HIP_TRY(d_n.alloc_pooled(nv * 3));
    BF_TRY(bf_ml_normals_launch(t, d_v.p, d_fn.p, nullptr, d_n.p));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(normals, d_n.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

extern "C" int bf_vertex_normals_vjp(const bf_topo *t, const float *verts, const float *dnormals, float *dverts) {
    if (!t || !verts || !dnormals || !dverts) return fail(BF_ERR_INVALID, "bf_vertex_normals_vjp: bad argument");
    HIP_TRY(hipSetDevice(t->device));
    const size_t nv = (size_t)t->nv, nf = (size_t)t->nf;
    DevBuf<float> d_v, d_dn, d_fn, d_vn, d_raw, d_dPf, d_dv;
    DrainOnExit drain;
    HIP_TRY(d_v.upload_pooled(verts, nv * 3));
    HIP_TRY(d_dn.upload_pooled(dnormals, nv * 3));
    HIP_TRY(d_fn.alloc_pooled(nf * 4)); HIP_TRY(d_vn.alloc_pooled(nv * 4)); HIP_TRY(d_raw.alloc_pooled(nv * 3));
    HIP_TRY(d_dPf.alloc_pooled(nf * 9)); HIP_TRY(d_dv.alloc_pooled(nv * 3));
    BF_TRY(bf_ml_normals_launch(t, d_v.p, d_fn.p, d_vn.p, nullptr));
    hipLaunchKernelGGL(bf_ml_vraw_kernel, dim3(blocks(t->nv)), dim3(256), 0, 0, t->nv, (const float *)d_vn.p, (const float *)d_dn.p, d_raw.p);
    hipLaunchKernelGGL(bf_ml_fgrad_kernel, dim3(blocks(t->nf)), dim3(256), 0, 0, (const int *)t->faces.p, t->nf, (const float *)d_v.p,
                       (const float *)d_fn.p, (const float *)d_raw.p, d_dPf.p);
    hipLaunchKernelGGL(bf_ml_gather_kernel, dim3(blocks(t->nv)), dim3(256), 0, 0, (const int *)t->adj_start.p, (const int *)t->adj.p, t->nv,
                       (const float *)d_dPf.p, d_dv.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dverts, d_dv.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

extern "C" int bf_normal_laplacian(const bf_topo *t, const float *norms, float *loss, float *dnorms) {
    if (!t || !norms) return fail(BF_ERR_INVALID, "bf_normal_laplacian: bad argument");
    if (!loss && !dnorms) return BF_OK;
    HIP_TRY(hipSetDevice(t->device));
    const size_t nv = (size_t)t->nv;
    const unsigned nblk = blocks(t->nf);
    DevBuf<float> d_n, d_part, d_loss, d_dn;
    DrainOnExit drain;
    HIP_TRY(d_n.upload_pooled(norms, nv * 3));
    if (loss) {
        HIP_TRY(d_part.alloc_pooled(nblk)); HIP_TRY(d_loss.alloc_pooled(1));
        hipLaunchKernelGGL(bf_ml_lap_partial_kernel, dim3(nblk), dim3(256), 0, 0, (const int *)t->faces.p, t->nf, (const float *)d_n.p, d_part.p);
        hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, 0, (const float *)d_part.p, (int)nblk, 0, (float)t->nf, d_loss.p);
    }
    if (dnorms) {
        HIP_TRY(d_dn.alloc_pooled(nv * 3));
        hipLaunchKernelGGL(bf_ml_lap_grad_kernel, dim3(blocks(t->nv)), dim3(256), 0, 0, (const int *)t->faces.p, (const int *)t->adj_start.p,
                           (const int *)t->adj.p, t->nf, t->nv, (const float *)d_n.p, d_dn.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (loss) HIP_TRY(hipMemcpy(loss, d_loss.p, sizeof(float), hipMemcpyDeviceToHost));
    if (dnorms) HIP_TRY(hipMemcpy(dnorms, d_dn.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

extern "C" int bf_scan_point_loss(bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints) {
    const char *who = "bf_scan_point_loss";
    if (!s || !points) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_check_count(who, "points", n));
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const unsigned nblk = blocks(n);
    DevBuf<float> d_p, d_c, d_part, d_loss, d_dp;
    DevBuf<int> d_f;
    DevBuf<ScanDev> d_s;
    DrainOnExit drain;
    HIP_TRY(d_p.upload_pooled(points, N * 3));
    HIP_TRY(d_c.alloc_pooled(N * 3)); HIP_TRY(d_f.alloc_pooled(N));
    HIP_TRY(d_s.upload_pooled(&s->dev, 1));
    // the closest-point launch of bf_scan_nearest (no warm start, no barycentrics), then the reduction on the points already there
    bf_nearest_launch(dim3((n + 3) / 4, 1), 0, (const ScanDev *)d_s.p, (const float *)d_p.p, n, d_f.p, d_c.p, (float *)nullptr, 0);
    if (loss || dpoints) {
        HIP_TRY(d_part.alloc_pooled(nblk)); HIP_TRY(d_loss.alloc_pooled(1));
        hipLaunchKernelGGL(bf_ml_pc_partial_kernel, dim3(nblk), dim3(256), 0, 0, n, (const float *)d_p.p, (const float *)d_c.p, d_part.p);
        hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, 0, (const float *)d_part.p, (int)nblk, 1, 1.f, d_loss.p);
    }
    if (dpoints) {
        HIP_TRY(d_dp.alloc_pooled(N * 3));
        hipLaunchKernelGGL(bf_ml_pc_grad_kernel, dim3(nblk), dim3(256), 0, 0, n, (const float *)d_p.p, (const float *)d_c.p,
                           (const float *)d_loss.p, d_dp.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (loss) HIP_TRY(hipMemcpy(loss, d_loss.p, sizeof(float), hipMemcpyDeviceToHost));
    if (face_ids) HIP_TRY(hipMemcpy(face_ids, d_f.p, N * sizeof(int), hipMemcpyDeviceToHost));
    if (nearest) HIP_TRY(hipMemcpy(nearest, d_c.p, N * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (dpoints) HIP_TRY(hipMemcpy(dpoints, d_dp.p, N * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

extern "C" int bf_normal_loss(int device, int n, const float *closest_face_norms, const float *point_norms, float *loss, float *dpoint_norms) {
    const char *who = "bf_normal_loss";
    if (!closest_face_norms || !point_norms) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_check_count(who, "points", n));
    if (!loss && !dpoint_norms) return BF_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t N = (size_t)n;
    const unsigned nblk = blocks(n);
    DevBuf<float> d_fn, d_pn, d_part, d_loss, d_dpn;
    DrainOnExit drain;
    HIP_TRY(d_fn.upload_pooled(closest_face_norms, N * 3));
    HIP_TRY(d_pn.upload_pooled(point_norms, N * 3));
    HIP_TRY(d_part.alloc_pooled(nblk)); HIP_TRY(d_loss.alloc_pooled(1));
    if (dpoint_norms) HIP_TRY(d_dpn.alloc_pooled(N * 3));
    hipLaunchKernelGGL(bf_ml_normal_partial_kernel, dim3(nblk), dim3(256), 0, 0, n, (const float *)d_fn.p, (const float *)d_pn.p, d_part.p,
                       d_dpn.p);
    hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, 0, (const float *)d_part.p, (int)nblk, 0, (float)n, d_loss.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (loss) HIP_TRY(hipMemcpy(loss, d_loss.p, sizeof(float), hipMemcpyDeviceToHost));
    if (dpoint_norms) HIP_TRY(hipMemcpy(dpoint_norms, d_dpn.p, N * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}
