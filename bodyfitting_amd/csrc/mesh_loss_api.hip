// Host side of bf_topo_* / bf_vertex_normals(_vjp) / bf_normal_laplacian / bf_scan_point_loss / bf_normal_loss (include/bodyfit.h):
// the SMPL+D stage's losses (smplify.py:236-245) as stateless calls on host arrays, for a user's own torch loop.  Kernels:
// mesh_loss_kernels.hip; the call's buffers come from the device's block cache; everything runs on the NULL stream, like
// bf_scan_nearest.  Their device route (bf_*_dev: device pointers, the caller's stream, a bf_workspace) is the second half of this file.
#include "bf_host.h"
#include "dev_route.h"
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
static int bf_ml_normals_launch(const bf_topo *t, const float *d_v, float *d_fn, float *d_vn, float *d_out, hipStream_t st = nullptr) {
    hipLaunchKernelGGL(bf_ml_face_kernel, dim3(blocks(t->nf)), dim3(256), 0, st, (const int *)t->faces.p, t->nf, d_v, d_fn);
    hipLaunchKernelGGL(bf_ml_vertex_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, (const int *)t->adj_start.p, (const int *)t->adj.p, t->nv,
                       (const float *)d_fn, d_vn, d_out);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_vertex_normals(const bf_topo *t, const float *verts, float *normals) {
    if (!t || !verts || !normals) return fail(BF_ERR_INVALID, "bf_vertex_normals: bad argument");
    ++bf_route_stats().host;
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
    ++bf_route_stats().host;
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
    ++bf_route_stats().host;
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
    ++bf_route_stats().host;
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
    ++bf_route_stats().host;
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

// ----------------------------------------------------------------------------------------------------------------------------------
// The device route (dev_route.h) of the calls above and of bf_scan_nearest: the twin's kernels in the twin's order, with its grids and
// arguments, on the caller's stream; every array a device pointer, read and written where it lies; scratch from the workspace.  Nothing
// is drained and nothing is copied to the host: a scalar loss is one float in device memory.
// ----------------------------------------------------------------------------------------------------------------------------------
namespace {
// what every *_dev call here checks first: -> BF_OK, or the refusal (nothing has been queued)
int bf_ml_dev_check(const char *who, const bf_workspace *ws, int device) {
    if (!ws) return fail(BF_ERR_INVALID, std::string(who) + ": the workspace is NULL");
    if (ws->device != device) return fail(BF_ERR_INVALID, std::string(who) + ": the workspace lives on another device");
    return BF_OK;
}

template <class T>
int bf_ml_take(bf_workspace *ws, size_t count, T **p) {
    void *v = nullptr;
    BF_TRY(bf_ws_take(ws, count * sizeof(T), &v));
    *p = (T *)v;
    return BF_OK;
}

// the scan's ScanDev in device memory, made once per scan: complete on the device when this returns (later calls come on any stream)
int bf_scan_resident(bf_scan *s, const ScanDev **out) {
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (!s->dev_resident.p) {
        HIP_TRY(s->dev_resident.upload(std::vector<ScanDev>(1, s->dev)));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    *out = s->dev_resident.p;
    return BF_OK;
}
}  // namespace

extern "C" int bf_vertex_normals_dev(const bf_topo *t, const float *verts, float *normals, bf_workspace *ws, void *stream) {
    const char *who = "bf_vertex_normals_dev";
    if (!t || !verts || !normals) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, t->device));
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(t->device));
    const hipStream_t st = (hipStream_t)stream;
    BfWsCall call(ws, st);
    BF_TRY(call.begin());
    float *d_fn = nullptr;
    BF_TRY(bf_ml_take(ws, (size_t)t->nf * 4, &d_fn));
    return bf_ml_normals_launch(t, verts, d_fn, nullptr, normals, st);
}

extern "C" int bf_vertex_normals_vjp_dev(const bf_topo *t, const float *verts, const float *dnormals, float *dverts, bf_workspace *ws,
                                         void *stream) {
    const char *who = "bf_vertex_normals_vjp_dev";
    if (!t || !verts || !dnormals || !dverts) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, t->device));
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(t->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t nv = (size_t)t->nv, nf = (size_t)t->nf;
    BfWsCall call(ws, st);
    BF_TRY(call.begin());
    float *d_fn = nullptr, *d_vn = nullptr, *d_raw = nullptr, *d_dPf = nullptr;
    BF_TRY(bf_ml_take(ws, nf * 4, &d_fn)); BF_TRY(bf_ml_take(ws, nv * 4, &d_vn));
    BF_TRY(bf_ml_take(ws, nv * 3, &d_raw)); BF_TRY(bf_ml_take(ws, nf * 9, &d_dPf));
    BF_TRY(bf_ml_normals_launch(t, verts, d_fn, d_vn, nullptr, st));
    hipLaunchKernelGGL(bf_ml_vraw_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, t->nv, (const float *)d_vn, dnormals, d_raw);
    hipLaunchKernelGGL(bf_ml_fgrad_kernel, dim3(blocks(t->nf)), dim3(256), 0, st, (const int *)t->faces.p, t->nf, verts, (const float *)d_fn,
                       (const float *)d_raw, d_dPf);
    hipLaunchKernelGGL(bf_ml_gather_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, (const int *)t->adj_start.p, (const int *)t->adj.p, t->nv,
                       (const float *)d_dPf, dverts);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_normal_laplacian_dev(const bf_topo *t, const float *norms, float *loss, float *dnorms, bf_workspace *ws, void *stream) {
    const char *who = "bf_normal_laplacian_dev";
    if (!t || !norms) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, t->device));
    ++bf_route_stats().dev;
    if (!loss && !dnorms) return BF_OK;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(t->device));
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = blocks(t->nf);
    BfWsCall call(ws, st);
    BF_TRY(call.begin());
    if (loss) {
        float *d_part = nullptr;
        BF_TRY(bf_ml_take(ws, nblk, &d_part));
        hipLaunchKernelGGL(bf_ml_lap_partial_kernel, dim3(nblk), dim3(256), 0, st, (const int *)t->faces.p, t->nf, norms, d_part);
        hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)d_part, (int)nblk, 0, (float)t->nf, loss);
    }
    if (dnorms)
        hipLaunchKernelGGL(bf_ml_lap_grad_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, (const int *)t->faces.p, (const int *)t->adj_start.p,
                           (const int *)t->adj.p, t->nf, t->nv, norms, dnorms);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_scan_point_loss_dev(bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints,
                                      bf_workspace *ws, void *stream) {
    const char *who = "bf_scan_point_loss_dev";
    if (!s || !points) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, s->device));
    BF_TRY(bf_ml_check_count(who, "points", n));
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(s->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)n;
    const unsigned nblk = blocks(n);
    const ScanDev *d_s = nullptr;
    BF_TRY(bf_scan_resident(s, &d_s));
    BfWsCall call(ws, st);
    BF_TRY(call.begin());
    int *d_f = (int *)face_ids;
    float *d_c = nearest, *d_loss = loss, *d_part = nullptr;
    if (!d_f) BF_TRY(bf_ml_take(ws, N, &d_f));
    if (!d_c) BF_TRY(bf_ml_take(ws, N * 3, &d_c));
    bf_nearest_launch(dim3((n + 3) / 4, 1), st, d_s, points, n, d_f, d_c, (float *)nullptr, 0);
    if (loss || dpoints) {
        BF_TRY(bf_ml_take(ws, nblk, &d_part));
        if (!d_loss) BF_TRY(bf_ml_take(ws, 1, &d_loss));
        hipLaunchKernelGGL(bf_ml_pc_partial_kernel, dim3(nblk), dim3(256), 0, st, n, points, (const float *)d_c, d_part);
        hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)d_part, (int)nblk, 1, 1.f, d_loss);
    }
    if (dpoints)
        hipLaunchKernelGGL(bf_ml_pc_grad_kernel, dim3(nblk), dim3(256), 0, st, n, points, (const float *)d_c, (const float *)d_loss, dpoints);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_scan_nearest_dev(bf_scan *s, int n, const float *points, int32_t *face_ids, float *nearest, float *bary, bf_workspace *ws,
                                   void *stream) {
    const char *who = "bf_scan_nearest_dev";
    if (!s || !points) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, s->device));
    BF_TRY(bf_ml_check_count(who, "points", n));
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(s->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)n;
    const ScanDev *d_s = nullptr;
    BF_TRY(bf_scan_resident(s, &d_s));
    BfWsCall call(ws, st);
    BF_TRY(call.begin());
    // (the twin's launch writes all three: an output not wanted lands in the workspace)
    int *d_f = (int *)face_ids;
    float *d_c = nearest, *d_b = bary;
    if (!d_f) BF_TRY(bf_ml_take(ws, N, &d_f));
    if (!d_c) BF_TRY(bf_ml_take(ws, N * 3, &d_c));
    if (!d_b) BF_TRY(bf_ml_take(ws, N * 3, &d_b));
    bf_nearest_launch(dim3((n + 3) / 4, 1), st, d_s, points, n, d_f, d_c, d_b, 0);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_normal_loss_dev(int device, int n, const int32_t *face_ids, const float *face_norm_table, int n_faces,
                                  const float *point_norms, float *loss, float *dpoint_norms, bf_workspace *ws, void *stream) {
    const char *who = "bf_normal_loss_dev";
    if (!face_ids || !face_norm_table || !point_norms) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, device));
    BF_TRY(bf_ml_check_count(who, "points", n));
    BF_TRY(bf_ml_check_count(who, "n_faces", n_faces));
    ++bf_route_stats().dev;
    if (!loss && !dpoint_norms) return BF_OK;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(device));
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = blocks(n);
    BfWsCall call(ws, st);
    BF_TRY(call.begin());
    float *d_part = nullptr, *d_loss = loss;
    BF_TRY(bf_ml_take(ws, nblk, &d_part));
    if (!d_loss) BF_TRY(bf_ml_take(ws, 1, &d_loss));
    hipLaunchKernelGGL(bf_ml_normal_gather_partial_kernel, dim3(nblk), dim3(256), 0, st, n, (const int *)face_ids, face_norm_table, n_faces,
                       point_norms, d_part, dpoint_norms);
    hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)d_part, (int)nblk, 0, (float)n, d_loss);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// the backward of a scalar loss on the device route: out[n] = grad[n] * cotangent[0] (+ 0.0f), the cotangent read on the device
extern "C" int bf_scale_gradient_dev(int device, int n, const float *grad, const float *cotangent, int plus_zero, float *out, void *stream) {
    const char *who = "bf_scale_gradient_dev";
    if (!grad || !cotangent || !out) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_check_count(who, "n", n));
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(bf_ml_scale_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, n, grad, cotangent, plus_zero ? 1 : 0, out);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}
