// Host side of bf_topo_* / bf_vertex_normals(_vjp) / bf_normal_laplacian / bf_scan_point_loss / bf_normal_loss and of their *_dev
// twins (include/bodyfit.h): the SMPL+D stage's losses (smplify.py:236-245) as stateless calls, for a user's own torch loop.  Kernels:
// mesh_loss_kernels.hip.  Every operation is ONE body on a BfRouteCall (dev_route.h) and its two entry points are wrappers that check
// their arguments, count their route and hand the body its call: host arrays on the NULL stream with the block cache's buffers and one
// drain, or device pointers on the caller's stream with a bf_workspace, where nothing is drained, nothing is
// copied to the host and a scalar loss is one float in device memory.  Both routes of a call issue the same kernels in the same order
// with the same grids and arguments.
#include "bf_host.h"
#include "dev_route.h"
#include "mesh_loss_kernels.h"
#include "scan_kernels.h"


struct bf_topo {
    int device = 0, nv = 0, nf = 0;
    BfTopoDev d;
};

namespace {
constexpr int BF_ML_MAX = 1 << 28;        // vertices, faces or points of one call: face * 4 + corner and index * 3 stay inside an int

inline unsigned blocks(int n) { return (unsigned)((n + 255) / 256); }
}  // namespace

int bf_ml_check_count(const char *who, const char *what, int n) {
    if (n <= 0) return fail(BF_ERR_INVALID, std::string(who) + ": " + what + " must be positive");
    if (n > BF_ML_MAX) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(BF_ML_MAX) + " " + what);
    return BF_OK;
}

int bf_ml_dev_check(const char *who, const bf_workspace *ws, int device) {
    if (!ws) return fail(BF_ERR_INVALID, std::string(who) + ": the workspace is NULL");
    if (ws->device != device) return fail(BF_ERR_INVALID, std::string(who) + ": the workspace lives on another device");
    return BF_OK;
}

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
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<bf_topo> t(new bf_topo);
    t->device = device; t->nv = n_verts; t->nf = n_faces;
    HIP_TRY(t->d.build(std::vector<int>(faces, faces + n3), n_verts));
    *out = t.release();
    return BF_OK;
}

extern "C" void bf_topo_destroy(bf_topo *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

// ----------------------------------------------------------------------------------------------------------------------------------
// The bodies: one launch sequence per operation, on either route
// ----------------------------------------------------------------------------------------------------------------------------------
namespace {
// face and vertex normals of `d_v` on the device (the forward, and the first half of the reverse)
int bf_ml_normals_launch(const bf_topo *t, const float *d_v, float *d_fn, float *d_vn, float *d_out, hipStream_t st) {
    hipLaunchKernelGGL(bf_ml_face_kernel, dim3(blocks(t->nf)), dim3(256), 0, st, (const int *)t->d.faces.p, t->nf, d_v, d_fn);
    hipLaunchKernelGGL(bf_ml_vertex_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, (const int *)t->d.adj_start.p, (const int *)t->d.adj.p, t->nv,
                       (const float *)d_fn, d_vn, d_out);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// the last launch of the three scalar losses: d_loss[0] = the nblk block sums of d_part, reduced (mode, divisor: bf_ml_finish_kernel)
void bf_ml_finish_launch(const BfRouteCall &c, const float *d_part, unsigned nblk, int mode, float divisor, float *d_loss) {
    hipLaunchKernelGGL(bf_ml_finish_kernel, dim3(1), dim3(256), 0, c.stream, d_part, (int)nblk, mode, divisor, d_loss);
}

int bf_ml_normals(BfRouteCall &c, const bf_topo *t, const float *verts, float *normals) {
    BF_TRY(c.begin(t->device));
    const float *d_v = nullptr;
    float *d_fn = nullptr, *d_n = nullptr;
    BF_TRY(c.in(verts, (size_t)t->nv * 3, d_v));
    BF_TRY(c.scratch((size_t)t->nf * 4, d_fn));
    BF_TRY(c.out(normals, (size_t)t->nv * 3, d_n));
    BF_TRY(bf_ml_normals_launch(t, d_v, d_fn, nullptr, d_n, c.stream));
    return c.finish();
}

int bf_ml_normals_vjp(BfRouteCall &c, const bf_topo *t, const float *verts, const float *dnormals, float *dverts) {
    BF_TRY(c.begin(t->device));
    const hipStream_t st = c.stream;
    const size_t nv = (size_t)t->nv, nf = (size_t)t->nf;
    const float *d_v = nullptr, *d_dn = nullptr;
    float *d_fn = nullptr, *d_vn = nullptr, *d_raw = nullptr, *d_dPf = nullptr, *d_dv = nullptr;
    BF_TRY(c.in(verts, nv * 3, d_v));
    BF_TRY(c.in(dnormals, nv * 3, d_dn));
    BF_TRY(c.scratch(nf * 4, d_fn)); BF_TRY(c.scratch(nv * 4, d_vn)); BF_TRY(c.scratch(nv * 3, d_raw)); BF_TRY(c.scratch(nf * 9, d_dPf));
    BF_TRY(c.out(dverts, nv * 3, d_dv));
    BF_TRY(bf_ml_normals_launch(t, d_v, d_fn, d_vn, nullptr, st));
    hipLaunchKernelGGL(bf_ml_vraw_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, t->nv, (const float *)d_vn, d_dn, d_raw);
    hipLaunchKernelGGL(bf_ml_fgrad_kernel, dim3(blocks(t->nf)), dim3(256), 0, st, (const int *)t->d.faces.p, t->nf, d_v, (const float *)d_fn,
                       (const float *)d_raw, d_dPf);
    hipLaunchKernelGGL(bf_ml_gather_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, (const int *)t->d.adj_start.p, (const int *)t->d.adj.p, t->nv,
                       (const float *)d_dPf, d_dv);
    return c.finish();
}

// (loss or dnorms is wanted)
int bf_ml_laplacian(BfRouteCall &c, const bf_topo *t, const float *norms, float *loss, float *dnorms) {
    BF_TRY(c.begin(t->device));
    const hipStream_t st = c.stream;
    const unsigned nblk = blocks(t->nf);
    const float *d_n = nullptr;
    float *d_part = nullptr, *d_loss = nullptr, *d_dn = nullptr;
    BF_TRY(c.in(norms, (size_t)t->nv * 3, d_n));
    if (loss) {
        BF_TRY(c.scratch(nblk, d_part));
        BF_TRY(c.out(loss, 1, d_loss));
        hipLaunchKernelGGL(bf_ml_lap_partial_kernel, dim3(nblk), dim3(256), 0, st, (const int *)t->d.faces.p, t->nf, d_n, d_part);
        bf_ml_finish_launch(c, d_part, nblk, 0, (float)t->nf, d_loss);
    }
    if (dnorms) {
        BF_TRY(c.out(dnorms, (size_t)t->nv * 3, d_dn));
        hipLaunchKernelGGL(bf_ml_lap_grad_kernel, dim3(blocks(t->nv)), dim3(256), 0, st, (const int *)t->d.faces.p, (const int *)t->d.adj_start.p,
                           (const int *)t->d.adj.p, t->nf, t->nv, d_n, d_dn);
    }
    return c.finish();
}

int bf_ml_point_loss(BfRouteCall &c, bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints) {
    BF_TRY(c.begin(s->device));
    const hipStream_t st = c.stream;
    const size_t N = (size_t)n;
    const unsigned nblk = blocks(n);
    const float *d_p = nullptr;
    const ScanDev *d_s = nullptr;
    int *d_f = nullptr;
    float *d_c = nullptr, *d_part = nullptr, *d_loss = nullptr, *d_dp = nullptr;
    BF_TRY(c.in(points, N * 3, d_p));
    // (the launch writes both: an output not wanted lands in a buffer of the call)
    BF_TRY(c.out((int *)face_ids, N, d_f, true));
    BF_TRY(c.out(nearest, N * 3, d_c, true));
    BF_TRY(bf_ml_scan_dev(c, s, d_s));
    // the closest-point launch of scan_nearest (scan_api.hip; no warm start, no barycentrics), then the reduction on the points already there
    bf_nearest_launch(dim3((n + 3) / 4, 1), st, d_s, d_p, n, d_f, d_c, (float *)nullptr, 0);
    if (loss || dpoints) {
        BF_TRY(c.scratch(nblk, d_part));
        BF_TRY(c.out(loss, 1, d_loss, true));
        hipLaunchKernelGGL(bf_ml_pc_partial_kernel, dim3(nblk), dim3(256), 0, st, n, d_p, (const float *)d_c, d_part);
        bf_ml_finish_launch(c, d_part, nblk, 1, 1.f, d_loss);
    }
    if (dpoints) {
        BF_TRY(c.out(dpoints, N * 3, d_dp));
        hipLaunchKernelGGL(bf_ml_pc_grad_kernel, dim3(nblk), dim3(256), 0, st, n, d_p, (const float *)d_c, (const float *)d_loss, d_dp);
    }
    return c.finish();
}

// closest_face_norms[n][3] (the host entry: rows gathered by the caller), or face_ids[n] into face_norm_table[n_faces][3] on the device
// (the device entry: gathered in the kernel).  (loss or dpoint_norms is wanted)
int bf_ml_normal_loss(BfRouteCall &c, int device, int n, const float *closest_face_norms, const int32_t *face_ids, const float *face_norm_table,
                      int n_faces, const float *point_norms, float *loss, float *dpoint_norms) {
    BF_TRY(c.begin(device));
    const size_t N = (size_t)n;
    const unsigned nblk = blocks(n);
    const float *d_fn = nullptr, *d_pn = nullptr;
    float *d_part = nullptr, *d_loss = nullptr, *d_dpn = nullptr;
    BF_TRY(c.in(closest_face_norms, N * 3, d_fn));
    BF_TRY(c.in(point_norms, N * 3, d_pn));
    BF_TRY(c.scratch(nblk, d_part));
    BF_TRY(c.out(loss, 1, d_loss, true));
    BF_TRY(c.out(dpoint_norms, N * 3, d_dpn));
    if (face_ids)
        hipLaunchKernelGGL(bf_ml_normal_gather_partial_kernel, dim3(nblk), dim3(256), 0, c.stream, n, (const int *)face_ids, face_norm_table,
                           n_faces, d_pn, d_part, d_dpn);
    else
        hipLaunchKernelGGL(bf_ml_normal_partial_kernel, dim3(nblk), dim3(256), 0, c.stream, n, d_fn, d_pn, d_part, d_dpn);
    bf_ml_finish_launch(c, d_part, nblk, 0, (float)n, d_loss);
    return c.finish();
}
}  // namespace

// ----------------------------------------------------------------------------------------------------------------------------------
// The entry points: the arguments checked (a refused call has queued nothing), the route counted, the body run on that route's call
// ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int bf_vertex_normals(const bf_topo *t, const float *verts, float *normals) {
    if (!t || !verts || !normals) return fail(BF_ERR_INVALID, "bf_vertex_normals: bad argument");
    ++bf_route_stats().host;
    BfRouteCall c(nullptr, nullptr);
    return bf_ml_normals(c, t, verts, normals);
}

extern "C" int bf_vertex_normals_dev(const bf_topo *t, const float *verts, float *normals, bf_workspace *ws, void *stream) {
    const char *who = "bf_vertex_normals_dev";
    if (!t || !verts || !normals) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, t->device));
    ++bf_route_stats().dev;
    BfRouteCall c(ws, (hipStream_t)stream);
    return bf_ml_normals(c, t, verts, normals);
}

extern "C" int bf_vertex_normals_vjp(const bf_topo *t, const float *verts, const float *dnormals, float *dverts) {
    if (!t || !verts || !dnormals || !dverts) return fail(BF_ERR_INVALID, "bf_vertex_normals_vjp: bad argument");
    ++bf_route_stats().host;
    BfRouteCall c(nullptr, nullptr);
    return bf_ml_normals_vjp(c, t, verts, dnormals, dverts);
}

extern "C" int bf_vertex_normals_vjp_dev(const bf_topo *t, const float *verts, const float *dnormals, float *dverts, bf_workspace *ws,
                                         void *stream) {
    const char *who = "bf_vertex_normals_vjp_dev";
    if (!t || !verts || !dnormals || !dverts) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, t->device));
    ++bf_route_stats().dev;
    BfRouteCall c(ws, (hipStream_t)stream);
    return bf_ml_normals_vjp(c, t, verts, dnormals, dverts);
}

extern "C" int bf_normal_laplacian(const bf_topo *t, const float *norms, float *loss, float *dnorms) {
    if (!t || !norms) return fail(BF_ERR_INVALID, "bf_normal_laplacian: bad argument");
    ++bf_route_stats().host;
    if (!loss && !dnorms) return BF_OK;
    BfRouteCall c(nullptr, nullptr);
    return bf_ml_laplacian(c, t, norms, loss, dnorms);
}

extern "C" int bf_normal_laplacian_dev(const bf_topo *t, const float *norms, float *loss, float *dnorms, bf_workspace *ws, void *stream) {
    const char *who = "bf_normal_laplacian_dev";
    if (!t || !norms) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, t->device));
    ++bf_route_stats().dev;
    if (!loss && !dnorms) return BF_OK;
    BfRouteCall c(ws, (hipStream_t)stream);
    return bf_ml_laplacian(c, t, norms, loss, dnorms);
}

extern "C" int bf_scan_point_loss(bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints) {
    const char *who = "bf_scan_point_loss";
    if (!s || !points) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_check_count(who, "points", n));
    ++bf_route_stats().host;
    BfRouteCall c(nullptr, nullptr);
    return bf_ml_point_loss(c, s, n, points, loss, face_ids, nearest, dpoints);
}

extern "C" int bf_scan_point_loss_dev(bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints,
                                      bf_workspace *ws, void *stream) {
    const char *who = "bf_scan_point_loss_dev";
    if (!s || !points) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, s->device));
    BF_TRY(bf_ml_check_count(who, "points", n));
    ++bf_route_stats().dev;
    BfRouteCall c(ws, (hipStream_t)stream);
    return bf_ml_point_loss(c, s, n, points, loss, face_ids, nearest, dpoints);
}

extern "C" int bf_normal_loss(int device, int n, const float *closest_face_norms, const float *point_norms, float *loss, float *dpoint_norms) {
    const char *who = "bf_normal_loss";
    if (!closest_face_norms || !point_norms) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_check_count(who, "points", n));
    ++bf_route_stats().host;
    if (!loss && !dpoint_norms) return BF_OK;
    BfRouteCall c(nullptr, nullptr);
    return bf_ml_normal_loss(c, device, n, closest_face_norms, nullptr, nullptr, 0, point_norms, loss, dpoint_norms);
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
    BfRouteCall c(ws, (hipStream_t)stream);
    return bf_ml_normal_loss(c, device, n, nullptr, face_ids, face_norm_table, n_faces, point_norms, loss, dpoint_norms);
}

// the backward of a scalar loss on the device route: out[n] = grad[n] * cotangent[0] (+ 0.0f), the cotangent read on the device.
// No buffer and no workspace: one launch on the caller's stream.
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
