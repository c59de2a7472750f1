// Host side of the scan (use_mesh) objects: grid construction, the closest-point, inside and intersection queries, and attaching a
// frame's scans to a batch.  The per-iteration schedule that fits against them is dense_api.hip.
#include "bf_host.h"
#include "dev_route.h"
#include "grid_kernels.h"
#include "scan_kernels.h"

void bf_batch_unlink_scans(bf_batch *b) {
    for (bf_scan *sc : b->scans) {
        if (!sc) continue;
        auto it = std::find(sc->holders.begin(), sc->holders.end(), b);
        if (it != sc->holders.end()) sc->holders.erase(it);
    }
    b->scans.clear();
    b->cface_valid = false;
    if (b->cscale.p) { (void)hipFree(b->cscale.p); b->cscale.p = nullptr; }
}

extern "C" {

// MeshGridSearcher.set_mesh (utils/mesh_grid_searcher.py:56-79) + insert_grid_surface
// (mesh_grid_kernel.cu:110-157): same cells, same triangle -> cell assignment, deterministic lists.
int bf_scan_create(int device, int n_verts, const float *verts, int n_faces, const int32_t *faces, bf_scan **out) {
    if (!verts || !faces || !out || n_verts <= 0 || n_faces <= 0) return fail(BF_ERR_INVALID, "bf_scan_create: bad argument");
    *out = nullptr;
    for (int i = 0; i < n_faces * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n_verts) return fail(BF_ERR_INVALID, "bf_scan_create: face index out of range");
    HIP_TRY(hipSetDevice(device));
    float mn[3] = {verts[0], verts[1], verts[2]}, mx[3] = {verts[0], verts[1], verts[2]};
    for (int v = 1; v < n_verts; ++v)
        for (int d = 0; d < 3; ++d) { mn[d] = std::min(mn[d], verts[v * 3 + d]); mx[d] = std::max(mx[d], verts[v * 3 + d]); }
    // float32 arithmetic in the order torch evaluates it
    float ext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    float prod = ext[0] * ext[1]; prod = prod * ext[2];
    float step = powf(prod / (float)n_verts, (float)(1.0 / 3.0));
    if (!(step > 0.f)) return fail(BF_ERR_INVALID, "bf_scan_create: degenerate (flat) scan");
    int num[3];
    float org[3];
    for (int d = 0; d < 3; ++d) {
        float l = std::max(floorf(ext[d] / step), 0.f) + 1.f;
        float c = (mx[d] + mn[d]) / 2.f;
        org[d] = c - step * l / 2.f;
        num[d] = (int)l;
    }
    const size_t ncell = (size_t)num[0] * num[1] * num[2];
    if (ncell > (size_t)1 << 28) return fail(BF_ERR_UNSUPPORTED, "bf_scan_create: grid too large");
    // everything below runs on the device: only the vertices and faces cross PCIe (the packed cell records would be ~50x that).
    // It runs on the NULL stream and this call waits for THAT stream only (hipStreamSynchronize(0), not hipDeviceSynchronize): the
    // library's own streams are all non-blocking, so neither the launches nor the wait are ordered behind a fit in flight on a
    // batch's stream - the previous frame's, in a capture - which keeps running under the build.
    // (A stream of its own per host thread was measured first and is what BF_SCAN_BUILD_STREAM=1 still selects: correct, but the
    //  extra stream changed the runtime's mapping of streams onto hardware queues, and config 5's fit - whose keypoint workgroups run
    //  on the batch's second stream beside the search - went from 62 to 139 ms.)
    static thread_local hipStream_t build_streams[16] = {};
    hipStream_t st = nullptr;
    static const bool own_stream = [] { const char *e = std::getenv("BF_SCAN_BUILD_STREAM"); return e && e[0] == '1'; }();
    if (own_stream && device >= 0 && device < 16) {
        if (!build_streams[device]) HIP_TRY(hipStreamCreateWithFlags(&build_streams[device], hipStreamNonBlocking));
        st = build_streams[device];
    }
    auto *s = new bf_scan();
    s->device = device; s->nv = n_verts; s->nf = n_faces;
    DevBuf<int> cursor, tris_raw;
    // (every device buffer of a scan and of its construction comes from the block cache: a capture makes one scan per frame)
    bool ok = s->verts.alloc_pooled((size_t)n_verts * 3) == hipSuccess &&
              s->faces.alloc_pooled((size_t)n_faces * 3) == hipSuccess &&
              s->cell_start.alloc_pooled(ncell + 1) == hipSuccess && cursor.alloc_pooled(ncell + 1) == hipSuccess &&
              s->face_norms.alloc_pooled((size_t)n_faces * 3) == hipSuccess;
    if (!ok) { delete s; return fail(BF_ERR_HIP, "bf_scan_create: device allocation failed"); }
    ScanDev &d = s->dev;
    d.nv = n_verts; d.nf = n_faces; d.nx = num[0]; d.ny = num[1]; d.nz = num[2];
    d.ox = org[0]; d.oy = org[1]; d.oz = org[2]; d.step = step; d.height = ext[1];
    d.verts = s->verts.p; d.faces = s->faces.p; d.cell_start = s->cell_start.p;
    d.cell_tris = nullptr; d.cell_pack = nullptr; d.cell_box = nullptr;
    const dim3 fgrid((n_faces + 255) / 256);
    int total = 0;
    // (pageable sources: the runtime stages them before the call returns; the copies themselves are ordered on `st`)
    hipError_t e = hipMemcpyAsync(s->verts.p, verts, (size_t)n_verts * 3 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->faces.p, faces, (size_t)n_faces * 3 * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->cell_start.p, 0, (ncell + 1) * sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bf_grid_count_kernel, fgrid, dim3(256), 0, st, d, s->cell_start.p);
        hipLaunchKernelGGL(bf_grid_scan_kernel, dim3(1), dim3(1024), 0, st, s->cell_start.p, cursor.p, (int)(ncell + 1));
        hipLaunchKernelGGL(bf_face_normal_kernel, fgrid, dim3(256), 0, st, (const float *)s->verts.p, (const int *)s->faces.p, n_faces,
                           s->face_norms.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, s->cell_start.p + ncell, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && total >= (1 << 28)) { delete s; return fail(BF_ERR_UNSUPPORTED, "bf_scan_create: more than 2^28 cell-list entries"); }   // (the search's queue entries: 28 bits of record index)
    if (e == hipSuccess && total > 0) {
        ok = tris_raw.alloc_pooled(total) == hipSuccess && s->cell_tris.alloc_pooled(total) == hipSuccess &&
             s->cell_pack.alloc_pooled((size_t)total * 12) == hipSuccess && s->cell_box.alloc_pooled((size_t)total * 8) == hipSuccess;
        if (!ok) { delete s; return fail(BF_ERR_HIP, "bf_scan_create: device allocation failed (cell lists)"); }
        d.cell_tris = s->cell_tris.p;
        d.cell_pack = (const float4 *)s->cell_pack.p;
        d.cell_box = (const float4 *)s->cell_box.p;
        hipLaunchKernelGGL(bf_grid_fill_kernel, fgrid, dim3(256), 0, st, d, cursor.p, tris_raw.p);
        hipLaunchKernelGGL(bf_grid_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, d, (const int *)tris_raw.p, s->cell_tris.p,
                           (float4 *)s->cell_pack.p, (float4 *)s->cell_box.p, total);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);       // tris_raw / cursor are released on return
    }
    if (e != hipSuccess) { delete s; return fail(BF_ERR_HIP, std::string("bf_scan_create: grid build: ") + hipGetErrorString(e)); }
    s->n_entries = total;
    *out = s;
    return BF_OK;
}

void bf_scan_destroy(bf_scan *s) {
    if (!s) return;
    // the scan's blocks go back to the cache without the device-wide wait a hipFree implies; a scan that a batch still holds may
    // be in use by queued work: wait for the device then, as hipFree would have - BEFORE the links' lock is taken (other threads'
    // bf_batch_set_scans / bf_batch_destroy do not queue up behind a device-wide wait)
    // ... and those batches forget ALL their scans and are marked `scans_lost`: their next bf_fit / bf_fit_displacement FAILS
    // (BF_ERR_INVALID) until bf_batch_set_scans is called again - with NULL to go on without scans.  (Rounds 4-5 let the fit run
    // silently without the closest-point loss: a lifetime bug in the caller - Python's GC closing a Scan early - then showed up as
    // quietly different results.)  bf_batch_set_scans / bf_batch_destroy never touch this pointer again.
    bool held;
    { std::lock_guard<std::mutex> lk(bf_scan_links()); held = !s->holders.empty(); }
    if (held) {
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
    }
    {
        std::lock_guard<std::mutex> lk(bf_scan_links());
        while (!s->holders.empty()) {
            bf_batch *b = s->holders.back();
            bf_batch_unlink_scans(b);
            b->scans_lost = true;
        }
    }
    delete s;
}

int64_t bf_device_cache_trim(int device) {
    if (device < 0 || device >= 16 || hipSetDevice(device) != hipSuccess) return -1;
    return (int64_t)bf_pool_trim(device);
}
float bf_scan_height(const bf_scan *s) { return s ? s->dev.height : 0.f; }

int bf_scan_grid_info(const bf_scan *s, int32_t dims[3], float origin_step[4]) {
    if (!s || !dims || !origin_step) return fail(BF_ERR_INVALID, "bf_scan_grid_info: null argument");
    dims[0] = s->dev.nx; dims[1] = s->dev.ny; dims[2] = s->dev.nz;
    origin_step[0] = s->dev.ox; origin_step[1] = s->dev.oy; origin_step[2] = s->dev.oz; origin_step[3] = s->dev.step;
    return BF_OK;
}

// The two tensors insert_grid_surface hands back to its caller (mesh_grid.cpp:129-136, mesh_grid_kernel.cu:209-215):
// tri_num = inclusive cumulative triangle count per cell, tri_idx = face id + 1 per list entry (here: ascending per cell).
int bf_scan_grid_lists(const bf_scan *s, int32_t *tri_num, int32_t *tri_idx, int32_t *n_entries) {
    if (!s) return fail(BF_ERR_INVALID, "bf_scan_grid_lists: null scan");
    HIP_TRY(hipSetDevice(s->device));
    const size_t ncell = (size_t)s->dev.nx * s->dev.ny * s->dev.nz;
    if (n_entries) *n_entries = s->n_entries;
    if (tri_num) HIP_TRY(hipMemcpy(tri_num, s->cell_start.p + 1, ncell * sizeof(int), hipMemcpyDeviceToHost));
    if (tri_idx && s->n_entries > 0) {
        HIP_TRY(hipMemcpy(tri_idx, s->cell_tris.p, (size_t)s->n_entries * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < s->n_entries; ++i) tri_idx[i] += 1;
    }
    return BF_OK;
}

// The queries below are stateless calls on host arrays: each runs on the host route of a BfRouteCall (dev_route.h), which uploads the
// inputs into blocks of the device's cache, hands the kernels blocks for their outputs, drains the device once and copies back.  Only
// bf_scan_nearest is one of the calls a torch loop goes through: it has a *_dev twin and counts its route (bf_dev_route_stats).

// MeshGridSearcher.inside_mesh (utils/mesh_grid_searcher.py:86-91 -> search_inside_mesh, mesh_grid.cpp:74-90)
int bf_scan_inside(bf_scan *s, int n, const float *points, float *signs) {
    if (!s || n <= 0 || !points || !signs) return fail(BF_ERR_INVALID, "bf_scan_inside: bad argument");
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(s->device));
    const float *d_p = nullptr;
    float *d_s = nullptr;
    BF_TRY(c.in(points, (size_t)n * 3, d_p));
    BF_TRY(c.out(signs, (size_t)n, d_s));
    hipLaunchKernelGGL(bf_inside_mesh_kernel, dim3((n + 255) / 256), dim3(256), 0, c.stream, s->dev, d_p, n, d_s);
    return c.finish();
}

// MeshGridSearcher.intersects_any (utils/mesh_grid_searcher.py:93-99 -> search_intersect, mesh_grid.cpp:92-110)
int bf_scan_intersects(bf_scan *s, int n, const float *origins, const float *directions, uint8_t *hit) {
    if (!s || n <= 0 || !origins || !directions || !hit) return fail(BF_ERR_INVALID, "bf_scan_intersects: bad argument");
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(s->device));
    const float *d_o = nullptr, *d_d = nullptr;
    unsigned char *d_h = nullptr;
    BF_TRY(c.in(origins, (size_t)n * 3, d_o));
    BF_TRY(c.in(directions, (size_t)n * 3, d_d));
    BF_TRY(c.out((unsigned char *)hit, (size_t)n, d_h));
    hipLaunchKernelGGL(bf_intersect_kernel, dim3((n + 255) / 256), dim3(256), 0, c.stream, s->dev, d_o, d_d, n, d_h);
    return c.finish();
}

}  // extern "C"

// the scan's ScanDev in device memory, made once per scan: complete on the device when this returns (later calls come on any stream)
int bf_scan_resident(bf_scan *s, const ScanDev **out) {
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (!s->dev_resident.p) {
        HIP_TRY(s->dev_resident.upload(&s->dev, 1));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    *out = s->dev_resident.p;
    return BF_OK;
}

// the scan's ScanDev where the kernels of `c` read it: the host route uploads it with the call, the device route keeps it resident
int bf_ml_scan_dev(BfRouteCall &c, bf_scan *s, const ScanDev *&d_s) {
    if (c.ws) return bf_scan_resident(s, &d_s);
    return c.in(&s->dev, 1, d_s);
}

// MeshGridSearcher.nearest_points -> SurfaceNearest (utils/mesh_grid_searcher.py:6-15,81-84): the body of bf_scan_nearest and of
// bf_scan_nearest_dev.  The launch writes all three outputs: one not wanted lands in a buffer of the call
static int scan_nearest(BfRouteCall &c, bf_scan *s, int n, const float *points, int32_t *face_ids, float *nearest, float *bary) {
    BF_TRY(c.begin(s->device));
    const size_t N = (size_t)n;
    const float *d_p = nullptr;
    const ScanDev *d_s = nullptr;
    int *d_f = nullptr;
    float *d_c = nullptr, *d_b = nullptr;
    BF_TRY(c.in(points, N * 3, d_p));
    BF_TRY(c.out((int *)face_ids, N, d_f, true));
    BF_TRY(c.out(nearest, N * 3, d_c, true));
    BF_TRY(c.out(bary, N * 3, d_b, true));
    BF_TRY(bf_ml_scan_dev(c, s, d_s));
    bf_nearest_launch(dim3((n + 3) / 4, 1), c.stream, d_s, d_p, n, d_f, d_c, d_b, 0);
    return c.finish();
}

extern "C" {

int bf_scan_nearest(bf_scan *s, int n, const float *points, int32_t *face_ids, float *nearest, float *bary) {
    if (!s || n <= 0 || !points) return fail(BF_ERR_INVALID, "bf_scan_nearest: bad argument");
    ++bf_route_stats().host;
    BfRouteCall c(nullptr, nullptr);
    return scan_nearest(c, s, n, points, face_ids, nearest, bary);
}

int bf_scan_nearest_dev(bf_scan *s, int n, const float *points, int32_t *face_ids, float *nearest, float *bary, bf_workspace *ws, void *stream) {
    const char *who = "bf_scan_nearest_dev";
    if (!s || !points) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_ml_dev_check(who, ws, s->device));
    BF_TRY(bf_ml_check_count(who, "points", n));
    ++bf_route_stats().dev;
    BfRouteCall c(ws, (hipStream_t)stream);
    return scan_nearest(c, s, n, points, face_ids, nearest, bary);
}

/* bf_scan_nearest with a GUESS per query: hint[n,3] = where the caller believes the nearest point is (the fit loop hands the search its
 * own answer of the previous iteration this way).  The guess only bounds the search - the kernel checks it against what it found and
 * searches again without it when it was wrong - so the results are bf_scan_nearest's for ANY hint (NaN and points far off the surface
 * included).  reps > 0 and kernel_us: the launch is repeated with the same hint and its mean duration (device events) returned. */
int bf_scan_nearest_hinted(bf_scan *s, int n, const float *points, const float *hint, int32_t *face_ids, float *nearest, float *bary,
                           int reps, float *kernel_us) {
    if (!s || n <= 0 || !points) return fail(BF_ERR_INVALID, "bf_scan_nearest_hinted: bad argument");
    struct Events {                         // destroyed on every way out
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(s->device));
    const size_t N = (size_t)n;
    const float *d_p = nullptr, *d_h = nullptr;
    const ScanDev *d_s = nullptr;
    int *d_f = nullptr;
    float *d_c = nullptr, *d_b = nullptr;
    BF_TRY(c.in(points, N * 3, d_p));
    BF_TRY(c.in(hint, N * 3, d_h));
    BF_TRY(c.out((int *)face_ids, N, d_f, true));
    BF_TRY(c.out(nearest, N * 3, d_c, true));
    BF_TRY(c.out(bary, N * 3, d_b, true));
    BF_TRY(bf_ml_scan_dev(c, s, d_s));
    HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
    double total_ms = 0.0;
    for (int r = 0; r < std::max(reps, 1); ++r) {
        if (hint) HIP_TRY(hipMemcpyAsync(d_c, d_h, N * 3 * sizeof(float), hipMemcpyDeviceToDevice, c.stream));
        HIP_TRY(hipEventRecord(ev.e0, c.stream));
        bf_nearest_launch(dim3((n + 3) / 4, 1), c.stream, d_s, d_p, n, d_f, d_c, d_b, hint ? 1 : 0);
        HIP_TRY(hipEventRecord(ev.e1, c.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventSynchronize(ev.e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        total_ms += ms;
    }
    if (kernel_us) *kernel_us = (float)(total_ms * 1e3 / std::max(reps, 1));
    return c.finish();
}

// self-tests of the reference-arithmetic rule (nearest_rule_ref.h): its division helper against the caller's IEEE quotients, and the
// per-triangle rule on explicit patches
int bf_nearest_selftest_quot(int device, int n, const float *num, const float *den, float *out) {
    if (n <= 0 || !num || !den || !out) return fail(BF_ERR_INVALID, "bf_nearest_selftest_quot: bad argument");
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(device));
    const float *d_n = nullptr, *d_d = nullptr;
    float *d_o = nullptr;
    BF_TRY(c.in(num, (size_t)n, d_n));
    BF_TRY(c.in(den, (size_t)n, d_d));
    BF_TRY(c.out(out, (size_t)n, d_o));
    hipLaunchKernelGGL(bf_nearest_quot_kernel, dim3((n + 255) / 256), dim3(256), 0, c.stream, n, d_n, d_d, d_o);
    return c.finish();
}
int bf_nearest_selftest_rule(int device, int n, const float *patches, int general, float *dist, float *coeff) {
    if (n <= 0 || !patches || !dist || !coeff) return fail(BF_ERR_INVALID, "bf_nearest_selftest_rule: bad argument");
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(device));
    const float *d_p = nullptr;
    float *d_d = nullptr, *d_c = nullptr;
    BF_TRY(c.in(patches, (size_t)n * 9, d_p));
    BF_TRY(c.out(dist, (size_t)n, d_d));
    BF_TRY(c.out(coeff, (size_t)n * 3, d_c));
    hipLaunchKernelGGL(bf_nearest_rule_kernel, dim3((n + 63) / 64), dim3(64), 0, c.stream, n, d_p, d_d, d_c, general);
    return c.finish();
}

// SurfaceNearest.backward with respect to the query points (utils/mesh_grid_searcher.py:17-49, unfinished in the reference):
// dpoints = (d nearest / d points)^T dnearest for the faces / coefficients bf_scan_nearest returned
int bf_scan_nearest_backward(bf_scan *s, int n, const int32_t *face_ids, const float *bary, const float *dnearest, float *dpoints) {
    if (!s || n <= 0 || !face_ids || !bary || !dnearest || !dpoints) return fail(BF_ERR_INVALID, "bf_scan_nearest_backward: bad argument");
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(s->device));
    const int *d_f = nullptr;
    const float *d_b = nullptr, *d_g = nullptr;
    float *d_o = nullptr;
    BF_TRY(c.in((const int *)face_ids, (size_t)n, d_f));
    BF_TRY(c.in(bary, (size_t)n * 3, d_b));
    BF_TRY(c.in(dnearest, (size_t)n * 3, d_g));
    BF_TRY(c.out(dpoints, (size_t)n * 3, d_o));
    hipLaunchKernelGGL(bf_nearest_backward_kernel, dim3((n + 255) / 256), dim3(256), 0, c.stream, s->dev, n, d_f, d_b, d_g, d_o);
    return c.finish();
}

// use_mesh=True, meshfile per frame (smplify.py:146-156): one scan per frame; constant_scale = scan_height / 1.7
int bf_batch_set_scans(bf_batch *b, bf_scan *const *scans) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_set_scans: null batch");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    // (`scans_lost` is cleared only where the caller has said what this batch's scans are now: on a detach, or once the new scans
    //  are linked - a rejected array leaves a batch that lost its scans failing its fits)
    if (!scans) {                                  // detach
        std::lock_guard<std::mutex> lk(bf_scan_links());
        bf_batch_unlink_scans(b);
        b->scans_lost = false;
        return BF_OK;
    }
    std::vector<ScanDev> dev(b->F);
    std::vector<float> cs(b->F);
    for (int f = 0; f < b->F; ++f) {
        if (!scans[f] || scans[f]->device != b->m->device) return fail(BF_ERR_INVALID, "bf_batch_set_scans: missing scan or wrong device");
        dev[f] = scans[f]->dev;
        cs[f] = scans[f]->dev.height / 1.7f;
    }
    {
        std::lock_guard<std::mutex> lk(bf_scan_links());
        for (bf_scan *old : b->scans) {            // (the tables below are rewritten in place: no detach of cscale)
            auto it = std::find(old->holders.begin(), old->holders.end(), b);
            if (it != old->holders.end()) old->holders.erase(it);
        }
        b->scans.assign(scans, scans + b->F);
        for (bf_scan *sc : b->scans) sc->holders.push_back(b);
        b->scans_lost = false;
    }
    b->cface_valid = false;
    // (a capture attaches new scans every frame: the two small tables are written in place - a hipFree waits for the whole device)
    if (b->scan_dev.p && b->scan_dev.n == dev.size()) HIP_TRY(hipMemcpy(b->scan_dev.p, dev.data(), dev.size() * sizeof(ScanDev), hipMemcpyHostToDevice));
    else { b->scan_dev.release(); HIP_TRY(b->scan_dev.upload(dev)); }
    if (b->cscale.p && b->cscale.n == cs.size()) HIP_TRY(hipMemcpy(b->cscale.p, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    else { b->cscale.release(); HIP_TRY(b->cscale.upload(cs)); }
    // (the SMPL+D stage's table of the scans' face normals: written here, where the device is idle anyway, not by every
    //  bf_fit_displacement behind a hipFree)
    std::vector<const float *> fn(b->F);
    for (int f = 0; f < b->F; ++f) fn[f] = scans[f]->face_norms.p;
    if (b->scan_fn.p && b->scan_fn.n == fn.size()) HIP_TRY(hipMemcpy((void *)b->scan_fn.p, fn.data(), fn.size() * sizeof(const float *), hipMemcpyHostToDevice));
    else { b->scan_fn.release(); HIP_TRY(b->scan_fn.upload(fn)); }
    return bf_ensure_dense_buffers(b);
}

}  // extern "C"
