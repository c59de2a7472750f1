// Host side of the stand-alone neural_renderer.Renderer (thirdparty/neural_renderer/neural_renderer/renderer.py; kernels:
// nr_kernels.hip, and tex_kernels.hip's projection / compose / depth).  Three objects: the renderer (image size, planes, light, one
// stream), a mesh resident on its device, and a tape - what the texture VJP needs of ONE render (pixel map, face records, light rows,
// flags), so that several renders of one mesh can be differentiated in one graph.  A geometry tape (BF_NR_TAPE_GEOMETRY) also keeps
// the render's vertices (world and projected), camera, super-sampled colours and unlit samples, and shares the mesh's topology:
// bf_nr_tape_vertex_grad forms d / d vertices, R, t from it (nr_kernels.hip: bf_nr_geometry_kernel, bf_nr_fold_kernel).
#include "bf_host.h"
#include "grid_kernels.h"
#include "nr_kernels.h"
#include "tex_bodies.h"
#include "dev_route.h"
#include "nr_tape_layout.h"

#include <climits>

static_assert(BF_NR_TAPE_REC_FLOATS == BF_TEX_REC && BF_NR_TAPE_VIEW_FLOATS * sizeof(float) == sizeof(TexView), "nr_tape_layout.h and the kernels disagree");

struct bf_nr {
    unsigned long long id = 0;        // never reused: meshes and tapes name their renderer by it (bf_nr_live)
    int device = 0, out = 0, is = 0, tiles = 0, aa = 1;
    float near = 0.1f, far = 100.f, bg[3] = {0.f, 0.f, 0.f};
    NrLight light{0.5f, 0.5f, {1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}, {0.f, 1.f, 0.f}, 1};      // renderer.py:17-19
    hipStream_t stream = nullptr;
    DevBuf<float> rgb, image, depth_image, alpha_image, grad_image;
    DevBuf<int> tile_start, cursor;
    int *h_total = nullptr;           // pinned: the number of tile-list entries the last render needed
    // the device route's (see "the two routes" below)
    hipEvent_t ev_total = nullptr;    // behind the 4-byte read-back of a device-route render: all such a render waits for
    hipEvent_t ev_dev = nullptr;      // behind the last device-route call, on that call's stream
    bool dev_pending = false;         // ... which no host-route call has waited for yet
};

// what one render leaves for its backward pass; the mesh's own (overwritten by its next render) or a tape's
struct NrFrame {
    DevBuf<float> pix, frec, light;
    int alloc(size_t npx, size_t nrec, bool lit) {
        HIP_TRY(pix.alloc_pooled(npx * 5)); HIP_TRY(frec.alloc_pooled(nrec * BF_TEX_REC));
        if (lit) HIP_TRY(light.alloc_pooled(nrec * 3));
        return BF_OK;
    }
};

// what never changes of a mesh, shared with its geometry tapes: the faces and the vertex -> (record, corner) incidence table over
// the 2 nf records of a fill-back render (record k >= nf: face k - nf with corner c at the face's corner 2 - c), rows ascending
struct NrTopology {
    DevBuf<int> faces, vstart, ventry;
};

struct bf_nr_mesh {
    unsigned long long owner = 0;
    int device = 0, nv = 0, nf = 0, ts = 0;
    bool has_tex = false;
    DevBuf<float> verts, tex, pv;
    DevBuf<int> tile_list;
    std::shared_ptr<NrTopology> topo;
};

struct bf_nr_tape {
    unsigned long long owner = 0;
    int device = 0, nf = 0, nrec = 0, ts = 0, lit = 0;
    NrFrame frame;
    // a geometry tape's own
    int flags = 0, nv = 0, ndc = 0;
    bool has_rgb = false, has_depth = false, has_alpha = false;
    TexView view{};
    NrLight light{};
    std::shared_ptr<NrTopology> topo;
    DevBuf<float> verts, pv, rgbmap, unlit;
    // where all of the above lie: the tape's own blocks (host route), or segments of the caller's storage (device route: the handle
    // owns no device memory, and d_view is the packed view in that storage)
    struct Mem { float *pix = nullptr, *frec = nullptr, *light = nullptr, *verts = nullptr, *pv = nullptr, *rgbmap = nullptr, *unlit = nullptr;
                 const TexView *d_view = nullptr; } mem;
    bool borrowed = false;
};

static std::mutex &nr_mu() { static std::mutex mu; return mu; }
static std::map<unsigned long long, bf_nr *> &nr_live() { static std::map<unsigned long long, bf_nr *> live; return live; }
static bf_nr *nr_find(unsigned long long id) {
    std::lock_guard<std::mutex> lk(nr_mu());
    auto it = nr_live().find(id);
    return it == nr_live().end() ? nullptr : it->second;
}

// ---- the two routes.  The host route runs on the renderer's private stream with blocks of the cache and ends
// drained; the device route (bf_nr_render_dev, bf_nr_tape_*_dev) runs on the caller's stream with the caller's arrays, a workspace's
// scratch and a tape that borrows the caller's storage.  The renderer's own buffers (rgb, tile_start, cursor, the pinned word) and a
// mesh's pv / tile lists serve both: a device-route call leaves ev_dev behind its work, which the next host-route call makes its
// stream wait for (a host-route call ends drained, so the other direction needs nothing), and device-route calls on different
// streams are ordered by the workspace's event (BfRouteCall::begin). ----
struct NrRouteStats { std::atomic<long long> renders{0}, growths{0}, bytes_back{0}; };
static NrRouteStats &nr_route_stats() { static NrRouteStats S; return S; }

// a host-route call's first step once the device is set: behind the renderer's last device-route call
static int nr_join_dev(bf_nr *r) {
    if (!r->dev_pending) return BF_OK;
    HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_dev, 0));
    r->dev_pending = false;
    return BF_OK;
}
// a device-route call's last step, on every way out
struct NrDevEnd {
    bf_nr *r;
    hipStream_t stream;
    ~NrDevEnd() {
        if (hipEventRecord(r->ev_dev, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); return; }
        r->dev_pending = true;
    }
};

// where one render reads its mesh and leaves its results (device memory all), on either route
struct NrTarget {
    hipStream_t stream;
    const float *verts, *tex;
    float *pix, *frec, *light;          // the frame; light NULL when unlit
    const TexView *d_view;              // device route: the packed view, read by pointer.  NULL: V by value
    float *rgb, *depth, *alpha;         // what the compose / depth / alpha kernels write, NULL: not wanted
};

static NrLight nr_light_of(const bf_nr *r, bool lit) { NrLight L = r->light; L.on = lit ? 1 : 0; return L; }

// projection, tile counts, scan, and the total on its way into the pinned word
static int nr_render_front(bf_nr *r, bf_nr_mesh *M, const NrTarget &T, const TexView &V, int nrec, bool lit) {
    const int is = r->is, tiles = r->tiles, ntile = tiles * tiles, cap = (int)M->tile_list.n;
    if (T.d_view)
        hipLaunchKernelGGL(bf_tex_project_view_kernel, dim3((M->nv + 255) / 256), dim3(256), 0, T.stream, M->nv, T.verts, T.d_view, M->pv.p);
    else
        hipLaunchKernelGGL(bf_tex_project_kernel, dim3((M->nv + 255) / 256), dim3(256), 0, T.stream, M->nv, T.verts, V, M->pv.p);
    HIP_TRY(hipMemsetAsync(r->tile_start.p, 0, (size_t)(ntile + 1) * sizeof(int), T.stream));
    hipLaunchKernelGGL(bf_nr_face_kernel, dim3((nrec + 255) / 256), dim3(256), 0, T.stream, M->nf, nrec, (const int *)M->topo->faces.p, (const float *)M->pv.p,
                       T.verts, nr_light_of(r, lit), is, tiles, T.frec, T.light, r->tile_start.p, (int *)nullptr, (int *)nullptr, 0, cap);
    hipLaunchKernelGGL(bf_grid_scan_kernel, dim3(1), dim3(1024), 0, T.stream, r->tile_start.p, r->cursor.p, ntile + 1);
    HIP_TRY(hipMemcpyAsync(r->h_total, r->tile_start.p + ntile, sizeof(int), hipMemcpyDeviceToHost, T.stream));
    return BF_OK;
}

// the fill pass, the rasteriser and the pooled outputs
static int nr_render_back(bf_nr *r, bf_nr_mesh *M, const NrTarget &T, int nrec, bool lit, bool want_rgb) {
    const int is = r->is, tiles = r->tiles, ntile = tiles * tiles, cap = (int)M->tile_list.n, npo = r->out * r->out;
    hipLaunchKernelGGL(bf_nr_face_kernel, dim3((nrec + 255) / 256), dim3(256), 0, T.stream, M->nf, nrec, (const int *)M->topo->faces.p, (const float *)M->pv.p,
                       T.verts, nr_light_of(r, lit), is, tiles, T.frec, T.light, r->tile_start.p, r->cursor.p, M->tile_list.p, 1, cap);
    hipLaunchKernelGGL(bf_nr_raster_kernel, dim3((ntile + 3) / 4), dim3(256), 0, T.stream, is, tiles, M->nf, (const float *)T.frec, (const float *)T.light,
                       (const int *)r->tile_start.p, (const int *)M->tile_list.p, want_rgb ? T.tex : (const float *)nullptr, M->ts,
                       r->near, r->far, r->bg[0], r->bg[1], r->bg[2], T.pix, r->rgb.p, cap);
    if (T.rgb) hipLaunchKernelGGL(bf_tex_compose_kernel, dim3((3 * npo + 255) / 256), dim3(256), 0, T.stream, r->out, r->aa, (const float *)r->rgb.p, T.rgb);
    if (T.depth) hipLaunchKernelGGL(bf_tex_depth_kernel, dim3((npo + 255) / 256), dim3(256), 0, T.stream, r->out, r->aa, (const float *)T.pix, T.depth);
    if (T.alpha) hipLaunchKernelGGL(bf_nr_alpha_kernel, dim3((npo + 255) / 256), dim3(256), 0, T.stream, r->out, r->aa, (const float *)T.pix, T.alpha);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// what a geometry tape keeps beside the frame: copies on the render's stream of its vertices, projected vertices and colours, and
// (lit, with a directional term) the unlit samples from the textures as they are now.  The tape's mem.* are set.
static int nr_keep_geometry(bf_nr *r, bf_nr_mesh *M, bf_nr_tape *tp, const NrTarget &T) {
    const size_t nv3 = (size_t)M->nv * 3, npx = (size_t)r->is * r->is;
    tp->topo = M->topo;
    HIP_TRY(hipMemcpyAsync(tp->mem.verts, T.verts, nv3 * sizeof(float), hipMemcpyDeviceToDevice, T.stream));
    HIP_TRY(hipMemcpyAsync(tp->mem.pv, M->pv.p, nv3 * sizeof(float), hipMemcpyDeviceToDevice, T.stream));
    if (tp->mem.rgbmap) HIP_TRY(hipMemcpyAsync(tp->mem.rgbmap, r->rgb.p, npx * 3 * sizeof(float), hipMemcpyDeviceToDevice, T.stream));
    if (tp->mem.unlit) {
        hipLaunchKernelGGL(bf_nr_unlit_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, T.stream, r->is, M->nf, (const float *)tp->mem.pix,
                           (const float *)tp->mem.frec, T.tex, M->ts, tp->mem.unlit);
        HIP_TRY(hipGetLastError());
    }
    return BF_OK;
}

// the refusals both render entry points share, before any launch
static int nr_render_check(bf_nr *r, bf_nr_mesh *m, bool has_K, bool has_R, bool has_t, float orig_size, int ndc, bf_nr_tape **tape, int tape_flags) {
    if (!r || !m) return fail(BF_ERR_INVALID, "bf_nr_render: null handle");
    if (tape && (!tape_flags || (tape_flags & ~(BF_NR_TAPE_TEXTURES | BF_NR_TAPE_GEOMETRY))))
        return fail(BF_ERR_INVALID, "bf_nr_render_taped: tape_flags must be a non-empty set of BF_NR_TAPE_TEXTURES | BF_NR_TAPE_GEOMETRY");
    if (m->owner != r->id) return fail(BF_ERR_INVALID, "bf_nr_render: the mesh belongs to another renderer");
    if (!ndc && (!has_K || !has_R || !has_t || !(orig_size > 0.f)))
        return fail(BF_ERR_INVALID, "bf_nr_render: K, R, t and a positive orig_size are needed unless ndc is set");
    return BF_OK;
}

static std::unique_ptr<bf_nr_tape> nr_new_tape(bf_nr *r, bf_nr_mesh *m, int nrec, bool lit, int tape_flags, int ndc, bool rgb, bool depth, bool alpha,
                                               const TexView &V) {
    std::unique_ptr<bf_nr_tape> tp(new bf_nr_tape());
    tp->owner = r->id; tp->device = r->device; tp->nf = m->nf; tp->nrec = nrec; tp->ts = m->ts; tp->lit = lit;
    tp->flags = tape_flags; tp->nv = m->nv; tp->ndc = ndc ? 1 : 0;
    tp->has_rgb = rgb; tp->has_depth = depth; tp->has_alpha = alpha;
    tp->view = V; tp->light = nr_light_of(r, lit);
    return tp;
}

// the two kernels of the texture gradient: d_grad_rgb[3][out][out] -> d_grad_tex, every texel written once, then the large faces added
static int nr_texture_grad_issue(bf_nr *r, bf_nr_tape *tape, hipStream_t stream, const float *d_grad_rgb, float *d_grad_tex) {
    const int ts = tape->ts;
    const float *light = tape->lit ? tape->mem.light : nullptr;
    hipLaunchKernelGGL(bf_nr_backward_kernel, dim3(tape->nf), dim3(64), (size_t)ts * ts * ts * 3 * sizeof(float), stream, tape->nf, tape->nrec, r->is,
                       r->out, r->aa, (const float *)tape->mem.pix, (const float *)tape->mem.frec, light, ts, d_grad_rgb, d_grad_tex);
    hipLaunchKernelGGL(bf_nr_backward_large_kernel, dim3((r->is * r->is + 255) / 256), dim3(256), 0, stream, tape->nf, r->is, r->out, r->aa,
                       (const float *)tape->mem.pix, (const float *)tape->mem.frec, light, ts, d_grad_rgb, d_grad_tex);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// the geometry gradient's kernels.  Device memory all; g_*: NULL = zero; lrec NULL: no light term; partial NULL: no camera sums
struct NrGradIo {
    hipStream_t stream;
    const float *g_rgb, *g_depth, *g_alpha;
    float *grad_frec, *grad_lrec, *grad_verts, *partial, *out_R, *out_t;
};
static int nr_vertex_grad_issue(bf_nr *r, bf_nr_tape *tape, const NrGradIo &io) {
    const int blocks = (tape->nv + 255) / 256;
    NrGeo G{};
    G.faces = tape->topo->faces.p; G.pv = tape->mem.pv; G.verts = tape->mem.verts; G.pix = tape->mem.pix; G.frec = tape->mem.frec;
    G.rgbmap = tape->mem.rgbmap; G.unlit = tape->mem.unlit;
    G.g_rgb = io.g_rgb; G.g_depth = io.g_depth; G.g_alpha = io.g_alpha;
    G.nf = tape->nf; G.nrec = tape->nrec; G.is = r->is; G.out = r->out; G.aa = r->aa;
    hipLaunchKernelGGL(bf_nr_geometry_kernel, dim3(tape->nrec), dim3(64), 0, io.stream, G, tape->light, io.grad_frec, io.grad_lrec);
    if (tape->mem.d_view)
        hipLaunchKernelGGL(bf_nr_fold_view_kernel, dim3(blocks), dim3(256), 0, io.stream, tape->nv, tape->nrec, (const int *)tape->topo->vstart.p,
                           (const int *)tape->topo->ventry.p, (const float *)io.grad_frec, (const float *)io.grad_lrec, (const float *)tape->mem.verts,
                           tape->mem.d_view, io.grad_verts, io.partial);
    else
        hipLaunchKernelGGL(bf_nr_fold_kernel, dim3(blocks), dim3(256), 0, io.stream, tape->nv, tape->nrec, (const int *)tape->topo->vstart.p,
                           (const int *)tape->topo->ventry.p, (const float *)io.grad_frec, (const float *)io.grad_lrec, (const float *)tape->mem.verts,
                           tape->view, io.grad_verts, io.partial);
    if (io.partial) hipLaunchKernelGGL(bf_nr_fold_sum_kernel, dim3(1), dim3(64), 0, io.stream, blocks, (const float *)io.partial, io.out_R, io.out_t);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

static int nr_vertex_grad_check(bf_nr_tape *tape, bool g_rgb, bool g_depth, bool g_alpha, bool g_verts, bool g_cam) {
    if (!tape || !g_verts) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: null argument");
    if (!(tape->flags & BF_NR_TAPE_GEOMETRY)) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: the tape was made without BF_NR_TAPE_GEOMETRY");
    if ((g_rgb && !tape->has_rgb) || (g_depth && !tape->has_depth) || (g_alpha && !tape->has_alpha))
        return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: a cotangent for an output the render did not produce");
    if (tape->ndc && g_cam) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: an ndc render has no R or t");
    return BF_OK;
}

extern "C" {

void bf_nr_destroy(bf_nr *r) {
    if (!r) return;
    { std::lock_guard<std::mutex> lk(nr_mu()); nr_live().erase(r->id); }
    (void)hipSetDevice(r->device);
    if (r->dev_pending) (void)hipEventSynchronize(r->ev_dev);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->h_total) (void)hipHostFree(r->h_total);
    if (r->ev_total) (void)hipEventDestroy(r->ev_total);
    if (r->ev_dev) (void)hipEventDestroy(r->ev_dev);
    delete r;
}

int bf_nr_create(int device, int image_size, int anti_aliasing, float near, float far, const float *background, bf_nr **out) {
    if (!out) return fail(BF_ERR_INVALID, "bf_nr_create: null output");
    *out = nullptr;
    if (image_size <= 0 || !(near < far)) return fail(BF_ERR_INVALID, "bf_nr_create: image_size must be positive and near < far");
    if (image_size > 4096) return fail(BF_ERR_UNSUPPORTED, "bf_nr_create: image_size above 4096");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_nr_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto *r = new bf_nr();
    static std::atomic<unsigned long long> next_id{1};
    r->id = next_id++;
    r->device = device; r->out = image_size; r->aa = anti_aliasing ? 1 : 0; r->is = image_size * (r->aa ? 2 : 1);
    r->tiles = (r->is + BF_TEX_TILE - 1) / BF_TEX_TILE;
    r->near = near; r->far = far;
    if (background) std::memcpy(r->bg, background, sizeof r->bg);
    const size_t npo = (size_t)image_size * image_size, npx = (size_t)r->is * r->is, ntile = (size_t)r->tiles * r->tiles;
    const bool ok = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) == hipSuccess && r->rgb.alloc(npx * 3) == hipSuccess &&
                    r->image.alloc(npo * 3) == hipSuccess && r->depth_image.alloc(npo) == hipSuccess && r->alpha_image.alloc(npo) == hipSuccess &&
                    r->grad_image.alloc(npo * 3) == hipSuccess && r->tile_start.alloc(ntile + 1) == hipSuccess &&
                    r->cursor.alloc(ntile + 1) == hipSuccess && hipHostMalloc((void **)&r->h_total, sizeof(int)) == hipSuccess &&
                    hipEventCreateWithFlags(&r->ev_total, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&r->ev_dev, hipEventDisableTiming) == hipSuccess;
    if (!ok) { bf_nr_destroy(r); return fail(BF_ERR_HIP, "bf_nr_create: device allocation failed"); }
    *r->h_total = 0;
    { std::lock_guard<std::mutex> lk(nr_mu()); nr_live()[r->id] = r; }
    *out = r;
    return BF_OK;
}

int bf_nr_set_light(bf_nr *r, float ambient, float directional, const float *color_ambient, const float *color_directional, const float *direction) {
    if (!r || !color_ambient || !color_directional || !direction) return fail(BF_ERR_INVALID, "bf_nr_set_light: null argument");
    r->light.ambient = ambient; r->light.directional = directional;
    std::memcpy(r->light.color_ambient, color_ambient, 3 * sizeof(float));
    std::memcpy(r->light.color_directional, color_directional, 3 * sizeof(float));
    std::memcpy(r->light.direction, direction, 3 * sizeof(float));
    return BF_OK;
}

void bf_nr_mesh_destroy(bf_nr_mesh *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (bf_nr *r = nr_find(m->owner)) { (void)nr_join_dev(r); (void)hipStreamSynchronize(r->stream); }
    delete m;
}

int bf_nr_mesh_set_textures(bf_nr_mesh *m, const float *textures) {
    if (!m || !textures) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_textures: null argument");
    if (!m->ts) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_textures: the mesh was created without a texture size");
    bf_nr *r = nr_find(m->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_textures: the mesh's renderer was destroyed");
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(nr_join_dev(r));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const size_t ntex = (size_t)m->nf * m->ts * m->ts * m->ts * 3;
    if (!m->tex.p) HIP_TRY(m->tex.alloc(ntex));
    HIP_TRY(hipMemcpy(m->tex.p, textures, ntex * sizeof(float), hipMemcpyHostToDevice));
    m->has_tex = true;
    return BF_OK;
}

int bf_nr_mesh_set_vertices(bf_nr_mesh *m, const float *verts) {
    if (!m || !verts) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_vertices: null argument");
    bf_nr *r = nr_find(m->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_vertices: the mesh's renderer was destroyed");
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(nr_join_dev(r));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(m->verts.p, verts, (size_t)m->nv * 3 * sizeof(float), hipMemcpyHostToDevice));
    return BF_OK;
}

int bf_nr_mesh_create(bf_nr *r, int n_verts, const float *verts, int n_faces, const int32_t *faces, int texture_size, const float *textures,
                      bf_nr_mesh **out) {
    if (!out) return fail(BF_ERR_INVALID, "bf_nr_mesh_create: null output");
    *out = nullptr;
    if (!r || n_verts <= 0 || n_faces <= 0 || !verts || !faces) return fail(BF_ERR_INVALID, "bf_nr_mesh_create: bad argument");
    if (texture_size < 0 || texture_size == 1 || (textures && !texture_size))
        return fail(BF_ERR_INVALID, "bf_nr_mesh_create: texture_size must be 0 (no textures) or at least 2");
    if (texture_size > 16) return fail(BF_ERR_UNSUPPORTED, "bf_nr_mesh_create: texture_size above 16");
    if (n_faces > INT_MAX / 2) return fail(BF_ERR_UNSUPPORTED, "bf_nr_mesh_create: 2 x n_faces does not fit an int");
    if (n_faces > INT_MAX / 6) return fail(BF_ERR_UNSUPPORTED, "bf_nr_mesh_create: 6 x n_faces (the corner rows of the front and back records) does not fit an int");
    for (size_t i = 0; i < (size_t)n_faces * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n_verts) return fail(BF_ERR_INVALID, "bf_nr_mesh_create: face index out of range");
    HIP_TRY(hipSetDevice(r->device));
    std::unique_ptr<bf_nr_mesh> m(new bf_nr_mesh());
    m->owner = r->id; m->device = r->device; m->nv = n_verts; m->nf = n_faces; m->ts = texture_size;
    HIP_TRY(m->verts.upload(verts, (size_t)n_verts * 3));
    m->topo = std::make_shared<NrTopology>();
    HIP_TRY(m->topo->faces.upload(faces, (size_t)n_faces * 3));
    {   // counting sort of (record * 3 + corner) by vertex, records ascending
        std::vector<int> start((size_t)n_verts + 1, 0), entry((size_t)n_faces * 6);
        for (size_t i = 0; i < (size_t)n_faces * 3; ++i) start[(size_t)faces[i] + 1] += 2;
        for (int v = 0; v < n_verts; ++v) start[(size_t)v + 1] += start[v];
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int k = 0; k < 2 * n_faces; ++k)
            for (int c = 0; c < 3; ++c) {
                const bool back = k >= n_faces;
                entry[(size_t)at[faces[(size_t)(back ? k - n_faces : k) * 3 + (back ? 2 - c : c)]]++] = k * 3 + c;
            }
        HIP_TRY(m->topo->vstart.upload(start));
        HIP_TRY(m->topo->ventry.upload(entry));
    }
    HIP_TRY(m->pv.alloc((size_t)n_verts * 3));
    HIP_TRY(m->tile_list.alloc((size_t)n_faces * 4 + (size_t)r->tiles * r->tiles + 1024));         // (first guess; grown when a render says so)
    if (textures) BF_TRY(bf_nr_mesh_set_textures(m.get(), textures));
    *out = m.release();
    return BF_OK;
}

void bf_nr_tape_destroy(bf_nr_tape *tape) {
    if (!tape) return;
    if (!tape->borrowed) {               // (a device-route tape owns no device memory: nothing to wait for)
        (void)hipSetDevice(tape->device);
        if (bf_nr *r = nr_find(tape->owner)) (void)hipStreamSynchronize(r->stream);      // (the pool hands the blocks out again: nothing may still read them)
    }
    delete tape;
}

int bf_nr_render(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                 float *rgb, float *depth, float *alpha, bf_nr_tape **tape) {
    return bf_nr_render_taped(r, m, K, R, t, orig_size, fill_back, lightoff, ndc, rgb, depth, alpha, BF_NR_TAPE_TEXTURES, tape);
}

int bf_nr_render_taped(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                       float *rgb, float *depth, float *alpha, int tape_flags, bf_nr_tape **tape) {
    if (tape) *tape = nullptr;
    BF_TRY(nr_render_check(r, m, K, R, t, orig_size, ndc, tape, tape_flags));
    const bool tex_tape = tape && (tape_flags & BF_NR_TAPE_TEXTURES), geo_tape = tape && (tape_flags & BF_NR_TAPE_GEOMETRY);
    if ((rgb || tex_tape) && !m->has_tex) return fail(BF_ERR_INVALID, "bf_nr_render: rgb or a tape asked of a mesh without textures");
    ++bf_route_stats().host;
    HIP_TRY(hipSetDevice(r->device));
    BF_TRY(nr_join_dev(r));
    TexView V{};
    V.orig = -1.f;                                    // (bf_tex_project_kernel: pass the vertices through)
    if (!ndc) { std::memcpy(V.R, R, sizeof V.R); std::memcpy(V.t, t, sizeof V.t); std::memcpy(V.K, K, sizeof V.K); V.orig = orig_size; }
    const int nrec = fill_back ? 2 * m->nf : m->nf;
    const bool lit = !lightoff && (rgb || tex_tape);
    const size_t npx = (size_t)r->is * r->is, npo = (size_t)r->out * r->out, nv3 = (size_t)m->nv * 3;
    std::unique_ptr<bf_nr_tape> tp;
    NrFrame scratch;
    if (tape) tp = nr_new_tape(r, m, nrec, lit, tape_flags, ndc, rgb != nullptr, depth != nullptr, alpha != nullptr, V);
    NrFrame &F = tape ? tp->frame : scratch;
    BF_TRY(F.alloc(npx, (size_t)nrec, lit));
    const NrTarget T{r->stream, m->verts.p, m->tex.p, F.pix.p, F.frec.p, lit ? F.light.p : nullptr, nullptr,
                     rgb ? r->image.p : nullptr, depth ? r->depth_image.p : nullptr, alpha ? r->alpha_image.p : nullptr};
    for (int attempt = 0; attempt < 3; ++attempt) {
        BF_TRY(nr_render_front(r, m, T, V, nrec, lit));
        BF_TRY(nr_render_back(r, m, T, nrec, lit, rgb || tex_tape));
        if (rgb) HIP_TRY(hipMemcpyAsync(rgb, r->image.p, 3 * npo * sizeof(float), hipMemcpyDeviceToHost, r->stream));
        if (depth) HIP_TRY(hipMemcpyAsync(depth, r->depth_image.p, npo * sizeof(float), hipMemcpyDeviceToHost, r->stream));
        if (alpha) HIP_TRY(hipMemcpyAsync(alpha, r->alpha_image.p, npo * sizeof(float), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));
        const size_t need = (size_t)std::max(*r->h_total, 0);
        if (need <= m->tile_list.n) {
            if (tape) { tp->mem.pix = F.pix.p; tp->mem.frec = F.frec.p; tp->mem.light = F.light.p; }
            if (geo_tape) {
                HIP_TRY(tp->verts.alloc_pooled(nv3)); HIP_TRY(tp->pv.alloc_pooled(nv3));
                tp->mem.verts = tp->verts.p; tp->mem.pv = tp->pv.p;
                if (tp->has_rgb) {
                    HIP_TRY(tp->rgbmap.alloc_pooled(npx * 3));
                    tp->mem.rgbmap = tp->rgbmap.p;
                    if (tp->lit && tp->light.directional != 0.f) { HIP_TRY(tp->unlit.alloc_pooled(npx * 3)); tp->mem.unlit = tp->unlit.p; }
                }
                BF_TRY(nr_keep_geometry(r, m, tp.get(), T));
                HIP_TRY(hipStreamSynchronize(r->stream));
            }
            if (tape) *tape = tp.release();
            return BF_OK;
        }
        m->tile_list.release();
        HIP_TRY(m->tile_list.alloc(need + need / 2 + 1024));
    }
    return fail(BF_ERR_HIP, "bf_nr_render: the tile lists keep overflowing");
}

int bf_nr_tape_layout(int is, int nrec, int nv, int lit, int flags, int has_rgb, int directional, uint64_t out[17]) {
    BfNrTapeLayout L;
    if (!out || !bf_nr_tape_layout_of(is, nrec, nv, lit != 0, flags, has_rgb != 0, directional != 0, &L))
        return fail(BF_ERR_INVALID, "bf_nr_tape_layout: bad argument");
    for (int k = 0; k < BF_NR_SEG_COUNT; ++k) { out[k] = L.off[k]; out[BF_NR_SEG_COUNT + k] = L.size[k]; }
    out[2 * BF_NR_SEG_COUNT] = L.total;
    return BF_OK;
}

int bf_nr_route_stats(int64_t out[3]) {
    if (!out) return fail(BF_ERR_INVALID, "bf_nr_route_stats: bad argument");
    const NrRouteStats &S = nr_route_stats();
    out[0] = S.renders; out[1] = S.growths; out[2] = S.bytes_back;
    return BF_OK;
}

int bf_nr_render_dev(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                     float *rgb, float *depth, float *alpha, int tape_flags, bf_nr_tape **tape, const float *verts, const float *textures,
                     const bf_nr_camera_dev *cam, float *tape_storage, size_t tape_floats, bf_workspace *ws, void *stream_) {
    if (tape) *tape = nullptr;
    const float *dK = cam ? cam->K : nullptr, *dR = cam ? cam->R : nullptr, *dt = cam ? cam->t : nullptr;
    BF_TRY(nr_render_check(r, m, K || dK, R || dR, t || dt, orig_size, ndc, tape, tape_flags));
    const bool tex_tape = tape && (tape_flags & BF_NR_TAPE_TEXTURES), geo_tape = tape && (tape_flags & BF_NR_TAPE_GEOMETRY);
    if ((rgb || tex_tape) && (!m->ts || !textures)) return fail(BF_ERR_INVALID, "bf_nr_render: rgb or a tape asked of a mesh without textures");
    BF_TRY(bf_ml_dev_check("bf_nr_render_dev", ws, r->device));
    if (!verts) return fail(BF_ERR_INVALID, "bf_nr_render_dev: null vertex pointer");
    if (!ndc && ((K && dK) || (R && dR) || (t && dt))) return fail(BF_ERR_INVALID, "bf_nr_render_dev: K, R and t each come by value or by address, not both");
    const int nrec = fill_back ? 2 * m->nf : m->nf;
    const bool lit = !lightoff && (rgb || tex_tape);
    BfNrTapeLayout L;
    if (!bf_nr_tape_layout_of(r->is, nrec, m->nv, lit, tape ? tape_flags : 0, rgb != nullptr, r->light.directional != 0.f, &L))
        return fail(BF_ERR_INVALID, "bf_nr_render_dev: no tape layout for these sizes");
    if (tape && (!tape_storage || tape_floats < L.total)) return fail(BF_ERR_INVALID, "bf_nr_render_dev: a tape needs tape_storage of bf_nr_tape_layout's total");
    ++bf_route_stats().dev;
    ++nr_route_stats().renders;
    const hipStream_t stream = (hipStream_t)stream_;
    BfRouteCall c(ws, stream);
    BF_TRY(c.begin(r->device));
    NrDevEnd end{r, stream};
    TexView V{};
    V.orig = -1.f;
    if (!ndc) {
        if (R) std::memcpy(V.R, R, sizeof V.R);
        if (t) std::memcpy(V.t, t, sizeof V.t);
        if (K) std::memcpy(V.K, K, sizeof V.K);
        V.orig = orig_size;
    } else {
        dK = dR = dt = nullptr;
    }
    float *base = tape_storage;
    if (!tape) BF_TRY(c.scratch(L.total, base));
    auto seg = [&](int k) { return L.size[k] ? base + L.off[k] : (float *)nullptr; };
    TexView *d_view = (TexView *)seg(BF_NR_SEG_VIEW);
    std::unique_ptr<bf_nr_tape> tp;
    if (tape) {
        tp = nr_new_tape(r, m, nrec, lit, tape_flags, ndc, rgb != nullptr, depth != nullptr, alpha != nullptr, V);
        tp->borrowed = true;
        tp->mem.pix = seg(BF_NR_SEG_PIX); tp->mem.frec = seg(BF_NR_SEG_FREC); tp->mem.light = seg(BF_NR_SEG_LIGHT);
        tp->mem.verts = seg(BF_NR_SEG_VERTS); tp->mem.pv = seg(BF_NR_SEG_PV); tp->mem.rgbmap = seg(BF_NR_SEG_RGBMAP); tp->mem.unlit = seg(BF_NR_SEG_UNLIT);
        tp->mem.d_view = d_view;
    }
    const NrTarget T{stream, verts, textures, seg(BF_NR_SEG_PIX), seg(BF_NR_SEG_FREC), seg(BF_NR_SEG_LIGHT), d_view, rgb, depth, alpha};
    hipLaunchKernelGGL(bf_tex_view_pack_kernel, dim3(1), dim3(64), 0, stream, dK, dR, dt, V, d_view);
    BF_TRY(nr_render_front(r, m, T, V, nrec, lit));
    // the one wait of this route: for the event behind projection + count + scan + 4 bytes, not for the stream's later work
    HIP_TRY(hipEventRecord(r->ev_total, stream));
    HIP_TRY(hipEventSynchronize(r->ev_total));
    nr_route_stats().bytes_back += (long long)sizeof(int);
    const size_t need = (size_t)std::max(*r->h_total, 0);
    if (need > m->tile_list.n) {
        // bf_grow's rule: replaced once nothing uses it - `stream` has just drained up to here, and work of other streams on this
        // renderer was put in front of this call (BfRouteCall::begin; a host-route call ends drained)
        m->tile_list.release();
        HIP_TRY(m->tile_list.alloc(need + need / 2 + 1024));
        ++nr_route_stats().growths;
    }
    BF_TRY(nr_render_back(r, m, T, nrec, lit, rgb || tex_tape));
    if (geo_tape) BF_TRY(nr_keep_geometry(r, m, tp.get(), T));
    BF_TRY(c.finish());
    if (tape) *tape = tp.release();
    return BF_OK;
}

int bf_nr_tape_texture_grad(bf_nr_tape *tape, const float *grad_rgb, float *grad_textures) {
    if (!tape || !grad_rgb || !grad_textures) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: null argument");
    if (!(tape->flags & BF_NR_TAPE_TEXTURES)) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: the tape was made without BF_NR_TAPE_TEXTURES");
    if (tape->borrowed) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: a tape of bf_nr_render_dev takes bf_nr_tape_texture_grad_dev");
    bf_nr *r = nr_find(tape->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: the tape outlived its renderer");
    ++bf_route_stats().host;
    HIP_TRY(hipSetDevice(r->device));
    BF_TRY(nr_join_dev(r));
    const size_t ntex = (size_t)tape->nf * tape->ts * tape->ts * tape->ts * 3;
    DevBuf<float> grad;
    HIP_TRY(grad.alloc_pooled(ntex));
    HIP_TRY(hipMemcpyAsync(r->grad_image.p, grad_rgb, r->grad_image.n * sizeof(float), hipMemcpyHostToDevice, r->stream));
    BF_TRY(nr_texture_grad_issue(r, tape, r->stream, r->grad_image.p, grad.p));
    HIP_TRY(hipMemcpyAsync(grad_textures, grad.p, ntex * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return BF_OK;
}

int bf_nr_tape_texture_grad_dev(bf_nr_tape *tape, const float *grad_rgb, float *grad_textures, bf_workspace *ws, void *stream_) {
    if (!tape || !grad_rgb || !grad_textures) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: null argument");
    if (!(tape->flags & BF_NR_TAPE_TEXTURES)) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: the tape was made without BF_NR_TAPE_TEXTURES");
    if (!tape->borrowed) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad_dev: the tape was not made by bf_nr_render_dev");
    bf_nr *r = nr_find(tape->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: the tape outlived its renderer");
    BF_TRY(bf_ml_dev_check("bf_nr_tape_texture_grad_dev", ws, r->device));
    ++bf_route_stats().dev;
    const hipStream_t stream = (hipStream_t)stream_;
    BfRouteCall c(ws, stream);
    BF_TRY(c.begin(r->device));
    NrDevEnd end{r, stream};
    BF_TRY(nr_texture_grad_issue(r, tape, stream, grad_rgb, grad_textures));
    return c.finish();
}

int bf_nr_tape_vertex_grad(bf_nr_tape *tape, const float *grad_rgb, const float *grad_depth, const float *grad_alpha, float *grad_verts, float *grad_R,
                           float *grad_t) {
    BF_TRY(nr_vertex_grad_check(tape, grad_rgb, grad_depth, grad_alpha, grad_verts, grad_R || grad_t));
    if (tape->borrowed) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: a tape of bf_nr_render_dev takes bf_nr_tape_vertex_grad_dev");
    bf_nr *r = nr_find(tape->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: the tape outlived its renderer");
    ++bf_route_stats().host;
    HIP_TRY(hipSetDevice(r->device));
    BF_TRY(nr_join_dev(r));
    const size_t npo = (size_t)r->out * r->out, nrec9 = (size_t)tape->nrec * 9, nv3 = (size_t)tape->nv * 3;
    const int blocks = (tape->nv + 255) / 256;
    const bool light_vjp = grad_rgb && tape->mem.unlit;
    DevBuf<float> g_rgb, g_depth, g_alpha, grad_frec, grad_lrec, gv, partial, sums;
    if (grad_rgb) HIP_TRY(g_rgb.alloc_pooled(npo * 3));
    if (grad_depth) HIP_TRY(g_depth.alloc_pooled(npo));
    if (grad_alpha) HIP_TRY(g_alpha.alloc_pooled(npo));
    HIP_TRY(grad_frec.alloc_pooled(nrec9));
    if (light_vjp) HIP_TRY(grad_lrec.alloc_pooled(nrec9));
    HIP_TRY(gv.alloc_pooled(nv3));
    if (!tape->ndc) { HIP_TRY(partial.alloc_pooled((size_t)blocks * 12)); HIP_TRY(sums.alloc_pooled(12)); }
    if (grad_rgb) HIP_TRY(hipMemcpyAsync(g_rgb.p, grad_rgb, npo * 3 * sizeof(float), hipMemcpyHostToDevice, r->stream));
    if (grad_depth) HIP_TRY(hipMemcpyAsync(g_depth.p, grad_depth, npo * sizeof(float), hipMemcpyHostToDevice, r->stream));
    if (grad_alpha) HIP_TRY(hipMemcpyAsync(g_alpha.p, grad_alpha, npo * sizeof(float), hipMemcpyHostToDevice, r->stream));
    const NrGradIo io{r->stream, grad_rgb ? g_rgb.p : nullptr, grad_depth ? g_depth.p : nullptr, grad_alpha ? g_alpha.p : nullptr, grad_frec.p,
                      light_vjp ? grad_lrec.p : nullptr, gv.p, tape->ndc ? nullptr : partial.p, sums.p, sums.p ? sums.p + 9 : nullptr};
    BF_TRY(nr_vertex_grad_issue(r, tape, io));
    float cam[12] = {};
    if (!tape->ndc) HIP_TRY(hipMemcpyAsync(cam, sums.p, sizeof cam, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipMemcpyAsync(grad_verts, gv.p, nv3 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (grad_R) std::memcpy(grad_R, cam, 9 * sizeof(float));
    if (grad_t) std::memcpy(grad_t, cam + 9, 3 * sizeof(float));
    return BF_OK;
}

int bf_nr_tape_vertex_grad_dev(bf_nr_tape *tape, const float *grad_rgb, const float *grad_depth, const float *grad_alpha, float *grad_verts, float *grad_R,
                               float *grad_t, bf_workspace *ws, void *stream_) {
    BF_TRY(nr_vertex_grad_check(tape, grad_rgb, grad_depth, grad_alpha, grad_verts, grad_R || grad_t));
    if (!tape->borrowed) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad_dev: the tape was not made by bf_nr_render_dev");
    bf_nr *r = nr_find(tape->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: the tape outlived its renderer");
    BF_TRY(bf_ml_dev_check("bf_nr_tape_vertex_grad_dev", ws, r->device));
    ++bf_route_stats().dev;
    const hipStream_t stream = (hipStream_t)stream_;
    BfRouteCall c(ws, stream);
    BF_TRY(c.begin(r->device));
    NrDevEnd end{r, stream};
    const bool light_vjp = grad_rgb && tape->mem.unlit;
    NrGradIo io{stream, grad_rgb, grad_depth, grad_alpha, nullptr, nullptr, grad_verts, nullptr, grad_R, grad_t};
    BF_TRY(c.scratch((size_t)tape->nrec * 9, io.grad_frec));
    if (light_vjp) BF_TRY(c.scratch((size_t)tape->nrec * 9, io.grad_lrec));
    if (grad_R || grad_t) BF_TRY(c.scratch((size_t)((tape->nv + 255) / 256) * 12, io.partial));
    BF_TRY(nr_vertex_grad_issue(r, tape, io));
    return c.finish();
}

}  // extern "C"
