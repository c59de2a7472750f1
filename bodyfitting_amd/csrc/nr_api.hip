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

#include <climits>

struct bf_nr {
    unsigned long long id = 0;        // never reused: meshes and tapes name their renderer by it (bf_nr_live)
    int device = 0, out = 0, is = 0, tiles = 0, aa = 1;
    float near = 0.1f, far = 100.f, bg[3] = {0.f, 0.f, 0.f};
    NrLight light{0.5f, 0.5f, {1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}, {0.f, 1.f, 0.f}, 1};      // renderer.py:17-19
    hipStream_t stream = nullptr;
    DevBuf<float> rgb, image, depth_image, alpha_image, grad_image;
    DevBuf<int> tile_start, cursor;
    int *h_total = nullptr;           // pinned: the number of tile-list entries the last render needed
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
};

static std::mutex &nr_mu() { static std::mutex mu; return mu; }
static std::map<unsigned long long, bf_nr *> &nr_live() { static std::map<unsigned long long, bf_nr *> live; return live; }
static bf_nr *nr_find(unsigned long long id) {
    std::lock_guard<std::mutex> lk(nr_mu());
    auto it = nr_live().find(id);
    return it == nr_live().end() ? nullptr : it->second;
}

// one attempt: everything up to the host copies, on the renderer's stream.  F: where pix / frec / light go.
static int nr_render_once(bf_nr *r, bf_nr_mesh *M, NrFrame &F, const TexView &V, int nrec, bool lit, bool want_rgb, float *rgb, float *depth,
                          float *alpha) {
    const int is = r->is, tiles = r->tiles, ntile = tiles * tiles, cap = (int)M->tile_list.n;
    NrLight L = r->light;
    L.on = lit ? 1 : 0;
    float *light = lit ? F.light.p : nullptr;
    hipLaunchKernelGGL(bf_tex_project_kernel, dim3((M->nv + 255) / 256), dim3(256), 0, r->stream, M->nv, (const float *)M->verts.p, V, M->pv.p);
    HIP_TRY(hipMemsetAsync(r->tile_start.p, 0, (size_t)(ntile + 1) * sizeof(int), r->stream));
    hipLaunchKernelGGL(bf_nr_face_kernel, dim3((nrec + 255) / 256), dim3(256), 0, r->stream, M->nf, nrec, (const int *)M->topo->faces.p, (const float *)M->pv.p,
                       (const float *)M->verts.p, L, is, tiles, F.frec.p, light, r->tile_start.p, (int *)nullptr, (int *)nullptr, 0, cap);
    hipLaunchKernelGGL(bf_grid_scan_kernel, dim3(1), dim3(1024), 0, r->stream, r->tile_start.p, r->cursor.p, ntile + 1);
    HIP_TRY(hipMemcpyAsync(r->h_total, r->tile_start.p + ntile, sizeof(int), hipMemcpyDeviceToHost, r->stream));
    hipLaunchKernelGGL(bf_nr_face_kernel, dim3((nrec + 255) / 256), dim3(256), 0, r->stream, M->nf, nrec, (const int *)M->topo->faces.p, (const float *)M->pv.p,
                       (const float *)M->verts.p, L, is, tiles, F.frec.p, light, r->tile_start.p, r->cursor.p, M->tile_list.p, 1, cap);
    hipLaunchKernelGGL(bf_nr_raster_kernel, dim3((ntile + 3) / 4), dim3(256), 0, r->stream, is, tiles, M->nf, (const float *)F.frec.p, (const float *)light,
                       (const int *)r->tile_start.p, (const int *)M->tile_list.p, want_rgb ? (const float *)M->tex.p : (const float *)nullptr, M->ts,
                       r->near, r->far, r->bg[0], r->bg[1], r->bg[2], F.pix.p, r->rgb.p, cap);
    const int npo = r->out * r->out;
    if (rgb) {
        hipLaunchKernelGGL(bf_tex_compose_kernel, dim3((3 * npo + 255) / 256), dim3(256), 0, r->stream, r->out, r->aa, (const float *)r->rgb.p, r->image.p);
        HIP_TRY(hipMemcpyAsync(rgb, r->image.p, (size_t)3 * npo * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    }
    if (depth) {
        hipLaunchKernelGGL(bf_tex_depth_kernel, dim3((npo + 255) / 256), dim3(256), 0, r->stream, r->out, r->aa, (const float *)F.pix.p, r->depth_image.p);
        HIP_TRY(hipMemcpyAsync(depth, r->depth_image.p, (size_t)npo * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    }
    if (alpha) {
        hipLaunchKernelGGL(bf_nr_alpha_kernel, dim3((npo + 255) / 256), dim3(256), 0, r->stream, r->out, r->aa, (const float *)F.pix.p, r->alpha_image.p);
        HIP_TRY(hipMemcpyAsync(alpha, r->alpha_image.p, (size_t)npo * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r->stream));
    return BF_OK;
}

// what a geometry tape keeps beside the frame: copies on the renderer's stream of this render's vertices, projected vertices and
// colours, and (lit, with a directional term) the unlit samples from the textures as they are now
static int nr_keep_geometry(bf_nr *r, bf_nr_mesh *M, bf_nr_tape *tp) {
    const size_t nv3 = (size_t)M->nv * 3, npx = (size_t)r->is * r->is;
    tp->topo = M->topo;
    HIP_TRY(tp->verts.alloc_pooled(nv3)); HIP_TRY(tp->pv.alloc_pooled(nv3));
    HIP_TRY(hipMemcpyAsync(tp->verts.p, M->verts.p, nv3 * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(tp->pv.p, M->pv.p, nv3 * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    if (tp->has_rgb) {
        HIP_TRY(tp->rgbmap.alloc_pooled(npx * 3));
        HIP_TRY(hipMemcpyAsync(tp->rgbmap.p, r->rgb.p, npx * 3 * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
        if (tp->lit && tp->light.directional != 0.f) {
            HIP_TRY(tp->unlit.alloc_pooled(npx * 3));
            hipLaunchKernelGGL(bf_nr_unlit_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, r->stream, r->is, M->nf, (const float *)tp->frame.pix.p,
                               (const float *)tp->frame.frec.p, (const float *)M->tex.p, M->ts, tp->unlit.p);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(r->stream));
    return BF_OK;
}

extern "C" {

void bf_nr_destroy(bf_nr *r) {
    if (!r) return;
    { std::lock_guard<std::mutex> lk(nr_mu()); nr_live().erase(r->id); }
    (void)hipSetDevice(r->device);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->h_total) (void)hipHostFree(r->h_total);
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
                    r->cursor.alloc(ntile + 1) == hipSuccess && hipHostMalloc((void **)&r->h_total, sizeof(int)) == hipSuccess;
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
    if (bf_nr *r = nr_find(m->owner)) (void)hipStreamSynchronize(r->stream);
    delete m;
}

int bf_nr_mesh_set_textures(bf_nr_mesh *m, const float *textures) {
    if (!m || !textures) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_textures: null argument");
    if (!m->ts) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_textures: the mesh was created without a texture size");
    bf_nr *r = nr_find(m->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_mesh_set_textures: the mesh's renderer was destroyed");
    HIP_TRY(hipSetDevice(m->device));
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
    (void)hipSetDevice(tape->device);
    if (bf_nr *r = nr_find(tape->owner)) (void)hipStreamSynchronize(r->stream);      // (the pool hands the blocks out again: nothing may still read them)
    delete tape;
}

int bf_nr_render(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                 float *rgb, float *depth, float *alpha, bf_nr_tape **tape) {
    return bf_nr_render_taped(r, m, K, R, t, orig_size, fill_back, lightoff, ndc, rgb, depth, alpha, BF_NR_TAPE_TEXTURES, tape);
}

int bf_nr_render_taped(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                       float *rgb, float *depth, float *alpha, int tape_flags, bf_nr_tape **tape) {
    if (tape) *tape = nullptr;
    if (!r || !m) return fail(BF_ERR_INVALID, "bf_nr_render: null handle");
    if (tape && (!tape_flags || (tape_flags & ~(BF_NR_TAPE_TEXTURES | BF_NR_TAPE_GEOMETRY))))
        return fail(BF_ERR_INVALID, "bf_nr_render_taped: tape_flags must be a non-empty set of BF_NR_TAPE_TEXTURES | BF_NR_TAPE_GEOMETRY");
    const bool tex_tape = tape && (tape_flags & BF_NR_TAPE_TEXTURES), geo_tape = tape && (tape_flags & BF_NR_TAPE_GEOMETRY);
    if (m->owner != r->id) return fail(BF_ERR_INVALID, "bf_nr_render: the mesh belongs to another renderer");
    if (!ndc && (!K || !R || !t || !(orig_size > 0.f))) return fail(BF_ERR_INVALID, "bf_nr_render: K, R, t and a positive orig_size are needed unless ndc is set");
    if ((rgb || tex_tape) && !m->has_tex) return fail(BF_ERR_INVALID, "bf_nr_render: rgb or a tape asked of a mesh without textures");
    HIP_TRY(hipSetDevice(r->device));
    TexView V{};
    V.orig = -1.f;                                    // (bf_tex_project_kernel: pass the vertices through)
    if (!ndc) { std::memcpy(V.R, R, sizeof V.R); std::memcpy(V.t, t, sizeof V.t); std::memcpy(V.K, K, sizeof V.K); V.orig = orig_size; }
    const int nrec = fill_back ? 2 * m->nf : m->nf;
    const bool lit = !lightoff && (rgb || tex_tape);
    const size_t npx = (size_t)r->is * r->is;
    std::unique_ptr<bf_nr_tape> tp;
    NrFrame scratch;
    if (tape) {
        tp.reset(new bf_nr_tape());
        tp->owner = r->id; tp->device = r->device; tp->nf = m->nf; tp->nrec = nrec; tp->ts = m->ts; tp->lit = lit;
        tp->flags = tape_flags; tp->nv = m->nv; tp->ndc = ndc ? 1 : 0;
        tp->has_rgb = rgb != nullptr; tp->has_depth = depth != nullptr; tp->has_alpha = alpha != nullptr;
        tp->view = V; tp->light = r->light; tp->light.on = lit ? 1 : 0;
    }
    NrFrame &F = tape ? tp->frame : scratch;
    BF_TRY(F.alloc(npx, (size_t)nrec, lit));
    for (int attempt = 0; attempt < 3; ++attempt) {
        BF_TRY(nr_render_once(r, m, F, V, nrec, lit, rgb || tex_tape, rgb, depth, alpha));
        const size_t need = (size_t)std::max(*r->h_total, 0);
        if (need <= m->tile_list.n) {
            if (geo_tape) BF_TRY(nr_keep_geometry(r, m, tp.get()));
            if (tape) *tape = tp.release();
            return BF_OK;
        }
        m->tile_list.release();
        HIP_TRY(m->tile_list.alloc(need + need / 2 + 1024));
    }
    return fail(BF_ERR_HIP, "bf_nr_render: the tile lists keep overflowing");
}

int bf_nr_tape_texture_grad(bf_nr_tape *tape, const float *grad_rgb, float *grad_textures) {
    if (!tape || !grad_rgb || !grad_textures) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: null argument");
    if (!(tape->flags & BF_NR_TAPE_TEXTURES)) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: the tape was made without BF_NR_TAPE_TEXTURES");
    bf_nr *r = nr_find(tape->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_tape_texture_grad: the tape outlived its renderer");
    HIP_TRY(hipSetDevice(r->device));
    const int ts = tape->ts;
    const size_t ntex = (size_t)tape->nf * ts * ts * ts * 3;
    DevBuf<float> grad;
    HIP_TRY(grad.alloc_pooled(ntex));
    const float *light = tape->lit ? tape->frame.light.p : nullptr;
    HIP_TRY(hipMemcpyAsync(r->grad_image.p, grad_rgb, r->grad_image.n * sizeof(float), hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(bf_nr_backward_kernel, dim3(tape->nf), dim3(64), (size_t)ts * ts * ts * 3 * sizeof(float), r->stream, tape->nf, tape->nrec, r->is,
                       r->out, r->aa, (const float *)tape->frame.pix.p, (const float *)tape->frame.frec.p, light, ts, (const float *)r->grad_image.p, grad.p);
    hipLaunchKernelGGL(bf_nr_backward_large_kernel, dim3((r->is * r->is + 255) / 256), dim3(256), 0, r->stream, tape->nf, r->is, r->out, r->aa,
                       (const float *)tape->frame.pix.p, (const float *)tape->frame.frec.p, light, ts, (const float *)r->grad_image.p, grad.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grad_textures, grad.p, ntex * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return BF_OK;
}

int bf_nr_tape_vertex_grad(bf_nr_tape *tape, const float *grad_rgb, const float *grad_depth, const float *grad_alpha, float *grad_verts, float *grad_R,
                           float *grad_t) {
    if (!tape || !grad_verts) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: null argument");
    if (!(tape->flags & BF_NR_TAPE_GEOMETRY)) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: the tape was made without BF_NR_TAPE_GEOMETRY");
    if ((grad_rgb && !tape->has_rgb) || (grad_depth && !tape->has_depth) || (grad_alpha && !tape->has_alpha))
        return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: a cotangent for an output the render did not produce");
    if (tape->ndc && (grad_R || grad_t)) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: an ndc render has no R or t");
    bf_nr *r = nr_find(tape->owner);
    if (!r) return fail(BF_ERR_INVALID, "bf_nr_tape_vertex_grad: the tape outlived its renderer");
    HIP_TRY(hipSetDevice(r->device));
    const size_t npo = (size_t)r->out * r->out, nrec9 = (size_t)tape->nrec * 9, nv3 = (size_t)tape->nv * 3;
    const int blocks = (tape->nv + 255) / 256;
    const bool light_vjp = grad_rgb && tape->unlit.p;
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
    NrGeo G{};
    G.faces = tape->topo->faces.p; G.pv = tape->pv.p; G.verts = tape->verts.p; G.pix = tape->frame.pix.p; G.frec = tape->frame.frec.p;
    G.rgbmap = tape->rgbmap.p; G.unlit = tape->unlit.p;
    G.g_rgb = grad_rgb ? g_rgb.p : nullptr; G.g_depth = grad_depth ? g_depth.p : nullptr; G.g_alpha = grad_alpha ? g_alpha.p : nullptr;
    G.nf = tape->nf; G.nrec = tape->nrec; G.is = r->is; G.out = r->out; G.aa = r->aa;
    float *lrec = light_vjp ? grad_lrec.p : nullptr;
    hipLaunchKernelGGL(bf_nr_geometry_kernel, dim3(tape->nrec), dim3(64), 0, r->stream, G, tape->light, grad_frec.p, lrec);
    hipLaunchKernelGGL(bf_nr_fold_kernel, dim3(blocks), dim3(256), 0, r->stream, tape->nv, tape->nrec, (const int *)tape->topo->vstart.p,
                       (const int *)tape->topo->ventry.p, (const float *)grad_frec.p, (const float *)lrec, (const float *)tape->verts.p, tape->view, gv.p,
                       tape->ndc ? (float *)nullptr : partial.p);
    float cam[12] = {};
    if (!tape->ndc) {
        hipLaunchKernelGGL(bf_nr_fold_sum_kernel, dim3(1), dim3(64), 0, r->stream, blocks, (const float *)partial.p, sums.p);
        HIP_TRY(hipMemcpyAsync(cam, sums.p, sizeof cam, hipMemcpyDeviceToHost, r->stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(grad_verts, gv.p, nv3 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (grad_R) std::memcpy(grad_R, cam, 9 * sizeof(float));
    if (grad_t) std::memcpy(grad_t, cam + 9, 3 * sizeof(float));
    return BF_OK;
}

}  // extern "C"
