// Host-side private definitions shared by the host files (*_api.hip, api.hip, lanes.hip, group.hip).
#pragma once
#include "../../include/bodyfit.h"
#include "bf_internal.h"
#include "lane_slots.h"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

std::string &bf_err_slot();
int bf_fail(int code, const std::string &msg);
#define fail bf_fail

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(BF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)
// a call of this library that has already said why it failed: pass its code on
#define BF_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)

// hipMemset of device memory returns before the fill has run, and the fill is on the NULL stream: work enqueued afterwards on a
// non-blocking stream (every stream of this library) is not ordered behind it.  Fills that are not stream-ordered wait here.
inline hipError_t bf_memset_sync(void *p, int value, size_t bytes) {
    hipError_t e = hipMemset(p, value, bytes);
    return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}
// A cache of freed device blocks per device (bf_pool_alloc / bf_pool_free), for objects that come and go with every frame of a
// capture: a scan is created, attached, fitted against and destroyed once per frame (apps/genebody_fitting.py:183-192), and every
// hipFree waits for the whole device - i.e. for the fit of the PREVIOUS frame that is still running - while a hipMalloc of a fresh
// block costs tens of microseconds.  A block is handed out again for a request of its size up to 25 % smaller (and comes back under its true size); the
// cache holds at most 2 GB per device (beyond that a block is really freed), gives everything back when a hipMalloc fails, and
// bf_pool_trim() empties it.  The caller guarantees what hipFree used to: nothing on the device
// still uses a block it gives back (bf_scan_destroy waits for the device itself when the scan is still attached to a batch, and detaches it).
struct BfPool {
    std::mutex mu;
    std::multimap<size_t, void *> blocks[16];
    size_t held[16] = {0};
};
inline BfPool &bf_pool() { static BfPool P; return P; }
// every cached block of a device goes back to the runtime (device idle or not: hipFree waits); -> bytes released
inline size_t bf_pool_trim(int dev) {
    std::vector<void *> drop;
    size_t bytes = 0;
    if (dev >= 0 && dev < 16) {
        BfPool &P = bf_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        for (auto &kv : P.blocks[dev]) drop.push_back(kv.second);
        bytes = P.held[dev];
        P.blocks[dev].clear();
        P.held[dev] = 0;
    }
    for (void *q : drop) (void)hipFree(q);
    return bytes;
}
// `*got` = the size of the block handed out (>= bytes): what bf_pool_free must be told, so that the cache's accounting holds
inline hipError_t bf_pool_alloc(void **p, size_t bytes, size_t *got) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    bytes = (bytes + 255) & ~(size_t)255;
    *got = bytes;
    if (dev >= 0 && dev < 16) {
        BfPool &P = bf_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.blocks[dev].lower_bound(bytes);
        if (it != P.blocks[dev].end() && it->first <= bytes + bytes / 4 + 4096) {
            *p = it->second;
            *got = it->first;
            P.held[dev] -= it->first;
            P.blocks[dev].erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess && bf_pool_trim(dev) > 0) {          // the cache itself may be what exhausted the device: give it back, once
        (void)hipGetLastError();
        e = hipMalloc(p, bytes);
    }
    return e;
}
// `bytes`: the block's size as bf_pool_alloc reported it
inline void bf_pool_free(void *p, size_t bytes, int dev) {
    if (!p) return;
    bytes = (bytes + 255) & ~(size_t)255;
    if (dev >= 0 && dev < 16) {
        BfPool &P = bf_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        if (P.held[dev] + bytes <= ((size_t)2 << 30)) { P.blocks[dev].emplace(bytes, p); P.held[dev] += bytes; return; }
    }
    (void)hipFree(p);
}
inline int bf_alloc_index() { static std::atomic<int> counter{0}; return counter++; }      // (of this translation unit's allocations, all types; bf_group's workers allocate side by side)
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    bool view = false;          // a slice of another allocation: not freed here
    int pool_dev = -1;          // >= 0: the block came from (and goes back to) bf_pool of that device
    size_t pool_bytes = 0;
    void slice(T *base, size_t count) { p = base; n = count; view = true; }
    hipError_t alloc_pooled(size_t count) {       // for buffers of per-frame objects (see BfPool); contents undefined
        n = count;
        (void)hipGetDevice(&pool_dev);
        return bf_pool_alloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T), &pool_bytes);
    }
    hipError_t upload_pooled(const T *h, size_t count) {
        hipError_t e = alloc_pooled(count);
        if (e != hipSuccess) return e;
        return count == 0 ? hipSuccess : hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t alloc(size_t count) {
        n = count;
        hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
        // BF_POISON=<byte>: fill every fresh allocation with that byte (255: NaNs) - a read of memory nobody wrote shows up in the
        // results instead of depending on what the allocator hands out (bring-up switch)
        // (BF_POISON_ONLY=<k>: only the k-th allocation of the process; BF_POISON_LOG=1 lists them on stderr)
        static const int poison = [] { const char *v = std::getenv("BF_POISON"); return v ? std::atoi(v) : -1; }();
        static const int only = [] { const char *v = std::getenv("BF_POISON_ONLY"); return v ? std::atoi(v) : -1; }();
        static const bool log = std::getenv("BF_POISON_LOG") != nullptr;
        const int k = bf_alloc_index();
        if (log) std::fprintf(stderr, "alloc %d: %zu x %zu bytes\n", k, count, sizeof(T));
        if (e == hipSuccess && poison >= 0 && (only < 0 || only == k)) {
            e = bf_memset_sync(p, poison, std::max<size_t>(count, 1) * sizeof(T));
        }
        return e;
    }
    hipError_t upload(const T *h, size_t count) {
        hipError_t e = alloc(count);
        if (e != hipSuccess) return e;
        return count == 0 ? hipSuccess : hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> &h) { return upload(h.data(), h.size()); }
    void drop() { if (p && !view) { if (pool_dev >= 0) bf_pool_free(p, pool_bytes, pool_dev); else (void)hipFree(p); } }
    void release() { drop(); p = nullptr; n = 0; view = false; pool_dev = -1; }
    ~DevBuf() { drop(); }
};

// A grow-only buffer used on one stream: replaced by a larger one once that stream has drained (nothing else uses it); contents undefined
template <typename T>
hipError_t bf_grow(hipStream_t s, DevBuf<T> &b, size_t count) {
    if (b.n >= count && b.p) return hipSuccess;
    if (b.p) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
    }
    b.release();
    return b.alloc(count);
}

// bf_dev_route_stats: calls of the host entry points a torch loop goes through (bf_smpl_forward, bf_smpl_vjp, bf_smplx_forward[_expr],
// bf_smplx_vjp[_expr], bf_keypoint_loss, the SMPL+D stage's losses of mesh_loss_api.hip, bf_scan_nearest, bf_silhouette_loss, the renderer's bf_nr_render[_taped] and bf_nr_tape_*_grad), calls of their *_dev twins, device (re)allocations of workspaces, and calls that had to wait
// for their workspace's previous call on another stream.  Process-wide; counted once the arguments have passed.
struct BfRouteStats { std::atomic<long long> host{0}, dev{0}, allocs{0}, switches{0}; };
inline BfRouteStats &bf_route_stats() { static BfRouteStats S; return S; }

// vertex -> (face, corner) lists in the order compute_normal_torch (io_utils.py:406-428) adds a vertex's face normals up: corner by
// corner, faces ascending.  start[nv + 1] = CSR offsets, adj[3 nf] = face * 4 + corner.  `faces` holds 3 nf indices inside [0, nv).
// Shared by the SMPL+D stage (bf_fit_displacement) and bf_topo_create, through BfTopoDev below.
inline void bf_build_vertex_adjacency(const std::vector<int> &faces, int nv, std::vector<int> &start, std::vector<int> &adj) {
    const int nf = (int)(faces.size() / 3);
    start.assign((size_t)nv + 1, 0);
    adj.assign(faces.size(), 0);
    for (int v : faces) ++start[v + 1];
    for (int v = 0; v < nv; ++v) start[v + 1] += start[v];
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int c = 0; c < 3; ++c)
        for (int f = 0; f < nf; ++f) adj[fill[faces[f * 3 + c]]++] = f * 4 + c;
}

// A mesh's topology on the device: its faces and the lists above.  build() uploads on the current device (blocking); faces last: it
// is the "built" flag of a record built on first use (bf_model's, under `lazy`)
struct BfTopoDev {
    DevBuf<int> faces, adj_start, adj;
    bool built() const { return faces.p != nullptr; }
    hipError_t build(const std::vector<int> &faces_host, int nv) {
        std::vector<int> start, list;
        bf_build_vertex_adjacency(faces_host, nv, start, list);
        hipError_t e = adj_start.upload(start);
        if (e == hipSuccess) e = adj.upload(list);
        return e == hipSuccess ? faces.upload(faces_host) : e;
    }
};

// Scratch of the MFMA batch path of the full-mesh forward (>= BF_MFMA_MIN_FRAMES frames).  Owned by whoever owns the stream
// the forward runs on (a bf_batch, or a one-off forward call): two batches of one model never share it.
struct MeshScratch {
    DevBuf<float> pose_off;       // [F][3NV] batched pose-blend result, grown on demand
    DevBuf<float> featT;          // [K padded][F padded] pose features of a batch, frame-minor (the GEMM's A operand)
};

// What an arena of either kind is made of: a device buffer and a pinned host buffer of the same size, both zero-filled.
inline hipError_t bf_alloc_mirrored(DevBuf<float> &dev, float **host, size_t n_floats) {
    hipError_t e = dev.alloc(n_floats);
    if (e == hipSuccess) e = bf_memset_sync(dev.p, 0, n_floats * sizeof(float));
    if (e == hipSuccess) e = hipHostMalloc((void **)host, n_floats * sizeof(float));
    if (e == hipSuccess) std::memset(*host, 0, n_floats * sizeof(float));
    return e;
}

// A result arena: ONE device buffer [params | terms | state | joints | vout] (the batch's layout: res_off / res_cnt) mirrored by ONE
// pinned host buffer, so a fetch is a single device-to-host copy of the prefix that is wanted.  A batch has two - a fresh fit
// (BF_FIT_RESET + FETCH, pipelined or frame after frame) writes the one the previous fit did not use and its hand-over runs on a second
// stream, under the next fit's kernels - and every fit lane has one.  Whoever owns it waits for its streams before it goes.
struct ResultArena {
    DevBuf<float> dev;
    float *host = nullptr;
    hipEvent_t ev_done = nullptr;   // the fit that fills the arena has finished (a lane's tail follows its fit in stream order: unused there)
    hipEvent_t ev_copied = nullptr; // the arena's last fit, mesh and hand-over have finished
    bool copy_pending = false;      // the hand-over ev_copied stands for has not been waited for yet
    long long seq = -1;             // the fit whose result the arena holds (-1: none)
    bool fetched = false, has_v = false;
    ResultArena() = default;
    ResultArena(const ResultArena &) = delete;
    hipError_t create(size_t n_floats) {
        hipError_t e = bf_alloc_mirrored(dev, &host, n_floats);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_done, hipEventDisableTiming);
        return e == hipSuccess ? hipEventCreateWithFlags(&ev_copied, hipEventDisableTiming) : e;
    }
    // This arena takes `from`'s buffers and what is known of their contents; `from` gets this one's, as holding nothing.  The events and
    // copy_pending stay: they speak of work on their owner's streams (which the caller has waited for), not of the memory.
    void trade_buffers(ResultArena &from) {
        std::swap(dev.p, from.dev.p);
        std::swap(host, from.host);
        seq = from.seq; fetched = from.fetched; has_v = from.has_v;
        from.seq = -1;
        from.fetched = from.has_v = false;
    }
    ~ResultArena() {
        if (ev_done) (void)hipEventDestroy(ev_done);
        if (ev_copied) (void)hipEventDestroy(ev_copied);
        if (host) (void)hipHostFree(host);
    }
};

// An input arena [keypoints | params0 | ndiv] (the batch's layout: in_off / in_total), fed from its own pinned staging buffer by a
// transfer on a stream of its owner.  Two per batch and two per fit lane: the next frame's inputs are packed into the staging buffer
// the fit in flight does not read - the setter never drains a stream (the reference pays 48 keypoint host-to-device copies per
// ITERATION, loss.py:160).
// A fit lane's arena holds the device arrays of up to W calls' frames, array-major like FrameIO ([W F] keypoints | [W F] params0 |
// [W F] ndiv: BfLanes::gin, lane_slots.h), and its pinned buffer has the same layout - slot s of the one mirrors slot s of the other,
// array by array.  A staging packs into the pinned slot and issues nothing; when the group is launched, one transfer on the lane's stream
// moves the prefix of slots that were filled (three contiguous ranges) and `ev` is recorded behind it.  The arena is opened again two of
// its lane's groups later: whoever opens it waits for `ev` on the host if that transfer has not finished.  W = 1 is the batch's own
// layout: one slot, filled by a transfer of its own at every staging (the call sequence before groups).
struct InputArena {
    DevBuf<float> dev;
    float *host = nullptr;          // the device arena's layout
    hipEvent_t ev = nullptr;        // the last transfer out of `host` has finished
    bool pending = false;           // ... and has not been waited for yet
    unsigned readers = 0;           // a lane's arena: the lanes that read the device arrays from outside since they were last filled (bit per lane) -
                                    // W = 1 a fit that read the slot in place, W > 1 a device-side copy of a slot; the next transfer waits for them
    InputArena() = default;
    InputArena(const InputArena &) = delete;
    hipError_t create(size_t n_floats) {
        hipError_t e = bf_alloc_mirrored(dev, &host, n_floats);
        return e == hipSuccess ? hipEventCreateWithFlags(&ev, hipEventDisableTiming) : e;
    }
    ~InputArena() {
        if (ev) (void)hipEventDestroy(ev);
        if (host) (void)hipHostFree(host);
    }
};

// A mask arena: ONE set of what a border-following pass (bf_contour_kernel) reads and writes.  A batch has two (BfMasks): a fit reads
// one while the next frame's silhouettes are staged into the other.  Whoever owns it waits for its streams before it goes.
struct MaskArena {
    unsigned char *h_masks = nullptr;   // pinned: the binarised masks
    int *h_counts = nullptr;            // pinned: [2 * F * M] contour lengths | which half of the slab holds them
    size_t h_masks_n = 0, h_counts_n = 0;
    hipEvent_t ev = nullptr;            // the arena's upload + border following have finished
    hipEvent_t ev_used = nullptr;       // the last fit that read the arena has finished
    DevBuf<unsigned char> masks;
    DevBuf<float> slab;                 // [F*M][2][cap][2] the contour kernel's two-slot slabs
    DevBuf<int> cnt2;
    DevBuf<unsigned> planes;            // bit planes of images too large for LDS
    int select = 0;                     // contour_select of the masks it holds
    MaskArena() = default;
    MaskArena(const MaskArena &) = delete;
    ~MaskArena() {
        for (hipEvent_t e : {ev, ev_used}) if (e) (void)hipEventDestroy(e);
        for (void *h : {(void *)h_masks, (void *)h_counts}) if (h) (void)hipHostFree(h);
    }
};

// A batch's silhouettes (use_mask, smplify.py:138-144,197-199; mask_api.hip).  "The active arena" is arena[cur], "the one staged into"
// arena[cur ^ 1].  Contours followed on the device are DEFERRED: attaching or staging queues the upload and the border following on the
// second stream and returns; what needs their lengths is finished by bf_masks_finalize right before the first kernel that reads them -
// in a fit the first iteration past dense_after, by which time the keypoint-only iterations in front have long covered the following.
//  * Freeing.  Finalize and staging free no device or pinned memory: a fit may be in flight - finalize runs in the middle of one, whose
//    resident launch waits for kernels not enqueued yet, and hipFree waits for the device.  Outgrown device blocks go onto `retired`,
//    emptied by the next bf_batch_set_masks after its bf_sync_all, and with the batch.  What finalize fills is sized at attach.
//  * Attach (bf_batch_set_masks) binarises into the active arena's pinned buffer BEFORE bf_sync_all, having waited for that arena's `ev`
//    alone (in a frame loop the work in flight is the previous fit, and that upload went out early in it), and clears `staged`.
//    n_masks <= 0 or masks NULL switches the term off, after bf_sync_all.
//  * Staging (bf_batch_stage_masks) waits for ev_used and ev of arena[cur ^ 1] and nothing else, and sizes that arena's slab to the shared
//    `cap` - which is how the arena that lags behind a regrow catches up.
//  * Commit flips `cur` (pointers only: the kernels of a fit still in flight hold the old arena's by value); contours pending again.
//  * Finalize waits on the host for arena[cur].ev; follows again, on the copy stream with a stream wait, only when a border outgrew
//    `cap`; queues the count, offset and xy copies on the BATCH stream, in front of the kernels that read them; and reuses the second
//    half of the pinned counts for the offsets.
struct BfMasks {
    bool on = false, pending = false;   // attached; a deferred border following has yet to be finalized
    bool on_device = false;             // the attached masks' contours were followed on the device (contour_count = NULL)
    MaskIO io{};
    MaskArena arena[2];
    int cur = 0;
    bool staged = false;                // arena[cur ^ 1] holds the next fit's silhouettes
    int cap = 0;                        // contour points a slab slot holds: shared by both arenas and the buffers sized by it below
    std::vector<void *> retired;        // outgrown device blocks nobody could free yet
    std::vector<int> view_host;         // the view indices the active masks were set with
    DevBuf<int> view, cstart, ccount, choice;
    DevBuf<float> cxy, uvi, duvb, cgrad, part, loss, gpart;
    DevBuf<unsigned long long> acc;     // [F][M][ns][2] fixed-point contour-gradient sums (MaskIO::acc)
    void free_retired() { for (void *q : retired) (void)hipFree(q); retired.clear(); }
    ~BfMasks() { free_retired(); }
};

struct bf_model {
    int device = 0;
    int nv = 0, nj = 0, nb = 0, npf = 0, ns = 0, nl = 0, np = 0, n_levels = 0;
    int n_selector = 0, n_extra = 0, n_joint_map = 0;
    FitTab fit{};
    MeshTab mesh{};
    size_t mesh_smem = 0;
    DevBuf<float> v_template, shapedirs, posedirs, lbs_weights, j_extra;
    DevBuf<int> selector_ids, joint_map;
    DevBuf<int> depth_d, sel_nzj;
    DevBuf<float> sel_nzw;
    DevBuf<unsigned long long> desc_d;
    DevBuf<int> dfs_order, dfs_last;
    DevBuf<float> g_plane, g_ptail;
    DevBuf<int> parents, level_start, level_joints, child_start, child_list, lj_kind, lj_index;
    DevBuf<float> Jtrel;
    DevBuf<float> Jt, Jd, Jdrel, sel_vt, sel_sd, sel_pd, sel_w, g_means, g_psym, g_logw;
    // SMPL-X pose assembly / parameter routing / landmarks / dense keypoint loss
    int kind = 0, kp_dense = 0, n_lmk = 0, n_all = 0, nl_loss = 0;
    DevBuf<int> th_kind, th_off, p_kind, p_a, p_b, faces_lm, lmk_faces, dyn_faces, kp_jm, cj_start, cj_list, lmk_fv, dyn_fv;
    DevBuf<float> pose_mean, hand_comp, lmk_bary, dyn_bary;
    KpIO kp{};
    DevBuf<int> v_nzj;            // sparse skinning rows (MeshTab::v_nnz)
    DevBuf<float> v_nzw;
    // The sampled-first sub-model: the vertices the dense losses of a fit WITHOUT scans can touch - every 4th vertex (the
    // silhouette loss, loss.py:99) first, then the selector and landmark vertices of the dense keypoint loss - with the model's
    // tables gathered for them.  The loop's forward / reverse mesh passes then stream ~30 % of posedirs; the result mesh after
    // the loop is the full model's.
    struct Sub {
        bool on = false;
        int ns = 0;                   // sampled vertices = the first ns of the sub-model
        MeshTab mesh{};
        KpIO kp{};
        DevBuf<float> v_template, shapedirs, posedirs, lbs_weights, j_extra, v_nzw, posedirsT;
        DevBuf<int> v_nzj, selector_ids, faces, lmk_fv, dyn_fv;
        DevBuf<int> verts;            // [mesh.nv] the full model's vertex of every sub-model vertex
        std::vector<int> verts_host;
    } sub, sub_kp;                // (sub_kp: the keypoint-only sub-model of the iterations before the dense losses switch on - no sampled vertices)
    DevBuf<float> posedirsT;      // [3NV][npf], built on first use of the dense reverse pass (under `lazy`, device-synchronised)
    DevBuf<float> fit_image;      // FitTab::lds_image of the dense-schedule fit instance, built on first use (under `lazy`)
    std::mutex lazy;              // guards the build-on-first-use tables (posedirsT, topo)
    std::vector<int> faces_host;  // body-model topology (for the SMPL+D stage), optional
    BfTopoDev topo;               // faces_host and its vertex -> (face, corner) lists on the device, built on first use
    // SMPL-X extension directions: the expression directions (bf_model_set_expression), or a shape space's directions from the eleventh
    // beta on followed by its expression directions (bf_model_set_shape_space).  n_ext = 0: none attached
    int n_expr = 0;               // expression coefficients of a call
    int nb_total = 0;             // betas of a call (0: nb - no shape space attached)
    int n_ext = 0;                // directions attached = (nb_total - nb) + n_expr: a frame's extension coefficients are [betas[nb:], expression]
    bool ext_wide = false;        // the kernels of shape_ext_kernels.hip serve them (n_ext > BF_EXPR_MAX, or BF_SHAPE_EXT_WIDE=1 at the attachment)
    DevBuf<float> exprT;          // [n_ext][3][nv]: E transposed, a coefficient's component contiguous over the vertices
    DevBuf<float> Jx;             // [nj*3][n_ext]   J_regressor E
    DevBuf<float> extVK;          // (ext_wide) [nv][3][n_ext]: E as it arrives, a vertex component's coefficients contiguous - the wide reverse
    DevBuf<float> JxT;            // (ext_wide) [n_ext][nj*3]: Jx transposed - the wide chain delta
    std::vector<int> jreg_start, jreg_v;   // the J_regressor's non-zero weights per joint (CSR), kept on the host for Jx (SMPL-X-kind models)
    std::vector<float> jreg_w;
};

struct bf_graph_key { int n_iters; uint32_t flags; int arena; bf_hyper h; };     // (arena: the result arena its nodes point at)

// A fit lane (BF_FIT_LANES, lanes.hip): everything a frame-after-frame fit (RESET | FETCH | NOTIME, keypoint-only) and its tail write,
// on a stream of its own, so that consecutive frames' fits run side by side on different CUs.  Successive groups go to successive lanes;
// nothing orders one lane behind another but HIP events.
// A lane launch carries a GROUP of up to W consecutive calls' frames (BF_FIT_LANE_WIDTH): the calls join the lane's open group, slot
// after slot, and one fit launch of G F workgroups, one tail and one hand-over serve all G of them.  Every buffer here is sized for W
// calls; a launched group's result arrays are packed for its G F frames (`held.off`).
struct BfLane {
    hipStream_t stream = nullptr;
    MeshScratch scratch;            // the tail's MFMA mesh path, on this lane's stream only
    DevBuf<float> adam_m, adam_v, vraw, xpart;
    ResultArena arena;              // (its mirror is filled by the tail's hand-over)
    InputArena in[2];               // fed on this lane's stream
    int in_next = 0;                            // arena the next group of this lane fills
    bool need_engage = false;                   // the stream has yet to wait for the batch stream (BfLanes::ev_engage)
    bool busy = false;                          // work was enqueued since the lanes were last drained
    hipEvent_t ev_join = nullptr;               // (W > 1) the lane's last device-side copy of current inputs into a slot has finished
    // the open group: calls that joined and wait for their launch
    bool open = false;                          // a group is open (by a staging or a fit) on input arena open_a
    int open_a = 0, n_open = 0;                 // ... with n_open calls joined
    bool slot_staged = false;                   // slot n_open was staged into: the next call to join finds its inputs there
    bool open_host = false;                     // (W > 1) the open group is host-fed: its slots were packed into the pinned buffer and go to the device
                                                // with the launch's one transfer; else device-fed: each slot was copied on the device when its call joined
    bool borrowed = false;                      // (W = 1) the group's call reads the batch's current inputs in place
    const float *bor_kp = nullptr, *bor_p0 = nullptr;
    const int *bor_ndiv = nullptr;
    long long open_seq0 = -1;                   // the first joined call's fit number
    std::chrono::steady_clock::time_point t_first{};    // ... and when it joined (the idle rule's hold, BF_FIT_LANE_HOLD_US)
    int open_iters = 0;
    HyperDev open_hd{};
    // the launched group the result arena holds (or will, once ev_copied completes): fits seq0 .. seq0 + G - 1, slot after slot
    struct Held { long long seq0 = -1; int G = 0; size_t off[5] = {0, 0, 0, 0, 0}, total = 0; } held;
    ~BfLane() { if (ev_join) (void)hipEventDestroy(ev_join); }
};

// The fit lanes of a batch (lanes.hip; the rest of the library goes through lanes.h): n > 1 gives frame-after-frame fits lanes of their
// own, created on first use.  `on`: lane work may be in flight or a lane holds the newest fit - every entry point that is not a lane fit or
// a staging drains the lanes first (bf_lanes_drain), which hands the last lane fit back to the batch's own buffers.
struct BfLanes {
    int n = 1;                          // lanes = min(BF_FIT_LANES, CUs / frames) (lane_policy.h)
    int W = 1;                          // calls per lane launch at most = min(BF_FIT_LANE_WIDTH, CUs / (lanes x frames))
    BfLaneLayout gin;                   // a lane's input arena: its [W F] keypoints, params0, ndiv arrays (lane_slots.h)
    std::unique_ptr<BfLane[]> lane;
    bool on = false;
    int next = 0, last = -1;            // the lane the next call joins; the lane whose newest group (open or launched) ends with the last lane fit
    DevBuf<float> proj_rep;             // (W > 1) the projection table W times over: FrameIO::proj of a group launch
    bool proj_rep_stale = true;         // ... has yet to be copied from `proj` (new cameras)
    hipEvent_t ev_engage = nullptr;     // recorded on the batch stream when the lanes take over: every lane stream waits for it
    bool called = false;                // a LANE-route call has been issued on this batch,
    std::chrono::steady_clock::time_point t_call{};             // ... the last one then: the feeder is fast while calls follow within H (bf_lanes_fit)
    int launches = 0, calls = 0, max_g = 0;                     // bf_batch_lane_stats
    long long feed_transfers = 0, feed_host_copies = 0, feed_dev_copies = 0, feed_waits = 0;    // bf_batch_lane_feed_stats
};

// Where the current inputs live - what `keypoints`, `params0`, `ndiv` of a batch are views of.  Set together with the views, by
// bf_set_inputs alone.
struct InputCursor {
    bool on_lane = false;           // input arena `arena` of fit lane `lane`; else the batch's own arena `arena`
    int lane = 0, arena = 0, slot = 0;      // slot: (on_lane) the slot of that lane arena the views are on
    bool pinned = false;            // (on_lane, W > 1) the pinned mirror of that slot holds the current inputs: a call without a staging of its own
                                    // copies them on the host.  Cleared by every drain - what follows may write the device slot alone
    bool host = false;              // the views point at the pinned staging buffer itself (BF_STAGE_MODE=zerocopy)
};

struct bf_batch {
    bf_model *m = nullptr;
    int F = 0, V = 0;
    size_t fit_smem = 0;            // dynamic LDS of the fit kernel for THIS batch's view count (the carve depends on V)
    MeshScratch scratch;            // pose_off / featT of the MFMA batch path, used on this batch's stream only
    hipStream_t stream = nullptr;
    static constexpr int kRing = 1024;
    std::vector<hipEvent_t> ring;   // kRing x 4 events: | fit | mesh | joints + fetch |
    int ring_n = 0;                 // calls recorded since the last timing reset
    hipEvent_t *ev = nullptr;       // the triple of the last call
    bool timed = false;
    DevBuf<float> params0;          // parameters of the last set_init / set_params / stage_inputs (a view into the current input arena)
    // Per-frame inputs live in TWO input arenas: bf_batch_stage_inputs fills the one the fit in flight does not read and queues its
    // transfer on the batch stream.  `keypoints`, `ndiv`, `params0` are views into the arena in_at names (one of these, or a lane's).
    InputArena in[2];
    size_t in_off[3] = {0, 0, 0}, in_total = 0;          // float offsets of keypoints, params0, ndiv inside an arena
    InputCursor in_at;
    // Staging ASIDE (round 5): the transfer of the next frame's inputs rides on the second stream, AHEAD of the mesh / hand-over tail of
    // the fit in flight - which is why that tail is enqueued late (`tail_k`: at the next entry point, bf_flush_tail) - so that the batch
    // stream holds fit kernel after fit kernel with nothing in between.  in_aside[k]: arena k's transfer is on the second stream and
    // the fit that reads it must see in[k].ev first; in_reader[k]: sequence number of the last fit that read arena k (-1: none);
    // tail_seq: the last fit whose tail - it starts by waiting for that fit - is already on the second stream.
    bool in_aside[2] = {false, false};
    long long in_reader[2] = {-1, -1};
    long long tail_seq = -1;
    int tail_k = -1;                // result arena whose tail is still to be enqueued (-1: none)
    bool tail_big = false;
    bool stage_zerocopy = false;    // staged inputs stay in pinned memory, the fit kernel's prologue reads them there (no copy kernel, no lanes)
    bool staged = false;            // inputs were staged since the last fit: the next bf_fit must carry BF_FIT_RESET
    long long fit_seq = 0;          // fits issued so far (a result arena's `seq` is one of these numbers)
    ResultArena arena[2];
    size_t res_total = 0;           // floats of a result arena
    size_t res_small = 0;           // floats up to the end of `joints` (everything but the vertices)
    size_t res_off[5] = {0, 0, 0, 0, 0}, res_cnt[5] = {0, 0, 0, 0, 0};   // params, terms, state, joints, vout
    int cur = 0;                    // arena the DevBuf views / h_* pointers are on
    hipStream_t copy_stream = nullptr;
    // dense schedule with the fit kernel resident for the whole call (BfDoor, bf_internal.h)
    hipStream_t fit_stream = nullptr;
    hipEvent_t ev_aux[2] = {nullptr, nullptr};   // fork / join of the dense keypoint loss on the second stream
    // bf_batch_dense_timing: events between the kernel classes of the LAST dense iteration of a fit (recorded only when asked for)
    bool dense_timing = false, dense_timed = false;
    hipEvent_t ev_dense[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool door_usable = false;           // the self-test at first use found the fit stream running beside the batch stream
    bool scans_lost = false;            // a scan this batch held was destroyed under it: fits fail until a bf_batch_set_scans call succeeds
    bool kp_door_ok = false;            // ... and the second stream beside the batch stream (the doorbell join of config 5's keypoint workgroups)
    int dense_resident = -1;            // bf_batch_dense_resident: how the last dense fit ran
    hipEvent_t ev_door[2] = {nullptr, nullptr};
    DevBuf<int> door;
    int *h_resident = nullptr;          // pinned, device-visible: workgroups of the persistent launch that have started (this call)
    int kp_tickets = 0;                 // keypoint workgroups launched beside the search since the doors were last zeroed (BF_DOOR_KP's target)
    int *h_door_err = nullptr;          // pinned; copied from door[BF_DOOR_ERR] at the end of a call, read by bf_sync_all
    hipGraphExec_t graph_pipe[2] = {nullptr, nullptr};   // kernels-only graphs of the pipelined path, one per arena
    bf_graph_key graph_pipe_key[2]{};
    float *h_params = nullptr, *h_vout = nullptr, *h_joints = nullptr, *h_terms = nullptr, *h_state = nullptr;
    bool fetched = false;
    int steps_done = 0;
    bf_hyper adam_hyper{};
    int adam_cap = 0;
    DevBuf<float> proj, keypoints, params, adam_m, adam_v, grads, terms, state, vraw, vout, joints, adam_tab, debug, xpart;
    DevBuf<int> ndiv;
    bool have_result = false;
    hipGraphExec_t graph_exec = nullptr;     // BF_FIT_GRAPH: the captured [re-arm, fit, mesh, joints, fetch] sequence
    bf_graph_key graph_key{};
    // dense vertex losses (use_mesh, smplify.py:146-156,205-206)
    std::vector<struct bf_scan *> scans;
    DevBuf<ScanDev> scan_dev;
    float *h_pc_weight = nullptr;   // pinned staging of pc_weight
    DevBuf<float> cscale, pc_weight, pc_partial, pc_loss, dvout, vposed, cpts, ext_part, ext;
    DevBuf<int> cface, lmk_vid;
    bool cface_valid = false;       // cface holds the faces of an earlier closest-point call for these scans (warm start)
    DevBuf<float> jraw, lmk_w;
    BfMasks masks;
    // SMPL+D stage (smplify.py:228-247)
    DevBuf<float> disp, disp_m, disp_v, disp_base, disp_P, disp_fn, disp_vn, disp_dv, disp_dPf;
    DevBuf<const float *> scan_fn;
    int disp_steps = 0;
    bool have_disp = false;
    int n_cus = 256;                    // compute units of the model's device (bf_batch_create)
    BfLanes lanes;                      // fit lanes (BF_FIT_LANES): lanes.h
    enum class TailHandOver { BY_SIZE, STORE, COPY };
    TailHandOver tail_handover = TailHandOver::BY_SIZE;         // BF_TAIL_HANDOVER (store | copy; unset: by size), read once per batch: whether a tail's
                                        // kernels store into the pinned mirror themselves (MeshPass::mirror) - store: wherever they can; copy: never, the
                                        // hand-over is a launch or a copy command behind them; by size: where that measured faster (tail_stores, api.hip)
};

struct bf_scan {
    int device = 0, nv = 0, nf = 0, n_entries = 0;
    std::vector<struct bf_batch *> holders;   // batches that hold this scan (bf_batch_set_scans), one entry per frame slot, under bf_scan_links():
                                              // destroying the scan waits for the device and detaches those batches' scans first
    ScanDev dev{};
    DevBuf<ScanDev> dev_resident;             // `dev` in device memory for the *_dev calls (mesh_loss_api.hip), made by the first of them
    DevBuf<float> verts, face_norms;
    DevBuf<int> faces, cell_start, cell_tris;
    DevBuf<float> cell_pack, cell_box;
};


inline std::mutex &bf_scan_links() { static std::mutex mu; return mu; }      // guards bf_scan::holders and bf_batch::scans of every object
void bf_batch_unlink_scans(struct bf_batch *b);                                // (caller holds bf_scan_links(); device idle) batch forgets its scans, scans forget the batch

// Shared between the host files (api.hip, dense_api.hip, mask_api.hip, scan_api.hip): ordinary C++ functions, hidden in the library like
// everything include/bodyfit.h does not declare - a declaration here that differs from its definition fails to link.
int bf_ensure_fit_image(struct bf_batch *b, FrameIO io, const HyperDev &hd);
// One forward mesh pass of `n` frames from their pose states, and the joints pass behind it when joints, joints_ori or jraw is asked for.
// Null / zero fields are left out of the pass.
struct MeshPass {
    // what is read
    MeshScratch *scr = nullptr;         // the stream owner's scratch: the batched path (>= BF_MFMA_MIN_FRAMES frames) needs one
    int n = 0;
    int per = 0;                        // > 0: the n frames are n / per independent calls' of `per` frames each (a fit-lane group) and every
                                        // frame gets the bits it gets in a pass of its call alone: one multi-frame launch for calls below 16
                                        // frames, a pass per call from there on (mesh_choice.h)
    const float *state = nullptr;
    hipStream_t stream = nullptr;
    const MeshTab *tab = nullptr;       // the sampled-first sub-model inside a dense loop without scans (null: the model's own table)
    // what is written
    float *vraw = nullptr, *vout = nullptr, *xpart = nullptr, *vposed = nullptr;
    float *joints = nullptr, *joints_ori = nullptr, *jraw = nullptr;
    int *lmk_vid = nullptr;
    float *lmk_w = nullptr;
    // what rides along
    float *dvzero = nullptr;            // a [n][NV][3] buffer the forward pass should zero while it is at it - only the 1..15-frame kernel does, `zeroed` says so
    bool want_xpart = false;            // fill xpart although no joints are asked for here - the caller forms them itself
    const MaskProj *mproj = nullptr;    // project the sampled vertices into the mask views as well - only the 1..15-frame kernel does, `projected` says so
    int *door = nullptr;                // the resident fit launch's doorbells the pass waits on, up to door_target
    int door_target = 0;
    hipEvent_t after_mesh = nullptr;    // recorded between the mesh and the joints pass
    hipEvent_t mesh_done = nullptr;     // completes with the mesh dispatch itself where the kernel can carry it: `mesh_done_set` says so
    const BfHandOver *mirror = nullptr; // the pinned mirror of the result arena the pass fills (vout, joints: its slices): the mesh kernel stores its
                                        // vertices there too and the joints kernel the arena's small slices - only the kernels below 16 frames per call do,
                                        // and never with a doorbell, a sub-model table or vposed; `handed_over` says so, the caller copies otherwise
};
struct MeshPassDone { bool zeroed = false, projected = false, mesh_done_set = false, handed_over = false; };      // (cleared by bf_launch_mesh)
int bf_launch_mesh(bf_model *m, const MeshPass &p, MeshPassDone &done);
inline int bf_launch_mesh(bf_model *m, const MeshPass &p) { MeshPassDone unasked; return bf_launch_mesh(m, p, unasked); }
int bf_fit_with_scans(bf_batch *b, int n_iters, const bf_hyper &h, const HyperDev &hd, FrameIO io);
int bf_dense_loss_grad(bf_batch *b, const bf_hyper &h, const HyperDev &hd, FrameIO io);
int bf_dense_iter_eval(bf_batch *b, const bf_hyper &h, const HyperDev &hd, FrameIO io, bool late, bool use_sub, const float *dverts_extra,
                       float *terms6);
int bf_ensure_dense_buffers(bf_batch *b);
int bf_ensure_posedirsT_locked(bf_model *m, hipStream_t stream);   // (caller holds m->lazy) posedirsT built on first use
// contours of n binary masks on the device (mask_api.hip): shared by bf_extract_contours and bf_silhouette_create
int bf_contours_on_device(const unsigned char *d_bin, int n, int H, int W, int select, std::vector<int> &counts, std::vector<int> &half,
                          DevBuf<float> &d_xy, int &cap);
// what a fit does with the batch's silhouettes, in this order (the rules: BfMasks)
void bf_masks_commit(bf_batch *b);       // no-op unless bf_batch_stage_masks has staged the next frame's silhouettes: they become the active ones
int bf_masks_finalize(bf_batch *b);      // no-op unless a deferred border following is pending: before the first kernel that reads the contours
int bf_masks_mark_used(bf_batch *b);     // no-op without masks: the fit just queued on the batch stream is the last reader of the active arena
HyperDev bf_to_dev(const bf_hyper &h);
// the frame loop's pieces that api.hip defines and the fit lanes (lanes.hip) use as well
FrameIO bf_frame_io(bf_batch *b, bool want_grads);      // the batch's own launch arguments
int bf_publish(hipStream_t stream, float *dst, const float *src, size_t n_floats);     // a copy by kernel, device arena <-> pinned buffer, whole 256-byte slices
struct TailOn { hipStream_t stream; MeshScratch *scr; float *vraw, *xpart; };           // the stream a tail runs on and that stream's owner's scratch buffers
int bf_enqueue_tail(bf_batch *b, ResultArena &r, const size_t off[5], int n_frames, int per, const TailOn &on, size_t n_floats,
                    bool with_mesh, bool may_store, bool big);
void bf_use_arena(bf_batch *b, int k);
void bf_set_inputs(bf_batch *b, const InputCursor &at, float *kp, float *p0, int *ndiv);
BfInitMap bf_init_map(const bf_model *m);
int bf_pack_staging(const bf_batch *b, float *h, hipEvent_t ev, bool &pending, const float *keypoints, const int32_t *n_use_frames,
                    const float *init_betas, const float *init_pose);
int bf_flush_tail(bf_batch *b);          // enqueue the deferred mesh / hand-over tail of the last frame-after-frame fit (api.hip)
int bf_sync_all(bf_batch *b);            // lanes, copy stream, then compute stream
int bf_lanes_drain(bf_batch *b);         // no-op unless fit lanes are on: launch the open group, wait for the lanes, hand the last lane fit back to the batch
int bf_guard_arena(bf_batch *b);         // the compute stream waits for a fetch still reading the current arena
// `with_kp`: the dense keypoint loss rides in the contour launch (bf_kp_contour_kernel) instead of a launch of its own
int launch_mask_kernels(bf_batch *b, float weight, bool want_loss, bool sum_views = true, const bf_hyper *with_kp = nullptr,
                        bool projected = false, const bf_model::Sub *sub = nullptr, bool fold_acc = false);
int launch_state_and_mesh(bf_batch *b, const HyperDev &hd);
