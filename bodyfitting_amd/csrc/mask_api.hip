// Host side of the silhouette (use_mask) path: contour extraction on the device, attaching and staging a batch's masks, the deferred
// bookkeeping behind them, and the stand-alone mask loss.
#include "bf_host.h"
#include "mask_kernels.h"

// use_mask=True (smplify.py:138-144): masks[F,M,H,W] uint8 as read from disk (thresholded > 128 here),
// view_index[M] = position of each mask view among the V views (use_frames.index(frame), smplify.py:141-142),
// contours: for every (frame, mask view) contour_count points (x, y), concatenated in contour_xy
// (extract_countours, loss.py:73-83 - the caller extracts them; the loss only sums over the points).

namespace {
// bf_contour_kernel keeps a mask's three bit planes in LDS up to kPlanesInLds bytes, in global memory beyond; dynamic LDS above kLdsUnasked
// has to be allowed first (raise_lds: the one-shot extraction and the attach do; stagings and re-follows keep the attach's shape).
constexpr size_t kPlanesInLds = 150 * 1024, kLdsUnasked = 64 * 1024;
struct PlaneGeom {
    int wpr;                    // 32-bit words per row of a plane
    size_t plane_bytes;         // a mask's three planes
    bool in_lds;
    PlaneGeom(int H, int W) : wpr((W + 31) / 32), plane_bytes((size_t)3 * H * wpr * sizeof(unsigned)), in_lds(plane_bytes <= kPlanesInLds) {}
    size_t lds() const { return in_lds ? plane_bytes : 0; }
    size_t global_words(size_t n) const { return in_lds ? 0 : n * (plane_bytes / sizeof(unsigned)); }
    hipError_t raise_lds() const {
        return lds() > kLdsUnasked ? hipFuncSetAttribute((const void *)bf_contour_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plane_bytes) : hipSuccess;
    }
};

// THE border-following pass, queued on `stream`: n masks d_bin[n][H][W] -> slab[n][2][cap][2] and cnt2[2 n] (lengths | which half of the
// slab holds each contour; a border longer than cap is counted, not stored), cnt2 read back into `counts`.  `planes`: global room for
// the bit planes, used only when they do not fit LDS.
int follow_borders(hipStream_t stream, size_t n, int H, int W, const unsigned char *d_bin, float *slab, int *cnt2, unsigned *planes, int cap,
                   int select, int *counts) {
    const PlaneGeom g(H, W);
    hipLaunchKernelGGL(bf_contour_kernel, dim3((unsigned)n), dim3(256), g.lds(), stream, d_bin, H, W, cap, select, slab, cnt2,
                       g.in_lds ? (unsigned *)nullptr : planes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts, cnt2, 2 * n * sizeof(int), hipMemcpyDeviceToHost, stream));
    return BF_OK;
}
int follow_borders(hipStream_t stream, size_t n, const MaskIO &K, MaskArena &A, int cap) {      // ... of an arena's masks into its own buffers
    return follow_borders(stream, n, K.H, K.W, A.masks.p, A.slab.p, A.cnt2.p, A.planes.p, cap, A.select, A.h_counts);
}

template <class T>
hipError_t grow_pinned(T *&p, size_t &n, size_t count) {        // a pinned buffer of at least `count` elements; contents undefined
    if (n >= count) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; n = 0;
    hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
}

// A device buffer of at least `count` elements; contents undefined.  The block it replaces (BfMasks, Freeing) is FREEd now (attach: the
// device is idle), RETIREd IF too SMALL and kept otherwise (staging), or RETIREd ALWAYS (finalize's regrow).
enum class Outgrown { FREE, RETIRE_IF_SMALL, RETIRE_ALWAYS };
template <class T>
hipError_t grow_dev(BfMasks &M, DevBuf<T> &buf, size_t count, Outgrown how) {
    const bool owned = buf.p && (how == Outgrown::RETIRE_IF_SMALL || !buf.view);
    if (how != Outgrown::RETIRE_ALWAYS && owned && buf.n >= count) return hipSuccess;
    if (how == Outgrown::FREE) buf.release();
    else if (owned) M.retired.push_back((void *)buf.p);
    buf.p = nullptr;
    return buf.alloc(count);
}
}  // namespace

// Contours of n binary masks on the device.  d_bin[n][H][W] -> counts (host), d_xy[n][2][cap][2] (device slab; half[i] says which half
// holds mask i's contour).  The slab is grown and the pass re-run when a contour is longer than the first guess.
int bf_contours_on_device(const unsigned char *d_bin, int n, int H, int W, int select, std::vector<int> &counts, std::vector<int> &half,
                              DevBuf<float> &d_xy, int &cap) {
    const PlaneGeom g(H, W);
    DevBuf<unsigned> planes;
    DevBuf<int> d_cnt;
    if (!g.in_lds) HIP_TRY(planes.alloc(g.global_words(n)));
    HIP_TRY(d_cnt.alloc(2 * (size_t)n));
    HIP_TRY(g.raise_lds());
    counts.assign(n, 0);
    cap = std::max(64, 4 * (H + W));
    for (int attempt = 0; attempt < 2; ++attempt) {
        d_xy.release();
        HIP_TRY(d_xy.alloc((size_t)n * 2 * cap * 2));
        std::vector<int> both(2 * (size_t)n);
        BF_TRY(follow_borders(nullptr, n, H, W, d_bin, d_xy.p, d_cnt.p, planes.p, cap, select, both.data()));
        HIP_TRY(hipStreamSynchronize(nullptr));
        counts.assign(both.begin(), both.begin() + n);
        half.assign(both.begin() + n, both.end());
        const int longest = *std::max_element(counts.begin(), counts.end());
        if (longest <= cap) return BF_OK;
        cap = longest;
    }
    return fail(BF_ERR_HIP, "contour extraction: inconsistent contour length");
}

extern "C" {
// extract_countours (smplify/loss.py:73-83): masks[n][H][W] uint8, non-zero = foreground (the reference passes
// (mask > 128) * 255) -> counts[n] and, when xy != NULL, the contours' (x, y) points concatenated (sum(counts) pairs,
// which the caller learns from a first call with xy == NULL).
int bf_extract_contours(int device, int n, int H, int W, const uint8_t *masks, int32_t *counts, float *xy, int select) {
    if (n <= 0 || H <= 0 || W <= 0 || !masks || !counts || select < 0 || select > 2) return fail(BF_ERR_INVALID, "bf_extract_contours: bad argument");
    if (bf_device_count() <= device || device < 0) return fail(BF_ERR_NO_DEVICE, "bf_extract_contours: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    DevBuf<unsigned char> d_bin;
    HIP_TRY(d_bin.upload(masks, (size_t)n * H * W));
    std::vector<int> cnt, half;
    DevBuf<float> d_xy;
    int cap = 0;
    int rc = bf_contours_on_device(d_bin.p, n, H, W, select, cnt, half, d_xy, cap);
    if (rc) return rc;
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        counts[i] = cnt[i];
        if (xy && cnt[i] > 0) HIP_TRY(hipMemcpy(xy + o * 2, d_xy.p + ((size_t)i * 2 + half[i]) * cap * 2, (size_t)cnt[i] * 2 * sizeof(float), hipMemcpyDeviceToHost));
        o += cnt[i];
    }
    return BF_OK;
}

int bf_batch_set_masks(bf_batch *b, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks,
                       const int32_t *contour_count, const float *contour_xy, int contour_select) {
    if (!b || contour_select < 0 || contour_select > 2) return fail(BF_ERR_INVALID, "bf_batch_set_masks: null batch / bad contour_select");
    HIP_TRY(hipSetDevice(b->m->device));
    BfMasks &M = b->masks;
    MaskArena &A = M.arena[M.cur];
    if (n_masks > 0 && masks) {
        if (!view_index || (contour_count && !contour_xy) || H <= 0 || W <= 0) return fail(BF_ERR_INVALID, "bf_batch_set_masks: bad argument");
        for (int i = 0; i < n_masks; ++i)
            if (view_index[i] < 0 || view_index[i] >= b->V) return fail(BF_ERR_INVALID, "bf_batch_set_masks: view index out of range");
        // the host's share - binarising 2 MB per frame (smplify.py:139) - BEFORE the wait for the work in flight (BfMasks, Attach)
        const size_t npix0 = (size_t)b->F * n_masks * H * W;
        if (A.ev) HIP_TRY(hipEventSynchronize(A.ev));
        HIP_TRY(grow_pinned(A.h_masks, A.h_masks_n, npix0));
        for (size_t i = 0; i < npix0; ++i) A.h_masks[i] = masks[i] > 128;
    }
    BF_TRY(bf_sync_all(b));
    if (n_masks <= 0 || !masks) { M.on = false; M.pending = false; return BF_OK; }   // (bf_sync_all above drained a deferred extraction)
    const int F = b->F, nv = b->m->nv;
    // (a frame loop hands over new masks of the same shape every frame: device buffers are kept and only grown - a dozen hipFree /
    //  hipMalloc pairs cost more than the contour extraction itself)
    auto ensure = [&M](auto &buf, size_t count) { return grow_dev(M, buf, count, Outgrown::FREE); };
    const size_t npix = (size_t)F * n_masks * H * W, fm = (size_t)F * n_masks;
    const int ns = (nv + 3) / 4, pblocks = (ns + 255) / 256;
    HIP_TRY(ensure(A.masks, npix));
    HIP_TRY(ensure(M.view, n_masks)); HIP_TRY(ensure(M.cstart, fm)); HIP_TRY(ensure(M.ccount, fm));
    HIP_TRY(hipMemcpy(M.view.p, view_index, (size_t)n_masks * sizeof(int), hipMemcpyHostToDevice));
    M.view_host.assign(view_index, view_index + n_masks);
    M.staged = false;                                        // (masks set synchronously supersede staged ones)
    HIP_TRY(ensure(M.uvi, fm * ns * 4)); HIP_TRY(ensure(M.duvb, fm * ns * 2)); HIP_TRY(ensure(M.gpart, fm * ns * 3)); HIP_TRY(ensure(M.acc, fm * ns * 2));
    HIP_TRY(ensure(M.loss, F));
    MaskIO &K = M.io;
    K.nv = nv; K.ns = ns; K.n_views = b->V; K.n_masks = n_masks; K.H = H; K.W = W; K.proj_blocks = pblocks;
    K.cdist = 1; K.sstride = 4; K.imsize = 512.f; K.eps = 10.f; K.weight = 5.f;
    K.view_index = M.view.p; K.masks = A.masks.p;
    M.pending = false;
    M.on_device = !contour_count;
    if (!contour_count) {
        // DEFERRED: upload + border following on the second stream; lengths into pinned memory; bf_masks_finalize does the rest
        if (!A.ev) HIP_TRY(hipEventCreateWithFlags(&A.ev, hipEventDisableTiming));
        HIP_TRY(grow_pinned(A.h_counts, A.h_counts_n, 2 * fm));
        const PlaneGeom g(H, W);
        if (!g.in_lds) HIP_TRY(ensure(A.planes, g.global_words(fm)));
        HIP_TRY(g.raise_lds());
        M.cap = std::max(M.cap, std::max(64, 4 * (H + W)));
        A.select = contour_select;
        M.free_retired();
        // everything bf_masks_finalize fills is sized NOW, for borders as long as the slab holds (BfMasks, Freeing)
        const size_t cap = (size_t)M.cap;
        HIP_TRY(ensure(A.slab, fm * 2 * cap * 2)); HIP_TRY(ensure(A.cnt2, 2 * fm));
        HIP_TRY(ensure(M.cxy, fm * cap * 2)); HIP_TRY(ensure(M.choice, fm * cap)); HIP_TRY(ensure(M.cgrad, fm * cap * 2));
        HIP_TRY(ensure(M.part, fm * (pblocks + (cap * 16 + 255) / 256)));
        hipStream_t cs = b->copy_stream;
        HIP_TRY(hipMemcpyAsync(A.masks.p, A.h_masks, npix, hipMemcpyHostToDevice, cs));
        BF_TRY(follow_borders(cs, fm, K, A, M.cap));
        HIP_TRY(hipEventRecord(A.ev, cs));
        M.pending = true;
        M.on = true;
        K.cmax = 1; K.part_stride = pblocks + 1;           // (placeholders until finalize; nothing reads them before)
        return bf_ensure_dense_buffers(b);
    }
    HIP_TRY(hipMemcpy(A.masks.p, A.h_masks, npix, hipMemcpyHostToDevice));
    std::vector<int> start(fm), count(contour_count, contour_count + fm);
    int total = 0, cmax = 1;
    for (size_t i = 0; i < fm; ++i) {
        if (count[i] < 0) return fail(BF_ERR_INVALID, "bf_batch_set_masks: negative contour count");
        start[i] = total; total += count[i]; cmax = std::max(cmax, count[i]);
    }
    const int stride = pblocks + (cmax * 16 + 255) / 256;     // (16 lanes per contour point)
    HIP_TRY(hipMemcpy(M.cstart.p, start.data(), fm * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(M.ccount.p, count.data(), fm * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(ensure(M.cxy, (size_t)std::max(total, 1) * 2));
    if (total > 0) HIP_TRY(hipMemcpy(M.cxy.p, contour_xy, (size_t)total * 2 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(ensure(M.choice, fm * cmax)); HIP_TRY(ensure(M.cgrad, fm * cmax * 2));
    HIP_TRY(ensure(M.part, fm * stride));
    K.cmax = cmax; K.part_stride = stride;
    K.contour_start = M.cstart.p; K.contour_count = M.ccount.p; K.contour_xy = M.cxy.p;
    M.on = true;
    return bf_ensure_dense_buffers(b);
}

/* The NEXT frame's silhouettes, WITHOUT draining the work in flight (the frame loop of apps/genebody_fitting.py:183-192 hands SMPLify
 * new masks with every frame): same views and shape as the masks attached with bf_batch_set_masks (contours extracted on the device).
 * They are binarised, uploaded and border-followed into the arena that is not the active one, on the batch's second stream - under the
 * fit in flight - and the next bf_fit switches to that arena (bf_masks_commit).  Two-deep like bf_batch_stage_inputs (BfMasks, Staging). */
int bf_batch_stage_masks(bf_batch *b, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks, int contour_select) {
    if (!b || !view_index || !masks || contour_select < 0 || contour_select > 2) return fail(BF_ERR_INVALID, "bf_batch_stage_masks: bad argument");
    BfMasks &M = b->masks;
    const MaskIO &K = M.io;
    if (!M.on || !M.on_device || K.n_masks != n_masks || K.H != H || K.W != W || (int)M.view_host.size() != n_masks ||
        !std::equal(view_index, view_index + n_masks, M.view_host.begin()))
        return fail(BF_ERR_INVALID, "bf_batch_stage_masks: the first frame's masks go through bf_batch_set_masks (device contours); later frames must "
                                    "keep its views and shape");
    HIP_TRY(hipSetDevice(b->m->device));
    MaskArena &S = M.arena[M.cur ^ 1];
    const size_t fm = (size_t)b->F * n_masks, npix = fm * H * W;
    if (S.ev_used) HIP_TRY(hipEventSynchronize(S.ev_used));          // the fit that read this arena two frames ago
    if (S.ev) HIP_TRY(hipEventSynchronize(S.ev));
    HIP_TRY(grow_pinned(S.h_masks, S.h_masks_n, npix)); HIP_TRY(grow_pinned(S.h_counts, S.h_counts_n, 2 * fm));
    for (size_t i = 0; i < npix; ++i) S.h_masks[i] = masks[i] > 128;
    // (first use, or the shared cap has grown since: fresh blocks)
    auto fresh = [&M](auto &buf, size_t count) { return grow_dev(M, buf, count, Outgrown::RETIRE_IF_SMALL); };
    const PlaneGeom g(H, W);
    HIP_TRY(fresh(S.masks, npix)); HIP_TRY(fresh(S.slab, fm * 2 * (size_t)M.cap * 2)); HIP_TRY(fresh(S.cnt2, 2 * fm));
    if (!g.in_lds) HIP_TRY(fresh(S.planes, g.global_words(fm)));
    if (!S.ev) HIP_TRY(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
    S.select = contour_select;
    hipStream_t cs = b->copy_stream;
    HIP_TRY(hipMemcpyAsync(S.masks.p, S.h_masks, npix, hipMemcpyHostToDevice, cs));
    BF_TRY(follow_borders(cs, fm, K, S, M.cap));
    HIP_TRY(hipEventRecord(S.ev, cs));
    M.staged = true;
    return BF_OK;
}
}  // extern "C"

void bf_masks_commit(bf_batch *b) {
    BfMasks &M = b->masks;
    if (!M.staged) return;
    M.staged = false;
    M.cur ^= 1;
    M.io.masks = M.arena[M.cur].masks.p;
    M.io.cmax = 1; M.io.part_stride = M.io.proj_blocks + 1;             // (placeholders until finalize, as after bf_batch_set_masks)
    M.pending = true;
}

int bf_masks_mark_used(bf_batch *b) {
    if (!b->masks.on) return BF_OK;
    MaskArena &A = b->masks.arena[b->masks.cur];
    if (!A.ev_used) HIP_TRY(hipEventCreateWithFlags(&A.ev_used, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(A.ev_used, b->stream));
    return BF_OK;
}

// The second half of a deferred border following: size and fill what depends on the contour lengths (BfMasks, Finalize).
int bf_masks_finalize(bf_batch *b) {
    BfMasks &M = b->masks;
    if (!M.pending) return BF_OK;
    M.pending = false;
    MaskArena &A = M.arena[M.cur];
    HIP_TRY(hipEventSynchronize(A.ev));
    MaskIO &K = M.io;
    const size_t fm = (size_t)b->F * K.n_masks;
    int *h = A.h_counts;                                      // [0, fm): lengths; [fm, 2 fm): halves -> reused below for the offsets
    int longest = 0;
    for (size_t i = 0; i < fm; ++i) longest = std::max(longest, h[i]);
    if (longest > M.cap) {
        // a border longer than the slab (more than 4 (H + W) points; counted, not stored): once more with room for it - nothing is FREED here
        auto regrow = [&M](auto &buf, size_t count) { return grow_dev(M, buf, count, Outgrown::RETIRE_ALWAYS); };
        M.cap = longest;
        const size_t cap = (size_t)longest;
        HIP_TRY(regrow(A.slab, fm * 2 * cap * 2));
        HIP_TRY(regrow(M.cxy, fm * cap * 2)); HIP_TRY(regrow(M.choice, fm * cap)); HIP_TRY(regrow(M.cgrad, fm * cap * 2));
        HIP_TRY(regrow(M.part, fm * (K.proj_blocks + (cap * 16 + 255) / 256)));
        BF_TRY(follow_borders(b->copy_stream, fm, K, A, M.cap));
        HIP_TRY(hipStreamSynchronize(b->copy_stream));
    }
    std::vector<int> start(fm);
    int total = 0, cmax = 1;
    for (size_t i = 0; i < fm; ++i) { start[i] = total; total += h[i]; cmax = std::max(cmax, h[i]); }
    const int stride = K.proj_blocks + (cmax * 16 + 255) / 256;
    std::vector<int> half(h + fm, h + 2 * fm);
    for (size_t i = 0; i < fm; ++i) h[fm + i] = start[i];
    HIP_TRY(hipMemcpyAsync(M.ccount.p, h, fm * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(M.cstart.p, h + fm, fm * sizeof(int), hipMemcpyHostToDevice, b->stream));
    for (size_t i = 0; i < fm; ++i)
        if (h[i] > 0)
            HIP_TRY(hipMemcpyAsync(M.cxy.p + (size_t)start[i] * 2, A.slab.p + (i * 2 + half[i]) * (size_t)M.cap * 2,
                                   (size_t)h[i] * 2 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
    K.cmax = cmax; K.part_stride = stride;
    K.contour_start = M.cstart.p; K.contour_count = M.ccount.p; K.contour_xy = M.cxy.p;
    return BF_OK;
}

extern "C" {
// multview_mask_loss (loss.py:85-130) at the current parameters: loss[F] (unweighted, as the function
// returns it) and its gradient w.r.t. body_vertices dverts[F,NV,3] (non-zero on every 4th vertex only).
int bf_batch_mask_loss(bf_batch *b, const bf_hyper *hyper, float *loss, float *dverts) {
    if (!b || !b->masks.on) return fail(BF_ERR_INVALID, "bf_batch_mask_loss: no masks attached");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_masks_finalize(b));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    HyperDev hd = bf_to_dev(h);
    b->masks.io.imsize = h.imsize;
    b->masks.io.cdist = h.mask_cdist_form != 0.f;
    int rc = bf_guard_arena(b);
    if (rc) return rc;
    rc = launch_state_and_mesh(b, hd);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(b->dvout.p, 0, b->dvout.n * sizeof(float), b->stream));
    rc = launch_mask_kernels(b, 1.0f, true);
    if (rc) return rc;
    BF_TRY(bf_sync_all(b));
    if (loss) HIP_TRY(hipMemcpy(loss, b->masks.loss.p, (size_t)b->F * sizeof(float), hipMemcpyDeviceToHost));
    if (dverts) HIP_TRY(hipMemcpy(dverts, b->dvout.p, b->dvout.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}
}  // extern "C"
