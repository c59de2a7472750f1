// Host side of the silhouette (use_mask) path: contour extraction on the device, attaching and staging a batch's masks, the deferred
// bookkeeping behind them, and the stand-alone mask loss.
#include "bf_host.h"
#include "mask_kernels.h"

// use_mask=True (smplify.py:138-144): masks[F,M,H,W] uint8 as read from disk (thresholded > 128 here),
// view_index[M] = position of each mask view among the V views (use_frames.index(frame), smplify.py:141-142),
// contours: for every (frame, mask view) contour_count points (x, y), concatenated in contour_xy
// (extract_countours, loss.py:73-83 - the caller extracts them; the loss only sums over the points).
// Contours of n binary masks on the device (bf_contour_kernel).  d_bin[n][H][W] -> counts (host), d_xy[n][2][cap][2] (device slab;
// half[i] says which half holds mask i's contour).
// The slab is grown and the kernel re-run when a contour is longer than the first guess.
int bf_contours_on_device(const unsigned char *d_bin, int n, int H, int W, int select, std::vector<int> &counts, std::vector<int> &half,
                              DevBuf<float> &d_xy, int &cap) {
    const int wpr = (W + 31) / 32;
    const size_t plane_bytes = (size_t)3 * H * wpr * sizeof(unsigned);
    const bool in_lds = plane_bytes <= 150 * 1024;
    DevBuf<unsigned> planes;
    DevBuf<int> d_cnt;
    if (!in_lds) HIP_TRY(planes.alloc((size_t)n * 3 * H * wpr));
    HIP_TRY(d_cnt.alloc(2 * (size_t)n));
    if (in_lds && plane_bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)bf_contour_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plane_bytes));
    counts.assign(n, 0);
    cap = std::max(64, 4 * (H + W));
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (d_xy.p) { (void)hipFree(d_xy.p); d_xy.p = nullptr; }
        HIP_TRY(d_xy.alloc((size_t)n * 2 * cap * 2));
        hipLaunchKernelGGL(bf_contour_kernel, dim3(n), dim3(256), in_lds ? plane_bytes : 0, 0, d_bin, H, W, cap, select, d_xy.p, d_cnt.p,
                           in_lds ? (unsigned *)nullptr : planes.p);
        HIP_TRY(hipGetLastError());
        std::vector<int> both(2 * (size_t)n);
        HIP_TRY(hipMemcpy(both.data(), d_cnt.p, both.size() * sizeof(int), hipMemcpyDeviceToHost));
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
    if (n_masks > 0 && masks) {
        if (!view_index || (contour_count && !contour_xy) || H <= 0 || W <= 0) return fail(BF_ERR_INVALID, "bf_batch_set_masks: bad argument");
        for (int i = 0; i < n_masks; ++i)
            if (view_index[i] < 0 || view_index[i] >= b->V) return fail(BF_ERR_INVALID, "bf_batch_set_masks: view index out of range");
        // The host's share - binarising 2 MB per frame (smplify.py:139) into the pinned staging buffer - happens BEFORE the wait for the
        // work in flight: in a frame loop that is the previous frame's fit, and the buffer is free (its last upload, ev_masks, went out
        // early in that fit).
        const size_t npix0 = (size_t)b->F * n_masks * H * W;
        if (b->ev_masks) HIP_TRY(hipEventSynchronize(b->ev_masks));
        if (b->h_masks_n < npix0) {
            if (b->h_masks) (void)hipHostFree(b->h_masks);
            b->h_masks = nullptr;
            HIP_TRY(hipHostMalloc((void **)&b->h_masks, npix0));
            b->h_masks_n = npix0;
        }
        for (size_t i = 0; i < npix0; ++i) b->h_masks[i] = masks[i] > 128;
    }
    BF_TRY(bf_sync_all(b));
    if (n_masks <= 0 || !masks) { b->has_masks = false; b->masks_pending = false; return BF_OK; }   // (bf_sync_all above drained a deferred extraction)
    const int F = b->F, nv = b->m->nv;
    // (a frame loop hands over new masks of the same shape every frame: device buffers are kept and only grown - a dozen hipFree /
    //  hipMalloc pairs cost more than the contour extraction itself)
    auto ensure = [](auto &buf, size_t count) -> hipError_t {
        if (buf.p && buf.n >= count && !buf.view) return hipSuccess;
        if (buf.p && !buf.view) (void)hipFree((void *)buf.p);
        buf.p = nullptr;
        return buf.alloc(count);
    };
    const size_t npix = (size_t)F * n_masks * H * W, fm = (size_t)F * n_masks;
    const int ns = (nv + 3) / 4, pblocks = (ns + 255) / 256;
    // (binarised into pinned staging above, before the wait)
    HIP_TRY(ensure(b->mk_masks, npix));
    HIP_TRY(ensure(b->mk_view, n_masks)); HIP_TRY(ensure(b->mk_cstart, fm)); HIP_TRY(ensure(b->mk_ccount, fm));
    HIP_TRY(hipMemcpy(b->mk_view.p, view_index, (size_t)n_masks * sizeof(int), hipMemcpyHostToDevice));
    b->mk_view_host.assign(view_index, view_index + n_masks);
    b->mk_stage.staged = false;                              // (masks set synchronously supersede staged ones)
    HIP_TRY(ensure(b->mk_uvi, fm * ns * 4)); HIP_TRY(ensure(b->mk_duvb, fm * ns * 2)); HIP_TRY(ensure(b->mk_gpart, fm * ns * 3)); HIP_TRY(ensure(b->mk_acc, fm * ns * 2));
    HIP_TRY(ensure(b->mk_loss, F));
    MaskIO &K0 = b->mask;
    K0.nv = nv; K0.ns = ns; K0.n_views = b->V; K0.n_masks = n_masks; K0.H = H; K0.W = W; K0.proj_blocks = pblocks;
    K0.cdist = 1; K0.sstride = 4; K0.imsize = 512.f; K0.eps = 10.f; K0.weight = 5.f;
    K0.view_index = b->mk_view.p; K0.masks = b->mk_masks.p;
    b->masks_pending = false;
    b->mk_on_device = !contour_count;
    if (!contour_count) {
        // DEFERRED: upload + border following on the second stream; lengths into pinned memory; bf_masks_finalize does the rest
        if (!b->ev_masks) HIP_TRY(hipEventCreateWithFlags(&b->ev_masks, hipEventDisableTiming));
        if (b->h_ccount_n < 2 * fm) {
            if (b->h_ccount) (void)hipHostFree(b->h_ccount);
            b->h_ccount = nullptr;
            HIP_TRY(hipHostMalloc((void **)&b->h_ccount, 2 * fm * sizeof(int)));
            b->h_ccount_n = 2 * fm;
        }
        const int wpr = (W + 31) / 32;
        const size_t plane_bytes = (size_t)3 * H * wpr * sizeof(unsigned);
        const bool in_lds = plane_bytes <= 150 * 1024;
        if (!in_lds) HIP_TRY(ensure(b->mk_planes, fm * 3 * H * wpr));
        if (in_lds && plane_bytes > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)bf_contour_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plane_bytes));
        b->mk_cap = std::max(b->mk_cap, std::max(64, 4 * (H + W)));
        b->mk_select = contour_select;
        HIP_TRY(ensure(b->mk_slab, fm * 2 * (size_t)b->mk_cap * 2));
        HIP_TRY(ensure(b->mk_cnt2, 2 * fm));
        for (float *q : b->mk_retired) (void)hipFree(q);          // (buffers a finalize inside a fit could not free: see there)
        b->mk_retired.clear();
        // everything bf_masks_finalize fills is sized NOW, for borders as long as the slab holds: it runs in the middle of a fit, with
        // the resident fit launch waiting for kernels that are not enqueued yet - a hipFree there (it waits for the device) would
        // never return
        {
            const size_t cap = (size_t)b->mk_cap;
            HIP_TRY(ensure(b->mk_cxy, fm * cap * 2)); HIP_TRY(ensure(b->mk_choice, fm * cap)); HIP_TRY(ensure(b->mk_cgrad, fm * cap * 2));
            HIP_TRY(ensure(b->mk_part, fm * (pblocks + (cap * 16 + 255) / 256)));
        }
        hipStream_t cs = b->copy_stream;
        HIP_TRY(hipMemcpyAsync(b->mk_masks.p, b->h_masks, npix, hipMemcpyHostToDevice, cs));
        hipLaunchKernelGGL(bf_contour_kernel, dim3((unsigned)fm), dim3(256), in_lds ? plane_bytes : 0, cs, (const unsigned char *)b->mk_masks.p, H, W,
                           b->mk_cap, contour_select, b->mk_slab.p, b->mk_cnt2.p, in_lds ? (unsigned *)nullptr : b->mk_planes.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(b->h_ccount, b->mk_cnt2.p, 2 * fm * sizeof(int), hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipEventRecord(b->ev_masks, cs));
        b->masks_pending = true;
        b->has_masks = true;
        K0.cmax = 1; K0.part_stride = pblocks + 1;         // (placeholders until finalize; nothing reads them before)
        return bf_ensure_dense_buffers(b);
    }
    HIP_TRY(hipMemcpy(b->mk_masks.p, b->h_masks, npix, hipMemcpyHostToDevice));
    std::vector<int> start(fm), count(contour_count, contour_count + fm);
    int total = 0, cmax = 1;
    for (size_t i = 0; i < fm; ++i) {
        if (count[i] < 0) return fail(BF_ERR_INVALID, "bf_batch_set_masks: negative contour count");
        start[i] = total; total += count[i]; cmax = std::max(cmax, count[i]);
    }
    const int stride = pblocks + (cmax * 16 + 255) / 256;     // (16 lanes per contour point)
    HIP_TRY(hipMemcpy(b->mk_cstart.p, start.data(), fm * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->mk_ccount.p, count.data(), fm * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(ensure(b->mk_cxy, (size_t)std::max(total, 1) * 2));
    if (total > 0) HIP_TRY(hipMemcpy(b->mk_cxy.p, contour_xy, (size_t)total * 2 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(ensure(b->mk_choice, fm * cmax)); HIP_TRY(ensure(b->mk_cgrad, fm * cmax * 2));
    HIP_TRY(ensure(b->mk_part, fm * stride));
    MaskIO &K = b->mask;
    K.cmax = cmax; K.part_stride = stride;
    K.contour_start = b->mk_cstart.p; K.contour_count = b->mk_ccount.p; K.contour_xy = b->mk_cxy.p;
    b->has_masks = true;
    return bf_ensure_dense_buffers(b);
}

/* The NEXT frame's silhouettes, WITHOUT draining the work in flight (the frame loop of apps/genebody_fitting.py:183-192 hands SMPLify
 * new masks with every frame): same views and shape as the masks attached with bf_batch_set_masks (contours extracted on the device).
 * They are binarised into a second pinned buffer, uploaded and border-followed into a second arena on the batch's second stream - under
 * the fit in flight - and the next bf_fit switches to that arena (bf_masks_commit).  Two-deep like bf_batch_stage_inputs: staging waits
 * for the fit that last read the arena it overwrites. */
int bf_batch_stage_masks(bf_batch *b, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks, int contour_select) {
    if (!b || !view_index || !masks || contour_select < 0 || contour_select > 2) return fail(BF_ERR_INVALID, "bf_batch_stage_masks: bad argument");
    const MaskIO &K = b->mask;
    if (!b->has_masks || !b->mk_on_device || K.n_masks != n_masks || K.H != H || K.W != W || (int)b->mk_view_host.size() != n_masks ||
        !std::equal(view_index, view_index + n_masks, b->mk_view_host.begin()))
        return fail(BF_ERR_INVALID, "bf_batch_stage_masks: the first frame's masks go through bf_batch_set_masks (device contours); later frames must "
                                    "keep its views and shape");
    HIP_TRY(hipSetDevice(b->m->device));
    bf_batch::MaskStage &S = b->mk_stage;
    const size_t fm = (size_t)b->F * n_masks, npix = fm * H * W;
    if (S.ev_used) HIP_TRY(hipEventSynchronize(S.ev_used));          // the fit that read this arena two frames ago
    if (S.ev) HIP_TRY(hipEventSynchronize(S.ev));
    if (S.h_masks_n < npix) {
        if (S.h_masks) (void)hipHostFree(S.h_masks);
        S.h_masks = nullptr;
        HIP_TRY(hipHostMalloc((void **)&S.h_masks, npix));
        S.h_masks_n = npix;
    }
    for (size_t i = 0; i < npix; ++i) S.h_masks[i] = masks[i] > 128;
    if (S.h_ccount_n < 2 * fm) {
        if (S.h_ccount) (void)hipHostFree(S.h_ccount);
        S.h_ccount = nullptr;
        HIP_TRY(hipHostMalloc((void **)&S.h_ccount, 2 * fm * sizeof(int)));
        S.h_ccount_n = 2 * fm;
    }
    const int wpr = (W + 31) / 32;
    const size_t plane_bytes = (size_t)3 * H * wpr * sizeof(unsigned);
    const bool in_lds = plane_bytes <= 150 * 1024;
    // (first use, or the active arena's slab has grown since: fresh blocks - nothing is freed while a fit may be running)
    auto fresh = [&](auto &buf, size_t count) -> hipError_t {
        if (buf.p && buf.n >= count) return hipSuccess;
        if (buf.p) b->mk_retired.push_back((float *)(void *)buf.p);
        buf.p = nullptr;
        return buf.alloc(count);
    };
    HIP_TRY(fresh(S.masks, npix));
    HIP_TRY(fresh(S.slab, fm * 2 * (size_t)b->mk_cap * 2));
    HIP_TRY(fresh(S.cnt2, 2 * fm));
    if (!in_lds) HIP_TRY(fresh(S.planes, fm * 3 * H * wpr));
    if (!S.ev) HIP_TRY(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
    S.select = contour_select;
    hipStream_t cs = b->copy_stream;
    HIP_TRY(hipMemcpyAsync(S.masks.p, S.h_masks, npix, hipMemcpyHostToDevice, cs));
    hipLaunchKernelGGL(bf_contour_kernel, dim3((unsigned)fm), dim3(256), in_lds ? plane_bytes : 0, cs, (const unsigned char *)S.masks.p, H, W,
                       b->mk_cap, contour_select, S.slab.p, S.cnt2.p, in_lds ? (unsigned *)nullptr : S.planes.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.h_ccount, S.cnt2.p, 2 * fm * sizeof(int), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(S.ev, cs));
    S.staged = true;
    return BF_OK;
}
}  // extern "C"

// bf_fit's first act when masks were staged: the two arenas change places (pointers only; the kernels of the fit still in flight
// hold the old ones by value) and the contours are pending again (bf_masks_finalize).
void bf_masks_commit(bf_batch *b) {
    bf_batch::MaskStage &S = b->mk_stage;
    if (!S.staged) return;
    S.staged = false;
    auto swap_buf = [](auto &x, auto &y) { std::swap(x.p, y.p); std::swap(x.n, y.n); };
    std::swap(b->h_masks, S.h_masks); std::swap(b->h_masks_n, S.h_masks_n);
    std::swap(b->h_ccount, S.h_ccount); std::swap(b->h_ccount_n, S.h_ccount_n);
    std::swap(b->ev_masks, S.ev); std::swap(b->ev_masks_used, S.ev_used);
    swap_buf(b->mk_masks, S.masks); swap_buf(b->mk_slab, S.slab); swap_buf(b->mk_cnt2, S.cnt2); swap_buf(b->mk_planes, S.planes);
    std::swap(b->mk_select, S.select);
    b->mask.masks = b->mk_masks.p;
    b->mask.cmax = 1; b->mask.part_stride = b->mask.proj_blocks + 1;      // (placeholders until finalize, as after bf_batch_set_masks)
    b->masks_pending = true;
}

// The second half of a deferred bf_batch_set_masks: wait (host) for the border following on the second stream, then size and fill
// what depends on the contour lengths.  Everything queued here goes onto the BATCH stream, in front of the kernels that read it.
int bf_masks_finalize(bf_batch *b) {
    if (!b->masks_pending) return BF_OK;
    b->masks_pending = false;
    HIP_TRY(hipEventSynchronize(b->ev_masks));
    MaskIO &K = b->mask;
    const size_t fm = (size_t)b->F * K.n_masks;
    int longest = 0;
    for (size_t i = 0; i < fm; ++i) longest = std::max(longest, b->h_ccount[i]);
    if (longest > b->mk_cap) {
        // A border longer than the slab (more than 4 (H + W) points; the kernel counted it without storing): follow again with room
        // for it.  This may be the middle of a fit whose resident launch waits for kernels that are not enqueued yet, so nothing is
        // FREED here (hipFree waits for the device): the outgrown buffers are retired and freed by the next bf_batch_set_masks.
        auto regrow = [&](auto &buf, size_t count) -> hipError_t {
            if (buf.p && !buf.view) b->mk_retired.push_back((float *)(void *)buf.p);
            buf.p = nullptr;
            return buf.alloc(count);
        };
        b->mk_cap = longest;
        const size_t cap = (size_t)longest;
        HIP_TRY(regrow(b->mk_slab, fm * 2 * cap * 2));
        HIP_TRY(regrow(b->mk_cxy, fm * cap * 2)); HIP_TRY(regrow(b->mk_choice, fm * cap)); HIP_TRY(regrow(b->mk_cgrad, fm * cap * 2));
        HIP_TRY(regrow(b->mk_part, fm * (K.proj_blocks + (cap * 16 + 255) / 256)));
        const int wpr = (K.W + 31) / 32;
        const size_t plane_bytes = (size_t)3 * K.H * wpr * sizeof(unsigned);
        const bool in_lds = plane_bytes <= 150 * 1024;
        hipLaunchKernelGGL(bf_contour_kernel, dim3((unsigned)fm), dim3(256), in_lds ? plane_bytes : 0, b->copy_stream, (const unsigned char *)b->mk_masks.p,
                           K.H, K.W, b->mk_cap, b->mk_select, b->mk_slab.p, b->mk_cnt2.p, in_lds ? (unsigned *)nullptr : b->mk_planes.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(b->h_ccount, b->mk_cnt2.p, 2 * fm * sizeof(int), hipMemcpyDeviceToHost, b->copy_stream));
        HIP_TRY(hipStreamSynchronize(b->copy_stream));
    }
    std::vector<int> start(fm);
    int total = 0, cmax = 1;
    for (size_t i = 0; i < fm; ++i) { start[i] = total; total += b->h_ccount[i]; cmax = std::max(cmax, b->h_ccount[i]); }
    const int stride = K.proj_blocks + (cmax * 16 + 255) / 256;
    int *h = b->h_ccount;                                     // [0, fm): lengths; [fm, 2 fm): halves -> reused below for the offsets
    std::vector<int> half(h + fm, h + 2 * fm);
    for (size_t i = 0; i < fm; ++i) h[fm + i] = start[i];
    HIP_TRY(hipMemcpyAsync(b->mk_ccount.p, h, fm * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->mk_cstart.p, h + fm, fm * sizeof(int), hipMemcpyHostToDevice, b->stream));
    for (size_t i = 0; i < fm; ++i)
        if (h[i] > 0)
            HIP_TRY(hipMemcpyAsync(b->mk_cxy.p + (size_t)start[i] * 2, b->mk_slab.p + (i * 2 + half[i]) * (size_t)b->mk_cap * 2,
                                   (size_t)h[i] * 2 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
    K.cmax = cmax; K.part_stride = stride;
    K.contour_start = b->mk_cstart.p; K.contour_count = b->mk_ccount.p; K.contour_xy = b->mk_cxy.p;
    return BF_OK;
}

extern "C" {
// multview_mask_loss (loss.py:85-130) at the current parameters: loss[F] (unweighted, as the function
// returns it) and its gradient w.r.t. body_vertices dverts[F,NV,3] (non-zero on every 4th vertex only).
int bf_batch_mask_loss(bf_batch *b, const bf_hyper *hyper, float *loss, float *dverts) {
    if (!b || !b->has_masks) return fail(BF_ERR_INVALID, "bf_batch_mask_loss: no masks attached");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_masks_finalize(b));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    HyperDev hd = bf_to_dev(h);
    b->mask.imsize = h.imsize;
    b->mask.cdist = h.mask_cdist_form != 0.f;
    int rc = bf_guard_arena(b);
    if (rc) return rc;
    rc = launch_state_and_mesh(b, hd);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(b->dvout.p, 0, b->dvout.n * sizeof(float), b->stream));
    rc = launch_mask_kernels(b, 1.0f, true);
    if (rc) return rc;
    BF_TRY(bf_sync_all(b));
    if (loss) HIP_TRY(hipMemcpy(loss, b->mk_loss.p, (size_t)b->F * sizeof(float), hipMemcpyDeviceToHost));
    if (dverts) HIP_TRY(hipMemcpy(dverts, b->dvout.p, b->dvout.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}
}  // extern "C"
