// The dense-iteration driver: the per-iteration schedule of smplify.py:205-213 - the point-cloud loss switched on after
// num_iters // 3, the silhouette and dense keypoint losses - around the fit kernel, and the buffers and streams it needs.
#include "bf_host.h"
#include "fit_kernels.h"
#include "mask_kernels.h"
#include "mesh_kernels.h"
#include "scan_kernels.h"
#include <chrono>

// [3NV][npf] transpose for the reverse pass (thread = pose-feature row, contiguous reads), built on the device once per model: the
// caller holds the model's lock (bf_model::lazy), and the table is finished before anybody can see the pointer (batches of the model run on
// other streams).  Used by the dense schedule and by bf_smpl_vjp.
int bf_ensure_posedirsT_locked(bf_model *m, hipStream_t stream) {
    if (m->posedirsT.p) return BF_OK;
    const size_t nv3 = (size_t)m->nv * 3;
    DevBuf<float> t;
    HIP_TRY(t.alloc((size_t)nv3 * m->npf));
    hipLaunchKernelGGL(bf_transpose_kernel, dim3((nv3 + 31) / 32, (m->npf + 31) / 32), dim3(256), 0, stream,
                       (const float *)m->posedirs.p, m->npf, (int)nv3, t.p, m->mesh.pd_pitch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    m->posedirsT.p = t.p; m->posedirsT.n = t.n; t.p = nullptr;
    return BF_OK;
}

int bf_ensure_dense_buffers(bf_batch *b) {
    bf_model *m = b->m;
    const size_t F = b->F, nv3 = (size_t)m->nv * 3;
    const int EXT = m->npf + m->nj * 12 + m->nb + 4, EXT_FULL = EXT + m->nj * 3 + 4;
    if (!b->dvout.p) {
        bool ok = b->dvout.alloc(F * nv3) == hipSuccess && b->vposed.alloc(F * nv3) == hipSuccess &&
                  b->cpts.alloc(F * nv3) == hipSuccess && b->cface.alloc(F * m->nv) == hipSuccess && !(b->cface_valid = false) &&
                  b->ext_part.alloc(F * m->mesh.n_tiles * EXT) == hipSuccess && b->ext.alloc(F * EXT_FULL) == hipSuccess &&
                  b->jraw.alloc(F * std::max(m->n_all, 1) * 3) == hipSuccess && b->lmk_vid.alloc(F * std::max(m->n_lmk, 1) * 3) == hipSuccess &&
                  b->lmk_w.alloc(F * std::max(m->n_lmk, 1) * 3) == hipSuccess &&
                  b->pc_partial.alloc(F * ((m->nv + 255) / 256)) == hipSuccess && b->pc_loss.alloc(F) == hipSuccess;
        if (!ok) return fail(BF_ERR_HIP, "dense-loss buffers: device allocation failed");
        HIP_TRY(bf_memset_sync(b->ext.p, 0, b->ext.n * sizeof(float)));
    }
    {
        std::lock_guard<std::mutex> g(m->lazy);
        BF_TRY(bf_ensure_posedirsT_locked(m, b->stream));
        for (bf_model::Sub *U : {&m->sub, &m->sub_kp}) {
            if (!U->on || U->posedirsT.p) continue;
            const size_t sv3 = (size_t)U->mesh.nv * 3;
            DevBuf<float> t;
            HIP_TRY(t.alloc(sv3 * m->npf));
            hipLaunchKernelGGL(bf_transpose_kernel, dim3((sv3 + 31) / 32, (m->npf + 31) / 32), dim3(256), 0, b->stream,
                               (const float *)U->posedirs.p, m->npf, (int)sv3, t.p, U->mesh.pd_pitch);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(b->stream));
            U->posedirsT.p = t.p; U->posedirsT.n = t.n; t.p = nullptr;
        }
    }
    return BF_OK;
}

static size_t kp_smem(const KpIO &K) {
    const int NLP = (K.nl + 31) & ~31, slots = std::max(1, 512 / NLP);
    // (the joints prologue's scratch, 32*3 + 256*3 + 4 floats, fits the head of this)
    // (+ sort keys, item weights, + the index tables staged in LDS: joint map, chain-joint CSR, selector ids)
    return sizeof(float) * std::max<size_t>(1024, (size_t)slots * NLP * 4 + (size_t)K.nl * 4 + (size_t)K.nl * 3 + 8 + 1024 + (size_t)K.nl * 3 + 16 +
                                                   (size_t)K.nl * 2 + K.nj + 1 + K.n_selector + 16);

}
static KpIO kp_io(bf_batch *b, const bf_hyper &h, const bf_model::Sub *sub = nullptr) {
    KpIO K = sub ? sub->kp : b->m->kp;
    K.n_views = b->V; K.sigma2 = h.sigma * h.sigma; K.coeff = h.imsize / 1024.0f;
    return K;
}
// (the keypoint workgroup computes the joints itself from the mesh pass's vraw / xpart: no bf_joints_kernel launch)
static int launch_kp(bf_batch *b, const bf_hyper &h, const bf_model::Sub *sub = nullptr, hipStream_t on = nullptr, int *door = nullptr) {
    const KpIO K = kp_io(b, h, sub);
    hipLaunchKernelGGL(bf_kp_loss_kernel, dim3(b->F), dim3(512), kp_smem(K), on ? on : b->stream, K, (const float *)b->jraw.p, (const float *)b->state.p,
                       (const float *)b->proj.p, (const float *)b->keypoints.p, (const int *)b->ndiv.p, (const int *)b->lmk_vid.p,
                       (const float *)b->lmk_w.p, b->ext.p, b->dvout.p, b->terms.p, sub ? sub->mesh : b->m->mesh, (const float *)b->vraw.p,
                       (const float *)b->xpart.p, door);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

int launch_mask_kernels(bf_batch *b, float weight, bool want_loss, bool sum_views, const bf_hyper *with_kp, bool projected,
                        const bf_model::Sub *sub, bool fold_acc) {
    // fold_acc: the contour scan adds its gradients into the fixed-point sums (MaskIO::acc) and the reverse mesh pass takes them from
    // there (MaskFold): no gather launch
    MaskIO K = b->masks.io;
    K.weight = weight;
    K.acc = fold_acc ? b->masks.acc.p : nullptr;
    if (sub) { K.nv = sub->mesh.nv; K.sstride = 1; }
    const int F = b->F;
    // (projected: the forward mesh pass already wrote uvi / duvb for its sampled vertices)
    if (!projected) hipLaunchKernelGGL(bf_mask_project_kernel, dim3(K.proj_blocks, K.n_masks, F), dim3(256), 0, b->stream, K, (const float *)b->vout.p,
                       (const float *)b->proj.p, b->masks.uvi.p, b->masks.duvb.p, b->masks.part.p);
    if (with_kp) {
        const KpIO Q = kp_io(b, *with_kp, sub);
        hipLaunchKernelGGL(bf_kp_contour_kernel, dim3((K.cmax * 16 + 511) / 512 + 1, K.n_masks, F), dim3(512), kp_smem(Q), b->stream, Q,
                           (const float *)b->jraw.p, (const float *)b->state.p, (const float *)b->proj.p, (const float *)b->keypoints.p,
                           (const int *)b->ndiv.p, (const int *)b->lmk_vid.p, (const float *)b->lmk_w.p, b->ext.p, b->dvout.p, b->terms.p,
                           K, (const float *)b->masks.uvi.p, b->masks.choice.p, b->masks.cgrad.p, b->masks.part.p, sub ? sub->mesh : b->m->mesh, (const float *)b->vraw.p,
                           (const float *)b->xpart.p);
    } else
    hipLaunchKernelGGL(bf_mask_contour_kernel, dim3((K.cmax * 16 + 255) / 256, K.n_masks, F), dim3(256), 0, b->stream, K,
                       (const float *)b->masks.uvi.p, b->masks.choice.p, b->masks.cgrad.p, b->masks.part.p);
    if (!fold_acc)
    hipLaunchKernelGGL(bf_mask_gather_kernel, dim3((K.ns + 63) / 64, K.n_masks, F), dim3(256), 0, b->stream, K, (const float *)b->proj.p,
                       (const float *)b->masks.uvi.p, (const float *)b->masks.duvb.p, (const int *)b->masks.choice.p,
                       (const float *)b->masks.cgrad.p, b->masks.gpart.p);
    // (sum_views = false: the reverse mesh pass adds the views itself while it loads dL/dvertices)
    if (sum_views) hipLaunchKernelGGL(bf_mask_gsum_kernel, dim3(K.proj_blocks, F), dim3(256), 0, b->stream, K, (const float *)b->masks.gpart.p, b->dvout.p);
    // (the loss VALUE is a serial sum over the partial blocks: only when somebody reads it - the fit loop needs the gradient)
    if (want_loss) hipLaunchKernelGGL(bf_mask_loss_kernel, dim3(F), dim3(64), 0, b->stream, K, (const float *)b->masks.part.p, b->masks.loss.p);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

int launch_state_and_mesh(bf_batch *b, const HyperDev &hd) {
    bf_model *m = b->m;
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(b->F), dim3(128), 0, b->stream, m->fit, (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, b->state.p,
                       (const float *)b->params.p, (const float *)b->cscale.p, hd.cscale);
    HIP_TRY(hipGetLastError());
    MeshPass mesh;
    mesh.scr = &b->scratch; mesh.n = b->F; mesh.state = b->state.p; mesh.stream = b->stream;
    mesh.vraw = b->vraw.p; mesh.vout = b->vout.p; mesh.vposed = b->vposed.p;
    return bf_launch_mesh(m, mesh);
}

// one dense iteration's forward + loss + reverse passes up to `ext` (everything except the fit kernel itself)
// (its options: DensePass below)
// BF_DOOR_COHERENT=0: the kernels that wait for the resident fit launch read its pose states with plain loads (see bf_ld_state)
// bf_mask_fold_set / BF_MASK_FOLD=gather: the silhouette's contour gradients through bf_mask_gather_kernel's ordered walk (rounds 2-4)
// instead of the contour scan's fixed-point atomic sums (MaskIO::acc)
static std::atomic<int> &mask_fold_cell() {
    static std::atomic<int> cell([] { const char *e = std::getenv("BF_MASK_FOLD"); return (e && e[0] == 'g') ? BF_MASK_FOLD_GATHER : BF_MASK_FOLD_SUMS; }());
    return cell;
}
extern "C" int bf_mask_fold_get(void) { return mask_fold_cell().load(std::memory_order_relaxed); }
extern "C" int bf_mask_fold_set(int mode) {
    if (mode != BF_MASK_FOLD_SUMS && mode != BF_MASK_FOLD_GATHER) return -1;
    mask_fold_cell().store(mode, std::memory_order_relaxed);
    return 0;
}
static bool fold_acc_on() { return bf_mask_fold_get() == BF_MASK_FOLD_SUMS; }
static bool door_coherent() { const char *e = std::getenv("BF_DOOR_COHERENT"); return !(e && e[0] == '0'); }

struct DensePass {
    bool late = false;                      // past the switch-on: the scan and silhouette losses count
    float mask_weight = 0.f;
    int *door = nullptr;                    // the persistent fit launch's doorbells and this pass's 1-based dense iteration
    int door_k = 0;                         // (null / 0: fit launches per iteration)
    // run the mesh passes on a sub-model (bf_model::Sub): the sampled-first one for fit loops without scans, the keypoint-only one for
    // the iterations before the dense losses switch on; null = the full model
    const bf_model::Sub *sub = nullptr;
    bool timed = false;                     // events between the kernel classes of this pass, for bf_batch_dense_timing
    // eval (bf_dense_iter_grad): dL/dvertices starts from zero whatever the model, the silhouette's loss value is summed, the
    // projection runs as a launch of its own (it leaves the binary term's partial sums), and dv_extra[F][NV][3] (device, full-model
    // vertex order) is added onto dL/dvertices just before the reverse mesh pass
    bool eval = false;
    const float *dv_extra = nullptr;
};
static int dense_pass(bf_batch *b, const bf_hyper &h, const HyperDev &hd, const DensePass &o) {
    bf_model *m = b->m;
    auto mark = [&](int k) -> hipError_t {
        if (!o.timed) return hipSuccess;
        if (!b->ev_dense[k]) { hipError_t e = hipEventCreate(&b->ev_dense[k]); if (e != hipSuccess) return e; }
        return hipEventRecord(b->ev_dense[k], b->stream);
    };
    HIP_TRY(mark(0));
    const MeshTab &Q = o.sub ? o.sub->mesh : m->mesh;
    const int F = b->F, nv = Q.nv, nblk = (nv + 255) / 256;
    const bool scans = o.late && !b->scans.empty(), masks = o.late && b->masks.on, kp = m->kp_dense;
    const bool acc_mode = fold_acc_on();          // (read once per pass)
    if (masks) BF_TRY(bf_masks_finalize(b));
    if (!o.door) {                     // (with the resident fit launch every state comes from it)
        hipLaunchKernelGGL(bf_pose_state_kernel, dim3(F), dim3(128), 0, b->stream, m->fit, (const float *)nullptr,
                           (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, b->state.p,
                           (const float *)b->params.p, (const float *)b->cscale.p, hd.cscale);
        HIP_TRY(hipGetLastError());
    }
    MaskProj mp;
    if (masks) {
        mp.on = 1; mp.K = b->masks.io; mp.K.weight = o.mask_weight; mp.proj = b->proj.p; mp.uvi = b->masks.uvi.p; mp.duvb = b->masks.duvb.p;
        mp.K.acc = (acc_mode && !scans) ? b->masks.acc.p : nullptr;      // (zeroed by the projection that precedes the contour scan)
        if (o.sub) { mp.K.nv = nv; mp.K.sstride = 1; }
    }
    const bool kp_aside = kp && !masks && scans && b->copy_stream;       // (see below)
    const bool kp_door = kp_aside && o.door && b->kp_door_ok;              // the join of the second stream's keypoint workgroups: doorbell or event
    if (kp_aside && !b->ev_aux[0]) {
        HIP_TRY(hipEventCreateWithFlags(&b->ev_aux[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b->ev_aux[1], hipEventDisableTiming));
    }
    MeshPass mesh;
    mesh.scr = &b->scratch; mesh.n = F; mesh.state = b->state.p; mesh.stream = b->stream;
    if (o.sub) mesh.tab = &Q;
    mesh.vraw = b->vraw.p; mesh.vout = b->vout.p; mesh.vposed = b->vposed.p;
    // (kp: the mesh pass leaves the extra-regressor partials in xpart; the joints are formed by the keypoint workgroup)
    if (kp) { mesh.xpart = b->xpart.p; mesh.want_xpart = true; }
    if (kp || masks || o.eval) mesh.dvzero = b->dvout.p;      // dL/dvertices = 0 before the keypoint / silhouette kernels add into it
    if (masks && !o.eval) mesh.mproj = &mp;
    mesh.door = o.door; mesh.door_target = (F * o.door_k) | (door_coherent() ? 0x40000000 : 0);
    if (kp_aside) mesh.mesh_done = b->ev_aux[0];            // (the fork completes with the mesh dispatch itself where it can)
    MeshPassDone did;
    int rc = bf_launch_mesh(m, mesh, did);
    if (rc) return rc;
    const bool zeroed = did.zeroed, projected = did.projected, forked = did.mesh_done_set;
    if ((kp || masks || o.eval) && !zeroed) HIP_TRY(hipMemsetAsync(b->dvout.p, 0, b->dvout.n * sizeof(float), b->stream));
    HIP_TRY(mark(1));                         // [0,1] pose state (when not resident) + forward mesh pass
    // The dense keypoint loss and the closest-point search both only read the mesh: with scans attached the keypoint workgroups (one
    // per frame, a ~25 us latency chain) run on the batch's second stream UNDER the search - that stream is idle during a dense loop
    // and, being on another priority, has a hardware queue of its own - and are joined before bf_pc_grad_kernel adds onto their
    // dL/dvertices.
    // (With a silhouette loss instead the keypoint workgroups ride in the contour launch: taking them out onto the second stream was
    //  measured slower - 0.093 vs 0.085 ms per iteration - the fork / join costs more than the 7 us the merged launch waits for them.)
    if (kp_aside) {
        // (the fork: the mesh dispatch's own completion signal when it could carry one - a record here is a marker packet between the
        //  mesh pass and the search, ~4 us of the batch stream's time per iteration)
        if (!forked || !zeroed) HIP_TRY(hipEventRecord(b->ev_aux[0], b->stream));
        HIP_TRY(hipStreamWaitEvent(b->copy_stream, b->ev_aux[0], 0));
        // (the join: with the resident launch's doorbells at hand the keypoint workgroups count themselves off there and
        //  bf_pc_grad_kernel waits for the count - BF_DOOR_KP; without them an event on the second stream and a wait on this one)
        //  The doorbell join needs the second stream's kernels to RUN while bf_pc_grad_kernel's workgroups spin on the batch stream: it is
        //  used only when ensure_fit_stream's second probe has shown that pair of streams side by side (kp_door_ok; BF_KP_JOIN=event
        //  forces the stream-level join) - the event join cannot fail that way.
        rc = launch_kp(b, h, o.sub, b->copy_stream, kp_door ? o.door : nullptr);
        if (rc) return rc;
        if (kp_door) b->kp_tickets += F;
        else HIP_TRY(hipEventRecord(b->ev_aux[1], b->copy_stream));
    } else if (kp && !masks) { rc = launch_kp(b, h, o.sub); if (rc) return rc; }
    // with a scan as well, bf_pc_grad_kernel adds onto (keypoints + silhouette): keep that order of additions
    const bool fold_views = masks && !scans;
    const bool fold_acc = fold_views && acc_mode;
    if (masks) { rc = launch_mask_kernels(b, o.mask_weight, o.eval, !fold_views, kp ? &h : nullptr, projected, o.sub, fold_acc); if (rc) return rc; }
    HIP_TRY(mark(2));                         // [1,2] keypoint loss (on this stream) and / or the silhouette kernels
    if (scans) {
        bf_nearest_launch(dim3((nv + 3) / 4, F), b->stream, (const ScanDev *)b->scan_dev.p,
                          (const float *)b->vout.p, nv, b->cface.p, b->cpts.p, (float *)nullptr, b->cface_valid ? 1 : 0);   // (one wave per query; warm start from the previous call's faces)
        b->cface_valid = true;
        HIP_TRY(mark(3));                     // [2,3] closest-point search
        hipLaunchKernelGGL(bf_pc_partial_kernel, dim3(nblk, F), dim3(256), 0, b->stream, (const float *)b->vout.p,
                           (const float *)b->cpts.p, nv, b->pc_partial.p);
        if (kp_aside && !kp_door) HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_aux[1], 0));
        hipLaunchKernelGGL(bf_pc_grad_kernel, dim3(nblk, F), dim3(256), 0, b->stream, (const float *)b->vout.p,
                           (const float *)b->cpts.p, nv, (const float *)b->pc_partial.p, (const float *)b->pc_weight.p,
                           b->dvout.p, b->pc_loss.p, (kp || masks) ? 1 : 0, kp_door ? o.door : (int *)nullptr, b->kp_tickets);
    }
    if (!scans) HIP_TRY(mark(3));
    if (o.dv_extra) {
        hipLaunchKernelGGL(bf_dv_add_kernel, dim3((nv * 3 + 255) / 256, F), dim3(256), 0, b->stream, b->dvout.p, o.dv_extra,
                           o.sub ? (const int *)o.sub->verts.p : (const int *)nullptr, nv, m->nv);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(mark(4));                         // [3,4] point-cloud loss + gradient (+ the join with the keypoint workgroups of the second stream)
    const int EXT = m->npf + m->nj * 12 + m->nb + 4;
    int part_rows = Q.n_tiles;             // (two per tile when the reverse pass splits its tiles: one frame, a small grid)
    {
        MaskFold fold = {};
        if (fold_acc) { fold.acc = b->masks.acc.p; fold.uvi = b->masks.uvi.p; fold.duvb = b->masks.duvb.p; fold.proj = b->proj.p; fold.view_index = b->masks.io.view_index; fold.n_views = b->V; }
        const int e = bf_mesh_bwd_multi_launch(&Q, o.sub ? o.sub->posedirsT.p : m->posedirsT.p, b->state.p, F, b->dvout.p, b->vposed.p, b->vraw.p, b->ext_part.p,
                                               b->stream, (fold_views && !fold_acc) ? (const float *)b->masks.gpart.p : nullptr, b->masks.io.n_masks, b->masks.io.ns, o.sub ? 1 : 4,
                                               (o.sub && o.sub == &m->sub_kp) ? Q.n_tiles : m->mesh.n_tiles, &part_rows, fold_acc ? &fold : nullptr);      // (keypoint-only sub-model: no tile split - a batch of 8 and its single frames keep the same partial sums)
        if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_bwd_multi_kernel: ") + hipGetErrorString((hipError_t)e));
    }
    HIP_TRY(mark(5));                         // [4,5] reverse mesh pass
    hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((EXT + BF_RED_COLS - 1) / BF_RED_COLS, F), dim3(8 * BF_RED_COLS), 0, b->stream,
                       (const float *)b->ext_part.p, part_rows, EXT, b->ext.p, EXT + m->nj * 3 + 4, o.door, o.door_k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(6));                         // [5,6] reduction of the partial blocks (rings the resident fit launch)
    if (o.timed) b->dense_timed = true;
    return BF_OK;
}

// FitTab::lds_image of the model's dense-schedule fit instance: one launch in mode 2 runs the kernel's ordinary prologue and
// dumps the LDS segment (everything up to the per-view projection matrices, which come last in the carve).  Built once per
// model, under its lock, finished before the pointer becomes visible.
int bf_ensure_fit_image(bf_batch *b, FrameIO io, const HyperDev &hd) {
    bf_model *m = b->m;
    std::lock_guard<std::mutex> g(m->lazy);
    if (m->fit.lds_image) return BF_OK;
    int seg[6];
    bf_fit_image_segments(m->fit.nj, m->fit.nb, m->fit.npf, m->fit.ns, m->fit.nl, m->fit.np, seg);
    const size_t bytes = (size_t)(seg[4] + seg[5] + 2 * ((m->fit.np + 3) / 4)) * 16;      // up to the end of am / av: everything before proj
    FitTab T = m->fit;
    T.lds_image_n4 = (int)(bytes / 16);
    HIP_TRY(m->fit_image.alloc(bytes / sizeof(float)));
    io.ext = nullptr; io.image_out = m->fit_image.p; io.n_frames = 1;      // (the carve, hence the image, is the same for every instance of the model's sizes)
    HIP_TRY(bf_fit_launch(&T, &io, &hd, 1, 2, b->adam_tab.p, 0, b->fit_smem, b->stream, nullptr));
    HIP_TRY(hipStreamSynchronize(b->stream));
    m->fit.lds_image_n4 = T.lds_image_n4;
    bf_fit_image_segments(m->fit.nj, m->fit.nb, m->fit.npf, m->fit.ns, m->fit.nl, m->fit.np, &m->fit.img_seg[0][0]);
    std::atomic_thread_fence(std::memory_order_release);      // (launches on other threads copy m->fit without the lock: sizes before the pointer)
    m->fit.lds_image = m->fit_image.p;
    return BF_OK;
}

// First use of the resident fit launch on a batch: its stream (highest priority), events, doorbells, the warm-up launch and the
// self-test that the fit stream really runs beside the batch stream (b->door_usable).
static int ensure_fit_stream(bf_batch *b, const FrameIO &io, const HyperDev &hd) {
    if (b->fit_stream) return BF_OK;
    bf_model *m = b->m;
    // the fit stream gets the highest priority: the runtime keeps a pool of hardware queues per priority, so it does not end
    // up on the queue of this (or another) batch's ordinary stream - where the dense kernels would queue up BEHIND the
    // resident launch that is waiting for them
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamCreateWithPriority(&b->fit_stream, hipStreamNonBlocking, greatest));
    HIP_TRY(hipEventCreateWithFlags(&b->ev_door[0], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&b->ev_door[1], hipEventDisableTiming));
    HIP_TRY(b->door.alloc(BF_DOOR_INTS));
    HIP_TRY(hipHostMalloc((void **)&b->h_door_err, sizeof(int)));
    HIP_TRY(hipHostMalloc((void **)&b->h_resident, sizeof(int)));
    *b->h_door_err = 0;
    // first use of the new stream: its queue, the kernel's code object and scratch come up now, not under a mesh pass that is
    // already waiting for this launch (mode 2 = prologue only)
    FrameIO iow = io;
    iow.ext = b->ext.p; iow.image_out = nullptr; iow.n_frames = 1;
    HIP_TRY(bf_fit_launch(&m->fit, &iow, &hd, 1, 2, b->adam_tab.p, 0, b->fit_smem, b->fit_stream, nullptr));
    HIP_TRY(hipStreamSynchronize(b->fit_stream));
    // ... and checked: do the two streams really run side by side? (bf_door_probe_kernel)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(bf_memset_sync(b->door.p, 0, BF_DOOR_STATE * sizeof(int)));
    hipLaunchKernelGGL(bf_door_probe_kernel, dim3(1), dim3(64), 0, b->fit_stream, b->door.p);
    hipLaunchKernelGGL(bf_door_ring_kernel, dim3(1), dim3(64), 0, b->stream, b->door.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->fit_stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    int verdict = 0;
    HIP_TRY(hipMemcpy(&verdict, b->door.p + BF_DOOR_TICKET, sizeof(int), hipMemcpyDeviceToHost));
    b->door_usable = verdict == 1;
    // the same question for the pair (batch stream, second stream): config 5's keypoint workgroups run on the second stream and are
    // joined by a doorbell that bf_pc_grad_kernel's workgroups wait on (BF_DOOR_KP) - only if that stream's kernels run beside them
    b->kp_door_ok = false;
    const char *kj = getenv("BF_KP_JOIN");
    if (b->door_usable && b->copy_stream && !(kj && kj[0] == 'e')) {
        HIP_TRY(hipStreamSynchronize(b->copy_stream));
        HIP_TRY(bf_memset_sync(b->door.p, 0, BF_DOOR_STATE * sizeof(int)));
        hipLaunchKernelGGL(bf_door_probe_kernel, dim3(1), dim3(64), 0, b->stream, b->door.p);
        hipLaunchKernelGGL(bf_door_ring_kernel, dim3(1), dim3(64), 0, b->copy_stream, b->door.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(b->stream));
        HIP_TRY(hipStreamSynchronize(b->copy_stream));
        int v2 = 0;
        HIP_TRY(hipMemcpy(&v2, b->door.p + BF_DOOR_TICKET, sizeof(int), hipMemcpyDeviceToHost));
        b->kp_door_ok = v2 == 1;
    }
    if (!b->door_usable) {
        // said once per process: the dense loops still give the same results, about three times slower (one fit launch per iteration)
        static std::atomic<bool> told{false};
        if (!told.exchange(true))
            std::fprintf(stderr, "libbodyfit: the resident fit launch is off - its stream shares a hardware queue with the batch stream (self-test "
                                 "verdict %d).  The dense loops (use_mask / use_mesh / SMPL-X) fall back to one fit launch per iteration: same "
                                 "results, ~3x slower.  HIP multiplexes a process's streams over the hardware queues GPU_MAX_HW_QUEUES allows; "
                                 "fewer streams elsewhere in the process leave more of them to the batch.\n", verdict);
    }
    return BF_OK;
}

// what every dense pass of a call reads besides the batch's own buffers: the scans' weights, the silhouette's image size and distance form
static int dense_prepare(bf_batch *b, const bf_hyper &h) {
    const int F = b->F;
    if (!b->scans.empty()) {
        // 5 * imsize / scan_height (smplify.py:206,210) of the scans attached NOW and of THIS call's imsize: F floats, staged in
        // pinned memory and copied on the batch's stream (a reused batch gets new scans on every SMPLify.__call__)
        if (b->pc_weight.n != (size_t)F) {
            if (b->pc_weight.p) { HIP_TRY(hipStreamSynchronize(b->stream)); (void)hipFree(b->pc_weight.p); b->pc_weight.p = nullptr; }
            HIP_TRY(b->pc_weight.alloc(F));
        }
        if (!b->h_pc_weight) HIP_TRY(hipHostMalloc((void **)&b->h_pc_weight, (size_t)F * sizeof(float)));
        else HIP_TRY(hipStreamSynchronize(b->stream));      // (an earlier call's copy may still be reading the staging buffer)
        for (int f = 0; f < F; ++f) b->h_pc_weight[f] = 5.0f * h.imsize / b->scans[f]->dev.height;
        HIP_TRY(hipMemcpyAsync(b->pc_weight.p, b->h_pc_weight, (size_t)F * sizeof(float), hipMemcpyHostToDevice, b->stream));
    }
    if (b->masks.on) { b->masks.io.imsize = h.imsize; b->masks.io.cdist = h.mask_cdist_form != 0.f; }
    return bf_ensure_dense_buffers(b);
}

// the sub-models of a fit loop's dense iterations: before (early) and after (late) the silhouette / scan losses switch on
static void dense_subs(bf_batch *b, const bf_model::Sub *&sub_early, const bf_model::Sub *&sub_late) {
    bf_model *m = b->m;
    // (read on every call: a test switches them between two calls of one process)
    const bool sub_ok = [] { const char *e = std::getenv("BF_DENSE_SUBMODEL"); return !(e && e[0] == '0'); }();
    // (the sub-model of iteration `it`: before the dense losses switch on only the keypoint loss's vertices matter - with or without scans)
    sub_late = (sub_ok && m->sub.on && b->scans.empty()) ? &m->sub : nullptr;
    const bool sub_kp_ok = [] { const char *e = std::getenv("BF_DENSE_SUBMODEL_KP"); return !(e && e[0] == '0'); }();      // (bring-up switch, like BF_DENSE_SUBMODEL)
    // With silhouettes attached too (round 6; BF_DENSE_SUBMODEL_KP_MASKS=0 keeps rounds 4-5's schedule): the iterations before the
    // silhouette switches on run on the 899 keypoint vertices instead of the 3,285 sampled-first ones - another summation order of those
    // mesh passes, nothing else (`test_sub_model_loop_matches_the_full_model_loop`: 2e-5 at the switch).  Round 5 left it out because
    // the chaotic end state moved from 1.9 % to 3.9 % of the reference's, outside a band that was 3 x the larger of TWO perturbed
    // reference runs; round 6 measures the reference under ten perturbations (tests/ref_drift.py).
    const bool sub_kp_masks = [] { const char *e = std::getenv("BF_DENSE_SUBMODEL_KP_MASKS"); return !(e && e[0] == '0'); }();
    sub_early = (sub_ok && sub_kp_ok && m->sub_kp.on && (!b->masks.on || sub_kp_masks)) ? &m->sub_kp : sub_late;
}

// a call that fails while the fit launch is resident: let everybody through (BF_DOOR_ERR) and wait for the launch, so that it is not
// left waiting for bells that will not ring
static void door_release(bf_batch *b) {
    const int one = 1;
    (void)hipMemcpy(b->door.p + BF_DOOR_ERR, &one, sizeof one, hipMemcpyHostToDevice);
    (void)hipStreamSynchronize(b->fit_stream);
}

// the loop of smplify.py:177-213 when a dense loss is present (use_mask, use_mesh, or the SMPL-X keypoints
// with hands + face): iterations that need no dense loss run as one persistent launch; every other iteration
// is state -> mesh -> losses -> reverse mesh pass -> one fit-kernel iteration (smplify.py:197-210).
int bf_fit_with_scans(bf_batch *b, int n_iters, const bf_hyper &h, const HyperDev &hd, FrameIO io) {
    bf_model *m = b->m;
    // iterations of THIS call that run before the dense losses switch on: local index it <= thr
    const int F = b->F, thr = h.dense_after < 0.f ? n_iters / 3 : (int)h.dense_after - b->steps_done;
    const int n_plain = m->kp_dense ? 0 : std::max(0, std::min(n_iters, thr + 1));
    int rc = dense_prepare(b, h);
    if (rc) return rc;
    if (n_plain > 0)
        HIP_TRY(bf_fit_launch(&m->fit, &io, &hd, n_plain, 0, b->adam_tab.p, b->steps_done, b->fit_smem, b->stream, nullptr));
    if (n_plain < n_iters) { rc = bf_ensure_fit_image(b, io, hd); if (rc) return rc; }
    // The dense iterations with the fit kernel RESIDENT (one launch on a second stream, paced by doorbells, BfDoor) when the
    // forward pass is a kernel that knows how to wait (1..15 frames); BF_DENSE_PERSISTENT=0, or a larger batch, keeps one fit launch
    // per iteration, with the pose state from bf_pose_state_kernel every time.
    const bf_model::Sub *sub_early = nullptr, *sub_late = nullptr;
    dense_subs(b, sub_early, sub_late);
    const bool door_ok = [] { const char *e = std::getenv("BF_DENSE_PERSISTENT"); return !(e && e[0] == '0'); }();
    const int n_dense = n_iters - n_plain;
    DensePass pass;
    pass.mask_weight = 5.0f;                                            // smplify.py:210
    auto pass_of = [&](int it) -> const DensePass & {
        pass.late = it > thr; pass.sub = it > thr ? sub_late : sub_early; pass.timed = b->dense_timing && it == n_iters - 1;
        return pass;
    };
    if (door_ok && n_dense >= 1 && F < BF_MFMA_MIN_FRAMES) { rc = ensure_fit_stream(b, io, hd); if (rc) return rc; }
    if (n_dense >= 1) b->dense_resident = (door_ok && F < BF_MFMA_MIN_FRAMES && b->door_usable) ? 1 : 0;
    if (door_ok && n_dense >= 1 && F < BF_MFMA_MIN_FRAMES && b->door_usable) {
        *(volatile int *)b->h_resident = 0;
        HIP_TRY(hipMemsetAsync(b->door.p, 0, BF_DOOR_INTS * sizeof(int), b->stream));
        b->kp_tickets = 0;
        HIP_TRY(hipEventRecord(b->ev_door[0], b->stream));              // parameters / Adam state / doorbells as the loop finds them
        HIP_TRY(hipStreamWaitEvent(b->fit_stream, b->ev_door[0], 0));
        FrameIO io2 = io;
        io2.ext = b->ext.p; io2.door = b->door.p; io2.door_resident = b->h_resident;
        HIP_TRY(bf_fit_launch(&m->fit, &io2, &hd, n_dense, 0, b->adam_tab.p, b->steps_done + n_plain, b->fit_smem, b->fit_stream, nullptr));
        HIP_TRY(hipEventRecord(b->ev_door[1], b->fit_stream));
        for (int it = n_plain; it < n_iters; ++it) {
            if (it == n_plain) {
                // the mesh passes WAIT for the fit launch: every one of its workgroups must be running before such a
                // pass can fill the machine
                const auto t0 = std::chrono::steady_clock::now();
                while (*(volatile int *)b->h_resident < F) {
                    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                        door_release(b);
                        return fail(BF_ERR_HIP, "dense schedule: the persistent fit launch did not start");
                    }
                }
            }
            pass.door = b->door.p; pass.door_k = it - n_plain + 1;
            rc = dense_pass(b, h, hd, pass_of(it));
            if (rc) { door_release(b); return rc; }
        }
        HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_door[1], 0));       // the last iteration's step, terms and state
        HIP_TRY(hipMemcpyAsync(b->h_door_err, b->door.p + BF_DOOR_ERR, sizeof(int), hipMemcpyDeviceToHost, b->stream));
        return BF_OK;
    }
    for (int it = n_plain; it < n_iters; ++it) {
        rc = dense_pass(b, h, hd, pass_of(it));
        if (rc) return rc;
        FrameIO io2 = io;
        io2.ext = b->ext.p;
        HIP_TRY(bf_fit_launch(&m->fit, &io2, &hd, 1, 0, b->adam_tab.p, b->steps_done + it, b->fit_smem, b->stream, nullptr));
    }
    return BF_OK;
}

extern "C" {
int bf_batch_dense_resident(const bf_batch *b) { return b ? b->dense_resident : -1; }

int bf_batch_dense_timing(bf_batch *b, int enable, float ms[6]) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_dense_timing: null batch");
    HIP_TRY(hipSetDevice(b->m->device));
    if (ms) {
        if (!b->dense_timed) return fail(BF_ERR_INVALID, "bf_batch_dense_timing: no dense iteration has been timed (enable, then bf_fit with a dense loss)");
        BF_TRY(bf_sync_all(b));
        for (int k = 0; k < 6; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], b->ev_dense[k], b->ev_dense[k + 1]));
    }
    b->dense_timing = enable != 0;
    return BF_OK;
}
}  // extern "C"

// bf_loss_grad for models whose keypoint loss is dense (SMPL-X): one evaluation, no update
int bf_dense_loss_grad(bf_batch *b, const bf_hyper &h, const HyperDev &hd, FrameIO io) {
    int rc = bf_ensure_dense_buffers(b);
    if (rc) return rc;
    DensePass pass;
    pass.mask_weight = 5.0f;
    rc = dense_pass(b, h, hd, pass);
    if (rc) return rc;
    io.ext = b->ext.p;
    HIP_TRY(bf_fit_launch(&b->m->fit, &io, &hd, 1, 1, b->adam_tab.p, 0, b->fit_smem, b->stream, nullptr));
    return BF_OK;
}

// bf_dense_iter_grad: what one dense iteration of bf_fit_with_scans hands to Adam, evaluated without the update (launch-per-iteration
// route, no doorbells).  terms6[6] per frame on the host, or null.
int bf_dense_iter_eval(bf_batch *b, const bf_hyper &h, const HyperDev &hd, FrameIO io, bool late, bool use_sub, const float *dverts_extra,
                       float *terms6) {
    bf_model *m = b->m;
    const int F = b->F;
    int rc = dense_prepare(b, h);
    if (rc) return rc;
    const bool scans = late && !b->scans.empty(), masks = late && b->masks.on;
    const bf_model::Sub *sub = nullptr;
    if (use_sub) {
        const bf_model::Sub *sub_early = nullptr, *sub_late = nullptr;
        dense_subs(b, sub_early, sub_late);
        sub = late ? sub_late : sub_early;
    }
    DevBuf<float> extra;
    if (dverts_extra) HIP_TRY(extra.upload(dverts_extra, (size_t)F * m->nv * 3));
    // the closest-point search warm-starts from the faces of the call before it: this call keeps them as it found them
    DevBuf<int> faces_kept;
    const bool warm = b->cface_valid;
    if (scans && warm) {
        HIP_TRY(faces_kept.alloc(b->cface.n));
        HIP_TRY(hipMemcpyAsync(faces_kept.p, b->cface.p, b->cface.n * sizeof(int), hipMemcpyDeviceToDevice, b->stream));
    }
    DensePass pass;
    pass.late = late; pass.mask_weight = 5.0f; pass.sub = sub;
    pass.eval = true; pass.dv_extra = extra.p;
    rc = dense_pass(b, h, hd, pass);
    if (rc) return rc;
    if (scans) {
        if (warm) HIP_TRY(hipMemcpyAsync(b->cface.p, faces_kept.p, b->cface.n * sizeof(int), hipMemcpyDeviceToDevice, b->stream));
        b->cface_valid = warm;
    }
    io.ext = b->ext.p;
    HIP_TRY(bf_fit_launch(&m->fit, &io, &hd, 1, 1, b->adam_tab.p, 0, b->fit_smem, b->stream, nullptr));
    BF_TRY(bf_sync_all(b));
    if (terms6) {
        std::vector<float> t4((size_t)F * 4), mk(F, 0.f), pc(F, 0.f);
        HIP_TRY(hipMemcpy(t4.data(), b->terms.p, t4.size() * sizeof(float), hipMemcpyDeviceToHost));
        if (masks) HIP_TRY(hipMemcpy(mk.data(), b->masks.loss.p, (size_t)F * sizeof(float), hipMemcpyDeviceToHost));
        if (scans) HIP_TRY(hipMemcpy(pc.data(), b->pc_loss.p, (size_t)F * sizeof(float), hipMemcpyDeviceToHost));
        for (int f = 0; f < F; ++f) {
            std::copy(t4.begin() + (size_t)f * 4, t4.begin() + (size_t)f * 4 + 4, terms6 + (size_t)f * 6);
            terms6[(size_t)f * 6 + 4] = 5.0f * mk[f];
            terms6[(size_t)f * 6 + 5] = pc[f];          // (bf_pc_grad_kernel leaves weight * norm)
        }
    }
    return BF_OK;
}
