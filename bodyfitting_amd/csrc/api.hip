// Host side of libbodyfit: the C ABI of include/bodyfit.h over the gfx950 kernels.
#include "lanes.h"
#include "fit_kernels.h"
#include "mesh_kernels.h"
#include "mesh_choice.h"
#include <cassert>
#include <chrono>


// The HIP runtime multiplexes all streams of a process over its hardware queues, and streams that share a queue run in order.  A batch
// uses up to three streams that must run side by side (batch stream; second stream for a call's mesh tail / the side kernels of a dense
// iteration; the resident fit launch's stream).  How many queues a process gets is the host's setting (GPU_MAX_HW_QUEUES): the library
// never changes it.  When the resident launch shares a queue with the batch stream its self-test fails and every dense iteration pays a
// fit launch instead - same results, slower (dense_api.hip).

std::string &bf_err_slot() { thread_local std::string e; return e; }
int bf_fail(int code, const std::string &msg) { bf_err_slot() = msg; return code; }

// Host time spent inside bf_batch_stage_inputs and bf_fit, summed per batch and printed when the batch goes - a build-time switch, so
// that the product build carries no timers: make variant TAG=timers VSRC=api VFLAGS=-DBF_HOST_TIMERS (profiles/lane_feed.md)
#ifdef BF_HOST_TIMERS
struct BfHostSums { long long ns[2] = {0, 0}, n[2] = {0, 0}; };
static std::mutex &host_sums_mu() { static std::mutex mu; return mu; }      // (batches of a group are driven from several threads)
static std::map<const void *, BfHostSums> &host_sums() { static std::map<const void *, BfHostSums> s; return s; }
static BfHostSums *host_sums_of(const void *b) { std::lock_guard<std::mutex> lk(host_sums_mu()); return &host_sums()[b]; }      // (node addresses are stable)
struct BfHostTimed {
    static constexpr long long kSkip = 16;
    BfHostSums *s; int k;
    std::chrono::steady_clock::time_point t0;
    BfHostTimed(const void *b, int k_) : s(b ? host_sums_of(b) : nullptr), k(k_), t0(std::chrono::steady_clock::now()) {}
    ~BfHostTimed() {
        if (!s) return;
        const long long dt = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (++s->n[k] > kSkip) s->ns[k] += dt;          // (the first calls create lanes, events and tables)
    }
};
static void host_sums_report(const void *b) {
    std::lock_guard<std::mutex> lk(host_sums_mu());
    auto it = host_sums().find(b);
    if (it == host_sums().end()) return;
    const BfHostSums &s = it->second;
    const long long n0 = s.n[0] - BfHostTimed::kSkip, n1 = s.n[1] - BfHostTimed::kSkip;
    std::fprintf(stderr, "BF_HOST_TIMERS batch %p: bf_batch_stage_inputs %lld calls %.3f us each; bf_fit %lld calls %.3f us each (first %lld of each left out)\n",
                 b, s.n[0], n0 > 0 ? s.ns[0] * 1e-3 / n0 : 0.0, s.n[1], n1 > 0 ? s.ns[1] * 1e-3 / n1 : 0.0, BfHostTimed::kSkip);
    host_sums().erase(it);
}
#define BF_HOST_TIMED(b, k) BfHostTimed host_timed_((b), (k))
#else
#define BF_HOST_TIMED(b, k) do { } while (0)
#endif

static_assert(kBfMeshMfmaMinFrames == BF_MFMA_MIN_FRAMES && kBfMeshBatch32MaxFrames == BF_BATCH32_MAX_FRAMES, "mesh_choice.h repeats bf_internal.h's thresholds");

extern "C" {

const char *bf_last_error(void) { return bf_err_slot().c_str(); }
const char *bf_version(void) { return "bodyfit-mi355x 0.1 (gfx950)"; }

int bf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void bf_hyper_default(bf_hyper *h) {
    if (!h) return;
    h->sigma = 100.f;
    h->pose_prior_weight = 4.78f;
    h->angle_prior_weight = 15.2f;
    h->shape_prior_weight = 5.f;
    h->constant_scale = 0.3f;
    h->imsize = 512.f;
    h->lr = 1e-2f;
    h->lr_transl_scale = 0.1f;
    h->adam_beta1 = 0.9f;
    h->adam_beta2 = 0.999f;
    h->adam_eps = 1e-8f;
    h->lr_displacement = 5e-2f;
    h->mask_cdist_form = 1.f;
    h->dense_after = -1.f;
}

}  // extern "C"
int bf_launch_mesh(bf_model *m, const MeshPass &p, MeshPassDone &told) {
    told = MeshPassDone{};
    const int n = p.n;
    const hipStream_t stream = p.stream;
    float *const xpart = (p.joints || p.joints_ori || p.jraw || p.want_xpart) ? p.xpart : nullptr;
    const MeshTab &Q = p.tab ? *p.tab : m->mesh;          // (the sampled-first sub-model inside a dense loop without scans)
    dim3 grid(Q.n_tiles, n);
    const float *pose_off = nullptr;
    // which kernel, in how many passes (mesh_choice.h).  A fit-lane group (p.per) of calls below the matrix-core threshold is ONE launch of
    // the multi-frame kernel over all its frames: a tile's posedirs slice is streamed once per eight frames, not once per frame
    // (bf_mesh_kernel's grid (tiles, frames)) or once per call; the kernels do the same arithmetic in the same order per frame, and the
    // group's state, vertex and extra-joint partial arrays are frame-major and contiguous, which is how the kernel indexes them
    // ((frame, tile, extra) for xpart).  A group of larger calls gets a pass per call, each the matrix-core kernel the call gets alone.
    const bool group = p.per > 0 && p.per < n;
    // the arena's pinned mirror, for the kernels that store to it themselves (the plain and the multi-frame kernel): a pass that hands over
    // is a result pass - vertices and mapped joints into an arena - with no doorbell, sub-model table or vposed
    const BfHandOver *const ho = (p.mirror && p.vout && p.joints && !p.door && !p.tab && !p.vposed) ? p.mirror : nullptr;
    bool mirrored = false;
    assert(bf_mesh_choice_multi(m->npf, 1) == (bf_mesh_use_multi(m->npf, 1) != 0) && "mesh_choice.h and bf_mesh_use_multi agree on the single-frame kernel");
    const BfMeshChoice ch = bf_mesh_choice(p.per, n, m->npf, p.tab != nullptr, (p.vposed ? BF_MESH_CHOICE_VPOSED : 0u) |
                                           (bf_mesh_batch32_fits(&m->mesh) ? BF_MESH_CHOICE_BATCH32_FITS : 0u));
    if (group && n % p.per) return fail(BF_ERR_INVALID, "bf_launch_mesh: a grouped pass carries whole calls only");
    if (ch.passes > 1) {
        if (p.vposed || p.dvzero || p.mproj || p.door || p.mesh_done)
            return fail(BF_ERR_INVALID, "bf_launch_mesh: a grouped pass carries the result mesh of whole calls only");
        MeshPass q = p;
        q.per = 0; q.n = ch.frames; q.joints = q.joints_ori = q.jraw = nullptr; q.want_xpart = xpart != nullptr; q.after_mesh = nullptr;
        q.mirror = nullptr;                               // (calls of 16 frames and more: the matrix-core kernels, which leave the hand-over to a copy command)
        const size_t s_state = bf_state_stride(m->nj, m->npf, m->nb), s_v = (size_t)m->nv * 3, s_x = (size_t)Q.n_tiles * Q.n_extra * 3;
        for (int c = 0; c < ch.passes; ++c) {
            const size_t f0 = (size_t)c * ch.frames;
            q.state = p.state + f0 * s_state; q.vraw = p.vraw + f0 * s_v; q.vout = p.vout ? p.vout + f0 * s_v : nullptr;
            q.xpart = p.xpart ? p.xpart + f0 * s_x : nullptr;
            BF_TRY(bf_launch_mesh(m, q));
        }
    } else if (ch.kernel == BfMeshKernel::BATCH32) {
        // one or two 32-frame blocks: pose blend on the matrix cores with the epilogue behind the accumulators, ONE launch
        // (13.4 us instead of 4.6 + 15.5 + 14.5 at 32 frames; from 128 frames on the 128-frame GEMM tile below wins)
        HIP_TRY(bf_mesh_batch32_launch(&m->mesh, p.state, n, p.vraw, p.vout, xpart, stream));
    } else if (ch.kernel == BfMeshKernel::GEMM) {
        // batched pose blend on the matrix cores (posedirs streamed once for up to 256 frames), then the per-frame
        // shape / skinning part only
        const size_t ncols = (size_t)m->nv * 3;
        MeshScratch *scr = p.scr;
        if (!scr) return fail(BF_ERR_INVALID, "bf_launch_mesh: the batched path needs a scratch owner");
        // (the scratch belongs to this stream's owner, so draining this stream is enough before a buffer is replaced)
        HIP_TRY(bf_grow(stream, scr->pose_off, (size_t)n * ncols));
        // A operand of the GEMM: the pose features of the batch, frame-minor and zero padded
        const int kpad = ((m->npf + 2 * BF_GEMM_KB - 1) / (2 * BF_GEMM_KB)) * 2 * BF_GEMM_KB, fpad = ((n + 127) / 128) * 128;
        HIP_TRY(bf_grow(stream, scr->featT, (size_t)kpad * fpad));
        HIP_TRY(bf_poseblend_launch(&m->mesh, p.state, n, scr->featT.p, kpad, fpad, scr->pose_off.p, stream));
        pose_off = scr->pose_off.p;
        if (m->mesh.v_nnz == 4 && m->nb <= 12 && !p.vposed) {
            bf_mesh_epilogue_batch_launch(&m->mesh, p.state, pose_off, n, p.vraw, p.vout, xpart, stream);
        } else
        hipLaunchKernelGGL(bf_mesh_epilogue_kernel, grid, dim3(128), 0, stream, m->mesh, p.state, pose_off, p.vraw, p.vout, xpart, p.vposed);
    } else if (ch.kernel == BfMeshKernel::MULTI) {
        const int e = bf_mesh_multi_launch(&Q, p.state, n, p.vraw, p.vout, xpart, p.vposed, p.dvzero, stream, p.mproj, p.door, p.door_target,
                                           p.mesh_done, ho ? ho->vout : nullptr);
        if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_multi_kernel: ") + hipGetErrorString((hipError_t)e));
        told.mesh_done_set = p.mesh_done != nullptr;          // (the event completes with the mesh dispatch: the caller records nothing)
        told.projected = p.mproj != nullptr;
        told.zeroed = p.dvzero != nullptr;
        mirrored = ho != nullptr;
    } else {
        hipLaunchKernelGGL(bf_mesh_kernel, grid, dim3(BF_MESH_TILE * 3 * BF_MESH_RG), m->mesh_smem, stream, Q,
                           p.state, p.vraw, p.vout, xpart, p.vposed, pose_off, p.door, p.door_target, ho ? ho->vout : (float *)nullptr);
        mirrored = ho != nullptr;
    }
    HIP_TRY(hipGetLastError());
    if (p.after_mesh) HIP_TRY(hipEventRecord(p.after_mesh, stream));
    if (p.joints || p.joints_ori || p.jraw) {
        hipLaunchKernelGGL(bf_joints_kernel, dim3(n), dim3(256), 0, stream, Q, p.state, (const float *)p.vraw,
                           (const float *)p.xpart, p.joints, p.joints_ori, p.jraw, p.lmk_vid, p.lmk_w, mirrored ? *ho : BfHandOver{});
        HIP_TRY(hipGetLastError());
        told.handed_over = mirrored;                      // (vertices by the mesh launch, the four small slices by this one: nothing left to copy)
    }
    return BF_OK;
}

extern "C" {
// A small fetch as a kernel: device arena -> pinned host mirror with plain stores over PCIe (posted writes, visible to the
// host when the stream drains); a copy node costs ~20 us of fixed overhead for the same 90 KB.
__global__ void __launch_bounds__(256) __attribute__((visibility("hidden"))) bf_publish_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

}  // extern "C"
int bf_publish(hipStream_t stream, float *dst, const float *src, size_t n_floats) {      // (slices are 256-byte multiples: float4 clean)
    const size_t n4 = n_floats / 4;
    hipLaunchKernelGGL(bf_publish_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 64)), dim3(256), 0, stream,
                       (const float4 *)src, (float4 *)dst, n4);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// the first n_floats of a result arena go to its pinned mirror: as a copy command (`big`: the caller's choice) or through the kernel above
static int hand_over(hipStream_t stream, ResultArena &r, size_t n_floats, bool big) {
    if (!big) return bf_publish(stream, r.host, r.dev.p, n_floats);
    HIP_TRY(hipMemcpyAsync(r.host, r.dev.p, n_floats * sizeof(float), hipMemcpyDeviceToHost, stream));
    return BF_OK;
}

// the result mesh of a batch: vertices and mapped joints of its F frames from their pose states into the batch's current arena, on the
// batch stream; `after_mesh`: an event recorded between the mesh and the joints pass
static int result_mesh(bf_batch *b, hipEvent_t after_mesh = nullptr) {
    MeshPass p;
    p.scr = &b->scratch; p.n = b->F; p.state = b->state.p; p.stream = b->stream;
    p.vraw = b->vraw.p; p.vout = b->vout.p; p.xpart = b->xpart.p; p.joints = b->joints.p;
    p.after_mesh = after_mesh;
    return bf_launch_mesh(b->m, p);
}

// Whether the tail of `n_frames` frames whose arena prefix is `bytes` long lets its mesh and joints kernels store into the pinned mirror
// themselves (MeshPass::mirror) instead of a hand-over behind them.  Stores over PCIe are no faster than the copy engine: a one-round
// mesh grid issues them all at its end, and the kernel then lasts its stream plus the transfer (33 -> 71 us at 32 frames).  What they
// save is the copy command's start-up behind the joints pass and a launch.  Measured, fit end to end of hand-over (profiles/lane_tail.md):
// against the copy command - 7 frames and more, 512 KB as in kLaneCopyBytes - the stores win at every size (47 -> 31 us at 7 frames,
// 104 -> 80 at 32); against the publish kernel below that they win for a lone frame (17.8 -> 14.9 us, the lone caller's round trip 479 ->
// 452 us) and tie at 2-6 frames (medians 0.6-2 us lower, not below the other's fastest): those keep the publish kernel.
static constexpr size_t kTailStoreBytes = (size_t)512 * 1024;
static bool tail_stores(const bf_batch *b, size_t bytes, int n_frames) {
    if (b->tail_handover != bf_batch::TailHandOver::BY_SIZE) return b->tail_handover == bf_batch::TailHandOver::STORE;
    return n_frames == 1 || bytes >= kTailStoreBytes;
}

// where the five slices of an arena laid out by `off` (the batch's res_off, or a lane group's) live on the device and in the pinned mirror
static BfHandOver arena_mirror(const bf_batch *b, const ResultArena &r, const size_t off[5]) {
    BfHandOver ho;
    ho.d_params = r.dev.p + off[0]; ho.d_terms = r.dev.p + off[1];
    ho.params = r.host + off[0]; ho.terms = r.host + off[1]; ho.state = r.host + off[2]; ho.joints = r.host + off[3]; ho.vout = r.host + off[4];
    ho.np = b->m->np; ho.nt = (int)(b->res_cnt[1] / b->F);
    return ho;
}

// The tail of a fit - of a batch's call or of a lane's group: mesh and joints of the arena's n_frames frames (`per` > 0: calls of `per`
// frames each, MeshPass::per) from the states the fit left in it, the hand-over of its first n_floats to the pinned mirror, then ev_copied,
// all on `on.stream` with that stream's owner's scratch.  The arena's slices are taken by address through `off`: the batch's views may be on
// another arena.  with_mesh = false: the arena already holds its mesh.  may_store: the mesh and joints kernels store into the mirror
// themselves where tail_stores says so for these n_floats and frames; the hand-over - a copy command (`big`) or the publish kernel - is
// issued only if the pass took kernels that do not (MeshPassDone::handed_over).
int bf_enqueue_tail(bf_batch *b, ResultArena &r, const size_t off[5], int n_frames, int per, const TailOn &on, size_t n_floats,
                    bool with_mesh, bool may_store, bool big) {
    float *d = r.dev.p;
    MeshPassDone did;
    if (with_mesh) {
        const BfHandOver ho = arena_mirror(b, r, off);
        MeshPass p;
        p.scr = on.scr; p.n = n_frames; p.per = per; p.state = d + off[2]; p.stream = on.stream;
        p.vraw = on.vraw; p.vout = d + off[4]; p.xpart = on.xpart; p.joints = d + off[3];
        if (may_store && tail_stores(b, n_floats * sizeof(float), n_frames)) p.mirror = &ho;
        BF_TRY(bf_launch_mesh(b->m, p, did));
    }
    if (!did.handed_over) BF_TRY(hand_over(on.stream, r, n_floats, big));
    HIP_TRY(hipEventRecord(r.ev_copied, on.stream));
    return BF_OK;
}

// ... of a call of the batch, on the second stream behind `after` (the fit, or the mesh, that filled arena r).  Only a whole-arena tail with
// its mesh (bf_flush_tail) may store into the mirror.
static int enqueue_tail(bf_batch *b, ResultArena &r, size_t n_floats, bool big, hipEvent_t after, bool with_mesh = true) {
    HIP_TRY(hipStreamWaitEvent(b->copy_stream, after, 0));
    return bf_enqueue_tail(b, r, b->res_off, b->F, 0, {b->copy_stream, &b->scratch, b->vraw.p, b->xpart.p}, n_floats, with_mesh,
                           n_floats == b->res_total, big);
}

// result arena k becomes the one the DevBuf views and the pinned mirrors point at
void bf_use_arena(bf_batch *b, int k) {
    float *d = b->arena[k].dev.p, *h = b->arena[k].host;
    b->params.slice(d + b->res_off[0], b->res_cnt[0]); b->terms.slice(d + b->res_off[1], b->res_cnt[1]);
    b->state.slice(d + b->res_off[2], b->res_cnt[2]); b->joints.slice(d + b->res_off[3], b->res_cnt[3]);
    b->vout.slice(d + b->res_off[4], b->res_cnt[4]);
    b->h_params = h + b->res_off[0]; b->h_terms = h + b->res_off[1]; b->h_state = h + b->res_off[2];
    b->h_joints = h + b->res_off[3]; b->h_vout = h + b->res_off[4];
    b->cur = k;
}

// `keypoints`, `params0`, `ndiv` become views of one call's frames at kp / p0 / ndiv, and the cursor says where that is: the one place
// that moves either
void bf_set_inputs(bf_batch *b, const InputCursor &at, float *kp, float *p0, int *ndiv) {
    b->keypoints.slice(kp, (size_t)b->F * b->V * b->m->nl_loss * 3);
    b->params0.slice(p0, (size_t)b->F * b->m->np);
    b->ndiv.slice(ndiv, (size_t)b->F);
    b->in_at = at;
}

// input arena k of the batch's own two becomes the current one (host = true: its pinned staging buffer itself)
static void bf_use_inputs(bf_batch *b, int k, bool host) {
    float *base = host ? b->in[k].host : b->in[k].dev.p;
    InputCursor at;
    at.arena = k; at.host = host;
    bf_set_inputs(b, at, base + b->in_off[0], base + b->in_off[1], (int *)(base + b->in_off[2]));
}

// a synchronous setter's write into the current input arena (the stream is idle)
static hipError_t write_input(bf_batch *b, void *dst, const void *src, size_t bytes) {
    if (b->in_at.host) { std::memcpy(dst, src, bytes); return hipSuccess; }
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}

// the deferred part of a frame-after-frame call (fit_tail_aside): mesh + joints + hand-over of result arena tail_k on the
// second stream, behind the fit that filled it.  Every entry point that looks at results, events of the second stream or starts
// another fit comes through here first (bf_sync_all, bf_fit, bf_batch_get_previous, bf_batch_stage_inputs, bf_batch_destroy).
int bf_flush_tail(bf_batch *b) {
    const int k = b->tail_k;
    if (k < 0) return BF_OK;
    b->tail_k = -1;
    ResultArena &r = b->arena[k];
    const int rc = enqueue_tail(b, r, b->res_total, b->tail_big, r.ev_done);
    if (rc) {
        // the mesh / copy / event of arena k did not all go out: its ev_copied still carries its previous (completed) record, so a
        // wait on it would pass and hand out the pinned buffer's OLD contents.  Nothing of this arena may be read any more:
        // bf_batch_get_previous (`fetched`) and bf_batch_get_result (have_result) then fail instead.
        r.fetched = r.has_v = r.copy_pending = false;
        if (k == b->cur) b->have_result = false;
        return rc;
    }
    b->tail_seq = r.seq;
    return BF_OK;
}

// net_output of smplify.py:103 -> the packed optimiser vector: transl = 0, scale = 1 (:126-128), body pose, betas, root orientation
// (bf_pack_init, lane_slots.h)
BfInitMap bf_init_map(const bf_model *m) { return {m->np, m->nb, m->fit.nbp, m->fit.off_pose, m->fit.off_beta, m->fit.off_orient}; }
static void pack_init(const bf_batch *b, const float *init_betas, const float *init_pose, float *dst) {
    bf_pack_init(bf_init_map(b->m), b->F, init_betas, init_pose, dst);
}

// keypoints | params0 | ndiv of the next frame packed into a pinned staging buffer (`h`; `ev`, `pending`: its transfer), once its previous
// transfer has left it
int bf_pack_staging(const bf_batch *b, float *h, hipEvent_t ev, bool &pending, const float *keypoints, const int32_t *n_use_frames,
                    const float *init_betas, const float *init_pose) {
    if (pending) {
        HIP_TRY(hipEventSynchronize(ev));
        pending = false;
    }
    std::memcpy(h + b->in_off[0], keypoints, (size_t)b->F * b->V * b->m->nl_loss * 3 * sizeof(float));
    pack_init(b, init_betas, init_pose, h + b->in_off[1]);
    bf_fill_ndiv((int32_t *)(h + b->in_off[2]), b->F, n_use_frames, b->V);
    return BF_OK;
}

int bf_sync_all(bf_batch *b) {
    BF_TRY(bf_lanes_drain(b));
    BF_TRY(bf_flush_tail(b));
    if (b->copy_stream) HIP_TRY(hipStreamSynchronize(b->copy_stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->arena[0].copy_pending = b->arena[1].copy_pending = false;
    if (b->h_door_err && *b->h_door_err) {
        const int who = *b->h_door_err;
        *b->h_door_err = 0;
        b->door_usable = false;          // this batch keeps one fit launch per iteration from now on (same results): a second call does not run into the same wait
        int d[BF_DOOR_STATE + 1] = {};
        (void)hipMemcpy(d, b->door.p, sizeof d, hipMemcpyDeviceToHost);
        return fail(BF_ERR_HIP, "dense schedule (bells: ext " + std::to_string(d[BF_DOOR_EXT]) + ", states " + std::to_string(d[BF_DOOR_STATE]) +
                                    ", tickets " + std::to_string(d[BF_DOOR_TICKET]) + ", waiter " + std::to_string(who) + "): a doorbell wait between the persistent fit launch and the dense kernels ran into its time limit");
    }
    return BF_OK;
}

int bf_guard_arena(bf_batch *b) {
    BF_TRY(bf_lanes_drain(b));
    BF_TRY(bf_flush_tail(b));
    ResultArena &r = b->arena[b->cur];
    if (r.copy_pending) {
        HIP_TRY(hipStreamWaitEvent(b->stream, r.ev_copied, 0));
        r.copy_pending = false;
    }
    return BF_OK;
}

extern "C" {
int bf_batch_create(bf_model *m, int n_frames, int n_views, bf_batch **out) {
    if (!m || !out || n_frames <= 0 || n_views <= 0) return fail(BF_ERR_INVALID, "bf_batch_create: bad argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(m->device));
    size_t smem = bf_fit_smem_bytes(m->nj, m->nb, m->npf, m->ns, m->nl, m->np, n_views);
    if (smem > 160 * 1024) return fail(BF_ERR_UNSUPPORTED, "bf_batch_create: too many views for one workgroup's LDS");
    auto *b = new bf_batch();
    b->m = m; b->F = n_frames; b->V = n_views;
    const size_t F = n_frames, np = m->np;
    bool ok = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess;
    b->ring.assign((size_t)bf_batch::kRing * 4, nullptr);
    b->ev = b->ring.data();          // (the events of a slot are created when the slot is first used: 4096 creations cost 4 ms)
    {
        const size_t n_kp = F * n_views * m->nl_loss * 3;
        b->in_off[0] = 0; b->in_off[1] = bf_up64(n_kp); b->in_off[2] = b->in_off[1] + bf_up64(F * np);
        b->in_total = b->in_off[2] + bf_up64(F);
        if (const char *e = getenv("BF_STAGE_MODE")) b->stage_zerocopy = !strcmp(e, "zerocopy");
        if (const char *e = getenv("BF_TAIL_HANDOVER"))          // (copy: the sequence before the kernels stored into the mirror)
            b->tail_handover = !strcmp(e, "copy") ? bf_batch::TailHandOver::COPY : !strcmp(e, "store") ? bf_batch::TailHandOver::STORE : bf_batch::TailHandOver::BY_SIZE;
        ok = ok && b->in[0].create(b->in_total) == hipSuccess && b->in[1].create(b->in_total) == hipSuccess;
        if (ok) bf_use_inputs(b, 0, false);
    }
    {
        const size_t n_par = F * np, n_terms = F * 4, n_state = F * bf_state_stride(m->nj, m->npf, m->nb),
                     n_joints = F * m->n_joint_map * 3, n_v = F * m->nv * 3;
        const size_t o_terms = bf_up64(n_par), o_state = o_terms + bf_up64(n_terms), o_joints = o_state + bf_up64(n_state),
                     o_v = o_joints + bf_up64(n_joints), total = o_v + bf_up64(n_v);          // 256-byte slices
        ok = ok && b->arena[0].create(total) == hipSuccess && b->arena[1].create(total) == hipSuccess;
        {
            // the second stream on the LOWEST priority: the runtime keeps a pool of hardware queues per priority, so it never shares a
            // queue with a batch's main stream (streams that share one run in order, and the hand-over of a call would no longer run
            // under the next call's fit kernel - observed with two live batches)
            int least = 0, greatest = 0;
            ok = ok && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
                 hipStreamCreateWithPriority(&b->copy_stream, hipStreamNonBlocking, least) == hipSuccess;
        }
        if (ok) {
            const size_t offs[5] = {0, o_terms, o_state, o_joints, o_v}, cnts[5] = {n_par, n_terms, n_state, n_joints, n_v};
            for (int i = 0; i < 5; ++i) { b->res_off[i] = offs[i]; b->res_cnt[i] = cnts[i]; }
            b->res_small = o_v; b->res_total = total;
            bf_use_arena(b, 0);
        }
    }
    ok = ok && b->proj.alloc(F * n_views * 12) == hipSuccess;
    if (ok) {
        const std::vector<int> nd(F, n_views);
        for (int k = 0; k < 2; ++k)
            ok = ok && hipMemcpy(b->in[k].dev.p + b->in_off[2], nd.data(), F * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && b->adam_m.alloc(F * np) == hipSuccess;
    ok = ok && b->adam_v.alloc(F * np) == hipSuccess && b->grads.alloc(F * np) == hipSuccess;
    ok = ok && b->vraw.alloc(F * m->nv * 3) == hipSuccess;
    ok = ok && b->xpart.alloc(F * m->mesh.n_tiles * std::max(m->n_extra, 1) * 3) == hipSuccess;
    ok = ok && b->debug.alloc(8192) == hipSuccess;
    if (ok) {
        ok = bf_memset_sync(b->adam_m.p, 0, F * np * sizeof(float)) == hipSuccess &&
             bf_memset_sync(b->adam_v.p, 0, F * np * sizeof(float)) == hipSuccess &&
             bf_memset_sync(b->params.p, 0, F * np * sizeof(float)) == hipSuccess &&
             bf_memset_sync(b->debug.p, 0, 8192 * sizeof(float)) == hipSuccess;
    }
    if (!ok) { bf_batch_destroy(b); return fail(BF_ERR_HIP, "bf_batch_create: device allocation failed"); }
    b->fit_smem = smem;
    {
        int n_cus = 0;
        (void)hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, m->device);
        if (n_cus > 0) b->n_cus = n_cus;
        bf_lanes_configure(b, n_cus);         // (fit lanes: created on first use)
    }
    *out = b;
    return BF_OK;
}

void bf_batch_destroy(bf_batch *b) {
    if (!b) return;
#ifdef BF_HOST_TIMERS
    host_sums_report(b);
#endif
    b->tail_k = -1;                       // (a tail never enqueued: nobody will read that result)
    bf_lanes_destroy(b);                  // (launches the open groups and waits for the lanes' work: it reads the batch's inputs, cameras and Adam table)
    if (b->copy_stream) (void)hipStreamSynchronize(b->copy_stream);
    if (b->stream) { (void)hipStreamSynchronize(b->stream); (void)hipStreamDestroy(b->stream); }
    { std::lock_guard<std::mutex> lk(bf_scan_links()); bf_batch_unlink_scans(b); }      // (its scans outlive it: they forget this batch)
    if (b->graph_exec) (void)hipGraphExecDestroy(b->graph_exec);
    for (auto &e : b->ring) if (e) (void)hipEventDestroy(e);
    if (b->h_pc_weight) (void)hipHostFree(b->h_pc_weight);
    for (auto &e : b->ev_dense) if (e) (void)hipEventDestroy(e);
    for (auto &g : b->graph_pipe) if (g) (void)hipGraphExecDestroy(g);
    if (b->copy_stream) (void)hipStreamDestroy(b->copy_stream);
    if (b->fit_stream) { (void)hipStreamSynchronize(b->fit_stream); (void)hipStreamDestroy(b->fit_stream); }
    for (auto &e : b->ev_door) if (e) (void)hipEventDestroy(e);
    for (auto &e : b->ev_aux) if (e) (void)hipEventDestroy(e);
    if (b->h_door_err) (void)hipHostFree(b->h_door_err);
    if (b->h_resident) (void)hipHostFree(b->h_resident);
    delete b;
}

// general 4x4 inverse, Gauss-Jordan with partial pivoting, in double
static bool invert4(const float *src, double *inv) {
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) { a[r][c] = src[r * 4 + c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (a[piv][c] == 0.0) return false;
        if (piv != c) for (int k = 0; k < 8; ++k) std::swap(a[piv][k], a[c][k]);
        double d = a[c][c];
        for (int k = 0; k < 8; ++k) a[c][k] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            double f = a[r][c];
            if (f != 0.0) for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) inv[r * 4 + c] = a[r][4 + c];
    return true;
}

int bf_batch_set_cameras(bf_batch *b, const float *c2w, const float *K) {
    if (!b || !c2w || !K) return fail(BF_ERR_INVALID, "bf_batch_set_cameras: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    const size_t n = (size_t)b->F * b->V;
    std::vector<float> proj(n * 12);
    for (size_t i = 0; i < n; ++i) {
        double w2c[16];
        if (!invert4(c2w + i * 16, w2c)) return fail(BF_ERR_INVALID, "bf_batch_set_cameras: singular c2w");
        const float *k = K + i * 9;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                proj[i * 12 + r * 4 + c] =
                    (float)((double)k[r * 3] * w2c[c] + (double)k[r * 3 + 1] * w2c[4 + c] + (double)k[r * 3 + 2] * w2c[8 + c]);
    }
    // bf_fit is asynchronous on the batch's own (non-blocking) stream: a fit still in flight reads these inputs
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(b->proj.p, proj.data(), proj.size() * sizeof(float), hipMemcpyHostToDevice));
    bf_lanes_cameras_changed(b);
    return BF_OK;
}

int bf_batch_set_keypoints(bf_batch *b, const float *keypoints, const int32_t *n_use_frames) {
    if (!b || !keypoints) return fail(BF_ERR_INVALID, "bf_batch_set_keypoints: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    std::vector<int> nd(b->F, b->V);
    if (n_use_frames)
        for (int f = 0; f < b->F; ++f) {
            if (n_use_frames[f] <= 0) return fail(BF_ERR_INVALID, "bf_batch_set_keypoints: n_use_frames must be positive");
            nd[f] = n_use_frames[f];
        }
    BF_TRY(bf_sync_all(b));      // (a fit still in flight reads the old keypoints)
    HIP_TRY(write_input(b, b->keypoints.p, keypoints, b->keypoints.n * sizeof(float)));
    HIP_TRY(write_input(b, b->ndiv.p, nd.data(), nd.size() * sizeof(int)));
    return BF_OK;
}

static int reset_adam(bf_batch *b, const float *params_host) {
    HIP_TRY(write_input(b, b->params0.p, params_host, b->params.n * sizeof(float)));
    HIP_TRY(bf_memset_sync(b->adam_m.p, 0, b->adam_m.n * sizeof(float)));
    HIP_TRY(bf_memset_sync(b->adam_v.p, 0, b->adam_v.n * sizeof(float)));
    b->steps_done = 0;
    b->have_result = false;
    b->fetched = false;
    b->staged = false;             // (a fresh start from these parameters: what BF_FIT_RESET would do for staged inputs)
    return BF_OK;
}

// the re-arm as stream commands: the parameters back to the initial estimate, the Adam moments to zero
static int rearm(bf_batch *b) {
    // (hipMemcpyDefault: with BF_STAGE_MODE=zerocopy params0 is a view into the pinned staging buffer, not device memory)
    HIP_TRY(hipMemcpyAsync(b->params.p, b->params0.p, b->params.n * sizeof(float), hipMemcpyDefault, b->stream));
    HIP_TRY(hipMemsetAsync(b->adam_m.p, 0, b->adam_m.n * sizeof(float), b->stream));
    HIP_TRY(hipMemsetAsync(b->adam_v.p, 0, b->adam_v.n * sizeof(float), b->stream));
    return BF_OK;
}

int bf_batch_reset(bf_batch *b) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_reset: null batch");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_guard_arena(b));
    BF_TRY(rearm(b));
    b->steps_done = 0;
    b->have_result = false;
    b->fetched = false;
    b->staged = false;             // (re-armed from the staged parameters: a following bf_fit needs no BF_FIT_RESET)
    return BF_OK;
}

/* The next frame's keypoints and initial estimate, WITHOUT draining the work in flight (apps/genebody_fitting.py:183-192 hands
 * SMPLify a new frame's detections and HMR estimate every call; loss.py:160 re-uploads the keypoints every iteration).  The
 * inputs are packed into the pinned staging buffer the fit in flight does not use and their transfer into the other device
 * arena is queued on the batch stream, behind that fit - or, frame after frame, on the second stream under it (below); the next
 * bf_fit - which must carry BF_FIT_RESET - reads them. */
int bf_batch_stage_inputs(bf_batch *b, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose) {
    BF_HOST_TIMED(b, 0);
    if (!b || !keypoints || !init_betas || !init_pose) return fail(BF_ERR_INVALID, "bf_batch_stage_inputs: null argument");
    if (n_use_frames)
        for (int f = 0; f < b->F; ++f)
            if (n_use_frames[f] <= 0) return fail(BF_ERR_INVALID, "bf_batch_stage_inputs: n_use_frames must be positive");
    HIP_TRY(hipSetDevice(b->m->device));
    if (bf_lanes_enabled(b)) return bf_lanes_stage(b, keypoints, n_use_frames, init_betas, init_pose);
    const int k = b->in_at.arena ^ 1;
    InputArena &in = b->in[k];
    BF_TRY(bf_pack_staging(b, in.host, in.ev, in.pending, keypoints, n_use_frames, init_betas, init_pose));      // (its last transfer: behind a fit that has long finished)
    if (b->stage_zerocopy) {
        // zero-copy: the fit kernel's prologue reads the pinned buffer itself; bf_fit records in.ev behind the fit that read it
        bf_use_inputs(b, k, true);
        b->staged = true;
        return BF_OK;
    }
    // Frame after frame (the fit in flight has its tail still to be enqueued): the transfer goes on the second stream, AHEAD of
    // that tail, and runs under the fit in flight; the batch stream then holds that fit and the next one back to back (the
    // transfer in between cost its 4.6 us and a second dispatch gap: ~13 us of a 430 us step).  Arena k was last read by fit
    // in_reader[k], whose tail - it starts by waiting for that fit - is already on the second stream: the transfer is ordered
    // behind it.  The fit that reads arena k waits for in.ev (bf_fit: on the host while the fit in flight runs).
    // Otherwise it goes on the batch stream, behind the tail's enqueueing (a kernel that reads the pinned buffer over PCIe with coalesced
    // 16-byte loads: one more dispatch on the queue the fit kernel is on, no engine hand-over).
    const bool aside = b->tail_k >= 0 && b->copy_stream && b->in_reader[k] <= b->tail_seq;
    const hipStream_t stream = aside ? b->copy_stream : b->stream;
    b->in_aside[k] = false;
    if (!aside) BF_TRY(bf_flush_tail(b));
    BF_TRY(bf_publish(stream, in.dev.p, in.host, b->in_total));
    HIP_TRY(hipEventRecord(in.ev, stream));
    in.pending = true;
    b->in_aside[k] = aside;
    bf_use_inputs(b, k, false);
    b->staged = true;
    return aside ? bf_flush_tail(b) : BF_OK;
}

int bf_batch_set_init(bf_batch *b, const float *init_betas, const float *init_pose) {
    if (!b || !init_betas || !init_pose) return fail(BF_ERR_INVALID, "bf_batch_set_init: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    const bf_model *m = b->m;
    std::vector<float> p((size_t)b->F * m->np, 0.f);
    pack_init(b, init_betas, init_pose, p.data());
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(b->params.p, p.data(), p.size() * sizeof(float), hipMemcpyHostToDevice));
    return reset_adam(b, p.data());
}

int bf_batch_set_params(bf_batch *b, const float *params) {
    if (!b || !params) return fail(BF_ERR_INVALID, "bf_batch_set_params: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(b->params.p, params, b->params.n * sizeof(float), hipMemcpyHostToDevice));
    return reset_adam(b, params);
}

int bf_batch_get_params(bf_batch *b, float *params) {
    if (!b || !params) return fail(BF_ERR_INVALID, "bf_batch_get_params: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    if (b->fetched) std::memcpy(params, b->h_params, b->params.n * sizeof(float));
    else HIP_TRY(hipMemcpy(params, b->params.p, b->params.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
FrameIO bf_frame_io(bf_batch *b, bool want_grads) {
    FrameIO io;
    io.n_frames = b->F; io.n_views = b->V;
    io.proj = b->proj.p; io.keypoints = b->keypoints.p; io.ndiv = b->ndiv.p;
    io.params = b->params.p; io.params0 = nullptr; io.adam_m = b->adam_m.p; io.adam_v = b->adam_v.p;
    io.grads = want_grads ? b->grads.p : nullptr;
    io.terms = b->terms.p; io.state = b->state.p;
    io.debug = b->debug.p;
    io.cscale = b->cscale.p;          // null unless scans are attached
    io.ext = nullptr;
    io.image_out = nullptr;
    io.door = nullptr;
    io.door_resident = nullptr;
    return io;
}

// full_pose[F, 3 nj] out of the F state rows a fit left at `state` (host memory)
static void full_pose_of(const bf_batch *b, const float *state, float *full_pose) {
    const bf_model *m = b->m;
    const size_t stride = bf_state_stride(m->nj, m->npf, m->nb);
    for (int f = 0; f < b->F; ++f) {
        StateView v = bf_state_view(const_cast<float *>(state) + (size_t)f * stride, m->nj, m->npf, m->nb);
        std::memcpy(full_pose + (size_t)f * 3 * m->nj, v.theta, sizeof(float) * 3 * m->nj);
    }
}

HyperDev bf_to_dev(const bf_hyper &h) {
    HyperDev d;
    d.sigma2 = h.sigma * h.sigma;
    d.w_pose = h.pose_prior_weight * h.pose_prior_weight;
    d.w_angle = h.angle_prior_weight * h.angle_prior_weight;
    d.w_shape = h.shape_prior_weight * h.shape_prior_weight;
    d.cscale = h.constant_scale;
    d.coeff = h.imsize / 1024.0f;
    d.beta1 = h.adam_beta1; d.beta2 = h.adam_beta2; d.eps = h.adam_eps;
    return d;
}

extern "C" {
// torch.optim.Adam evaluates the bias corrections in python floats (double): SURVEY.md 10C
static int ensure_adam_tab(bf_batch *b, const bf_hyper &h, int upto) {
    bool same = b->adam_cap >= upto && b->adam_hyper.lr == h.lr && b->adam_hyper.lr_transl_scale == h.lr_transl_scale &&
                b->adam_hyper.adam_beta1 == h.adam_beta1 && b->adam_hyper.adam_beta2 == h.adam_beta2;
    if (same) return BF_OK;
    int cap = std::max(upto, 1024);
    std::vector<float> tab((size_t)(cap + 1) * 3);            // (+1: a kernel may look one step ahead)
    const double b1 = (double)h.adam_beta1, b2 = (double)h.adam_beta2;
    for (int t = 1; t <= cap + 1; ++t) {
        double bc1 = 1.0 - std::pow(b1, t), bc2 = 1.0 - std::pow(b2, t);
        tab[(size_t)(t - 1) * 3 + 0] = (float)((double)h.lr_transl_scale / bc1);
        tab[(size_t)(t - 1) * 3 + 1] = (float)((double)h.lr / bc1);
        tab[(size_t)(t - 1) * 3 + 2] = (float)std::sqrt(bc2);
    }
    // a table in use is replaced behind everything that reads it; a batch's first table has no reader yet, and building it must not
    // drain the lanes - the first fit of a stream of staged frames would find its slot sent ahead and its group closed
    if (b->adam_tab.p) {
        BF_TRY(bf_sync_all(b));
        (void)hipFree(b->adam_tab.p); b->adam_tab.p = nullptr;
    }
    HIP_TRY(b->adam_tab.upload(tab));
    b->adam_cap = cap;
    b->adam_hyper = h;
    return BF_OK;
}

// floats of a result arena a fetch hands over: [params | terms | state | joints] and, when they were built, the vertices
static size_t result_floats(const bf_batch *b, bool with_v) { return with_v ? b->res_total : b->res_small; }

// How one bf_fit call is put on the GPU.  fit_plan names the route from the flags and the batch's facts before anything is issued;
// fit_impl dispatches on it to one function per route, each the HIP call sequence of that route.
enum class FitRoute {
    LANE,                       // frame after frame on the next fit lane's stream
    GRAPH,                      // the whole call as one hipGraph launch
    GRAPH_PIPELINED,            // ... of kernels only; the fetch runs on the second stream, under whatever is enqueued next
    TAIL_ASIDE,                 // frame after frame on the batch stream; mesh, joints and hand-over deferred to the second stream
    TAIL_ASIDE_CROWDED,         // ... of a batch that fills the machine: the mesh stays on the batch stream, only the copy goes aside
    UNTIMED,                    // the sparse schedule without event records
    TIMED_SPARSE,               // the sparse schedule between the call's timing events
    TIMED_DENSE_LOSSES,         // scans, silhouettes or a dense keypoint loss: bf_fit_with_scans
    TIMED_REFERENCE_LITERAL,    // BF_FIT_DENSE: every iteration evaluates the whole mesh
};
struct FitCall {
    uint32_t flags;             // (BF_FIT_DENSE cleared when dense losses are present)
    bool reset, want_v, fetch;
    bool big_fetch;             // the fetch is 512 KB or more: a copy command (below that the publish kernel)
    int n_iters;
    FitRoute route;
};
// what the routes leave differently: the result is in the pinned mirror, it has vertices, the call's timing events were recorded, the call
// is in a fit lane's group (the lane holds its result)
struct FitDone { bool fetched, has_v, timed, on_lane = false; };

static FitCall fit_plan(const bf_batch *b, int n_iters, uint32_t flags) {
    FitCall c;
    const bool dense_losses = !b->scans.empty() || b->masks.on || b->m->kp_dense;
    if (dense_losses) flags &= ~BF_FIT_DENSE;
    const bool dense = flags & BF_FIT_DENSE, sparse = !dense_losses && !dense;
    c.flags = flags; c.n_iters = n_iters;
    c.reset = flags & BF_FIT_RESET; c.want_v = !(flags & BF_FIT_NO_VERTICES); c.fetch = flags & BF_FIT_FETCH;
    // (a small fetch is cheaper as a copy node inside the graph than as a second stream with two event hand-offs)
    c.big_fetch = result_floats(b, c.want_v) * sizeof(float) >= (size_t)512 * 1024;
    // Calls issued back to back without timing records (frame after frame, as the reference's loop does): the fit kernel is a
    // latency chain of one workgroup per frame, so the mesh / joints / result hand-over of a call runs on the second stream UNDER the
    // next call's fit kernel; the two result arenas alternate as in the pipelined fetch.  With fit lanes such a call goes to the next
    // lane instead; every other call first finds the last fit in the batch's own buffers (bf_lanes_drain).
    const bool tail_aside = (flags & BF_FIT_NOTIME) && !(flags & BF_FIT_GRAPH) && c.reset && sparse && c.fetch && c.want_v;
    if (tail_aside && bf_lanes_enabled(b)) c.route = FitRoute::LANE;
    else if ((flags & BF_FIT_GRAPH) && c.reset && sparse) c.route = (c.fetch && c.big_fetch) ? FitRoute::GRAPH_PIPELINED : FitRoute::GRAPH;
    else if (tail_aside) c.route = b->F >= b->n_cus ? FitRoute::TAIL_ASIDE_CROWDED : FitRoute::TAIL_ASIDE;
    else if ((flags & BF_FIT_NOTIME) && sparse) c.route = FitRoute::UNTIMED;
    else if (sparse) c.route = FitRoute::TIMED_SPARSE;
    else c.route = dense_losses ? FitRoute::TIMED_DENSE_LOSSES : FitRoute::TIMED_REFERENCE_LITERAL;
    return c;
}

// stream work of one sparse-schedule call: [re-arm] -> persistent fit -> [mesh + joints] -> [fetch]; `ev` = event
// records between the parts (null inside a graph capture)
static int enqueue_plain(bf_batch *b, const FitCall &c, const HyperDev &hd, hipEvent_t *ev) {
    FrameIO io = bf_frame_io(b, false);
    if (c.reset) io.params0 = b->params0.p;      // re-arm inside the fit kernel: no copy / memset commands
    HIP_TRY(bf_fit_launch(&b->m->fit, &io, &hd, c.n_iters, 0, b->adam_tab.p, b->steps_done, b->fit_smem, b->stream, nullptr));
    if (ev) HIP_TRY(hipEventRecord(ev[1], b->stream));
    if (c.want_v) {
        BF_TRY(result_mesh(b, ev ? ev[2] : nullptr));
    } else if (ev) HIP_TRY(hipEventRecord(ev[2], b->stream));
    // one copy of the result arena
    if (c.fetch) BF_TRY(hand_over(b->stream, b->arena[b->cur], result_floats(b, c.want_v), c.big_fetch));
    return BF_OK;
}

// `exec` holds the re-armed sparse-schedule call `c` captured for `key`: captured now unless the graph there already is that one
static int ensure_graph(bf_batch *b, hipGraphExec_t &exec, bf_graph_key &exec_key, const bf_graph_key &key, const FitCall &c, const HyperDev &hd) {
    if (exec && std::memcmp(&key, &exec_key, sizeof key) == 0) return BF_OK;
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_plain(b, c, hd, nullptr);
    hipError_t e = hipStreamEndCapture(b->stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    HIP_TRY(e);
    HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    exec_key = key;
    return BF_OK;
}

// LANE: the call joins the open group of the next lane, which goes out when lanes.hip's rules say so
static int fit_lane(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    BF_TRY(bf_lanes_fit(b, c.n_iters, hd));
    done = {true, true, false, true};
    return BF_OK;
}

// both graph routes: the MFMA batch path may grow its scratch buffer - make sure that happened before capturing
static int graph_grow_scratch(bf_batch *b, const FitCall &c) {
    if (c.want_v && b->F >= BF_MFMA_MIN_FRAMES && b->scratch.pose_off.n < (size_t)b->F * b->m->nv * 3) {
        BF_TRY(bf_sync_all(b));
        BF_TRY(result_mesh(b));
        BF_TRY(bf_sync_all(b));
    }
    return BF_OK;
}

// both graph routes: the graph of call `c` into result arena k (the current one), captured if need be, launched between the timing events
static int graph_replay(bf_batch *b, const FitCall &c, const bf_hyper &h, const HyperDev &hd, int k, hipGraphExec_t &exec, bf_graph_key &exec_key) {
    const InputCursor &at = b->in_at;
    const bf_graph_key key{c.n_iters, c.flags, k | (at.arena << 4) | (at.lane << 5) | ((int)at.on_lane << 10) | ((int)at.host << 12) | (at.slot << 16), h};   // (the captured nodes hold the arenas' addresses)
    BF_TRY(ensure_graph(b, exec, exec_key, key, c, hd));
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    HIP_TRY(hipGraphLaunch(exec, b->stream));
    HIP_TRY(hipEventRecord(b->ev[1], b->stream));       // (no events inside a graph: the whole call is charged to ms[0])
    HIP_TRY(hipEventRecord(b->ev[2], b->stream));
    HIP_TRY(hipEventRecord(b->ev[3], b->stream));
    return BF_OK;
}

// GRAPH: the whole call as one hipGraph launch - the host issues a single command per fit
static int fit_graph(bf_batch *b, const FitCall &c, const bf_hyper &h, const HyperDev &hd, FitDone &done) {
    BF_TRY(graph_grow_scratch(b, c));
    BF_TRY(graph_replay(b, c, h, hd, b->cur, b->graph_exec, b->graph_key));
    done = {c.fetch, c.want_v, true};
    return BF_OK;
}

// GRAPH_PIPELINED: this fit writes the result arena the previous one did not use; its device-to-host copy
// runs on the copy stream, under the kernels of whatever is enqueued next
static int fit_graph_pipelined(bf_batch *b, const FitCall &c, const bf_hyper &h, const HyperDev &hd, FitDone &done) {
    BF_TRY(graph_grow_scratch(b, c));
    const int k = b->cur ^ 1;
    ResultArena &r = b->arena[k];
    if (r.copy_pending) { HIP_TRY(hipStreamWaitEvent(b->stream, r.ev_copied, 0)); r.copy_pending = false; }
    bf_use_arena(b, k);
    FitCall kernels = c;                                // (the pipelined graphs hold kernels only)
    kernels.fetch = false;
    BF_TRY(graph_replay(b, kernels, h, hd, k, b->graph_pipe[k], b->graph_pipe_key[k]));
    HIP_TRY(hipEventRecord(r.ev_done, b->stream));
    BF_TRY(enqueue_tail(b, r, result_floats(b, c.want_v), true, r.ev_done, false));
    r.copy_pending = true;
    done = {true, c.want_v, true};
    return BF_OK;
}

// both tail-aside routes: the fit into the result arena the previous one did not use - the current one from here on - re-armed inside
// the kernel; own_signal: the arena's ev_done completes with the fit's own dispatch
static int tail_aside_fit(bf_batch *b, const FitCall &c, const HyperDev &hd, bool own_signal) {
    const int k = b->cur ^ 1;
    ResultArena &r = b->arena[k];
    if (r.copy_pending) {          // (arena k's hand-over of two calls ago: normally long done - then no wait packet goes into the stream)
        if (hipEventQuery(r.ev_copied) != hipSuccess) HIP_TRY(hipStreamWaitEvent(b->stream, r.ev_copied, 0));
        r.copy_pending = false;
    }
    bf_use_arena(b, k);
    FrameIO io = bf_frame_io(b, false);
    io.params0 = b->params0.p;                  // re-arm inside the fit kernel
    HIP_TRY(bf_fit_launch(&b->m->fit, &io, &hd, c.n_iters, 0, b->adam_tab.p, b->steps_done, b->fit_smem, b->stream, own_signal ? r.ev_done : nullptr));
    return BF_OK;
}

// TAIL_ASIDE: the rest - wait for this fit, mesh, joints, hand-over, on the second stream - is enqueued at the next entry point
// (bf_flush_tail): a bf_batch_stage_inputs that follows puts the next frame's inputs ahead of it
static int fit_tail_aside(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    // (ev_done completes with the fit's own dispatch: no marker packet between this fit and the next)
    static const bool own_signal = [] { const char *e = getenv("BF_FIT_DONE_EVENT"); return !(e && e[0] == '0'); }();
    BF_TRY(tail_aside_fit(b, c, hd, own_signal));
    ResultArena &r = b->arena[b->cur];
    if (!own_signal) HIP_TRY(hipEventRecord(r.ev_done, b->stream));
    b->tail_k = b->cur; b->tail_big = c.big_fetch;
    r.copy_pending = true;
    done = {true, true, false};
    return BF_OK;
}

// TAIL_ASIDE_CROWDED.  A batch that fills the machine (a frame's workgroup per CU, one workgroup fits per CU): under the NEXT fit the
// mesh kernels would only get the CUs that fit's workgroups leave as they finish - measured 379 us for a 33 us GEMM at 256 frames.  The
// mesh then goes on the fit's own stream, ahead of the next fit (0.462 + 0.074 ms instead of 0.601); only the copy stays aside.
static int fit_tail_aside_crowded(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    BF_TRY(tail_aside_fit(b, c, hd, false));
    ResultArena &r = b->arena[b->cur];
    BF_TRY(result_mesh(b));
    HIP_TRY(hipEventRecord(r.ev_done, b->stream));
    BF_TRY(enqueue_tail(b, r, b->res_total, c.big_fetch, r.ev_done, false));
    r.copy_pending = true;
    done = {true, true, false};
    return BF_OK;
}

// UNTIMED
static int fit_untimed(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    BF_TRY(enqueue_plain(b, c, hd, nullptr));
    done = {c.fetch, c.want_v, false};
    return BF_OK;
}

// TIMED_SPARSE
static int fit_timed_sparse(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    BF_TRY(enqueue_plain(b, c, hd, b->ev));
    HIP_TRY(hipEventRecord(b->ev[3], b->stream));
    done = {c.fetch, c.want_v, true};
    return BF_OK;
}

// TIMED_DENSE_LOSSES: the loop with scans, silhouettes or the dense keypoint loss (dense_api.hip), then the result mesh
static int fit_timed_dense_losses(bf_batch *b, const FitCall &c, const bf_hyper &h, const HyperDev &hd, FitDone &done) {
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    if (c.reset) BF_TRY(rearm(b));
    BF_TRY(bf_fit_with_scans(b, c.n_iters, h, hd, bf_frame_io(b, false)));
    HIP_TRY(hipEventRecord(b->ev[1], b->stream));
    if (c.want_v) {
        BF_TRY(result_mesh(b, b->ev[2]));
    } else HIP_TRY(hipEventRecord(b->ev[2], b->stream));
    if (c.fetch) BF_TRY(hand_over(b->stream, b->arena[b->cur], result_floats(b, c.want_v), true));      // (always a copy command here)
    HIP_TRY(hipEventRecord(b->ev[3], b->stream));
    done = {c.fetch, c.want_v, true};
    return BF_OK;
}

// TIMED_REFERENCE_LITERAL: every iteration evaluates the whole mesh (smplify.py:179-190)
static int fit_timed_reference_literal(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    const FrameIO io = bf_frame_io(b, false);
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    if (c.reset) BF_TRY(rearm(b));
    for (int it = 0; it < c.n_iters; ++it) {
        HIP_TRY(bf_fit_launch(&b->m->fit, &io, &hd, 1, 0, b->adam_tab.p, b->steps_done + it, b->fit_smem, b->stream, nullptr));
        BF_TRY(result_mesh(b));
    }
    HIP_TRY(hipEventRecord(b->ev[1], b->stream));
    HIP_TRY(hipEventRecord(b->ev[2], b->stream));
    if (c.fetch) BF_TRY(hand_over(b->stream, b->arena[b->cur], b->res_total, true));      // (always a copy command here)
    HIP_TRY(hipEventRecord(b->ev[3], b->stream));
    done = {c.fetch, true, true};
    return BF_OK;
}

// `done`: what the call's route left (the batch's own bookkeeping is done here)
static int fit_impl(bf_batch *b, int n_iters, const bf_hyper *hyper, uint32_t flags, FitDone &done) {
    HIP_TRY(hipSetDevice(b->m->device));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    const FitCall c = fit_plan(b, n_iters, flags);
    // preamble: the lanes drained (or kept, for a lane fit), the counters, the Adam table, the fit image and this call's ring events
    if (c.route != FitRoute::LANE) BF_TRY(bf_lanes_drain(b));
    if (c.reset) { b->steps_done = 0; b->have_result = false; }
    BF_TRY(ensure_adam_tab(b, h, b->steps_done + n_iters));
    const HyperDev hd = bf_to_dev(h);
    BF_TRY(bf_ensure_fit_image(b, bf_frame_io(b, false), hd));       // (once per model: the fit kernel's batched prologue, before any graph captures a launch)
    b->ev = b->ring.data() + (size_t)(b->ring_n % bf_batch::kRing) * 4;
    for (int k = 0; k < 4; ++k)
        if (!b->ev[k]) HIP_TRY(hipEventCreate(&b->ev[k]));
    // a pipelined fetch may still be reading the arena this call writes: the routes that write the current one wait for it
    const bool other_arena = c.route == FitRoute::LANE || c.route == FitRoute::GRAPH_PIPELINED || c.route == FitRoute::TAIL_ASIDE ||
                             c.route == FitRoute::TAIL_ASIDE_CROWDED;
    if (!other_arena) BF_TRY(bf_guard_arena(b));
    switch (c.route) {
    case FitRoute::LANE:                    BF_TRY(fit_lane(b, c, hd, done)); break;
    case FitRoute::GRAPH:                   BF_TRY(fit_graph(b, c, h, hd, done)); break;
    case FitRoute::GRAPH_PIPELINED:         BF_TRY(fit_graph_pipelined(b, c, h, hd, done)); break;
    case FitRoute::TAIL_ASIDE:              BF_TRY(fit_tail_aside(b, c, hd, done)); break;
    case FitRoute::TAIL_ASIDE_CROWDED:      BF_TRY(fit_tail_aside_crowded(b, c, hd, done)); break;
    case FitRoute::UNTIMED:                 BF_TRY(fit_untimed(b, c, hd, done)); break;
    case FitRoute::TIMED_SPARSE:            BF_TRY(fit_timed_sparse(b, c, hd, done)); break;
    case FitRoute::TIMED_DENSE_LOSSES:      BF_TRY(fit_timed_dense_losses(b, c, h, hd, done)); break;
    case FitRoute::TIMED_REFERENCE_LITERAL: BF_TRY(fit_timed_reference_literal(b, c, hd, done)); break;
    }
    // epilogue: the bookkeeping the routes differ in, once
    b->fetched = done.fetched;
    b->have_result = done.has_v;
    b->steps_done += n_iters;           // (a graph call carries BF_FIT_RESET: from zero)
    if (done.timed) { b->ring_n += 1; b->timed = true; }
    return BF_OK;
}

int bf_fit(bf_batch *b, int n_iters, const bf_hyper *hyper, uint32_t flags) {
    BF_HOST_TIMED(b, 1);
    if (!b || n_iters <= 0) return fail(BF_ERR_INVALID, "bf_fit: bad argument");
    if (b->scans_lost)
        return fail(BF_ERR_INVALID, "bf_fit: a scan this batch held was destroyed (bf_scan_destroy) - call bf_batch_set_scans again (NULL: go on without scans)");
    if (b->staged && !(flags & BF_FIT_RESET))
        return fail(BF_ERR_INVALID, "bf_fit: inputs were staged with bf_batch_stage_inputs - the fit of a new frame starts from its initial estimate (BF_FIT_RESET)");
    bf_masks_commit(b);                       // (silhouettes staged with bf_batch_stage_masks become this fit's)
    BF_TRY(bf_flush_tail(b));
    if (!b->in_at.on_lane && b->in_aside[b->in_at.arena]) {
        // inputs staged aside: their transfer was queued on the second stream a few microseconds ago and runs under the fit in flight.
        // Waiting for it HERE, on the host, keeps a wait packet out of the batch stream (the fit in flight has hundreds of
        // microseconds to go); only if it does not show up in time does the stream wait for it.
        const hipEvent_t staged = b->in[b->in_at.arena].ev;
        hipError_t q = hipErrorNotReady;
        const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(500);
        while ((q = hipEventQuery(staged)) == hipErrorNotReady && std::chrono::steady_clock::now() < t_end) { }
        if (q == hipErrorNotReady) HIP_TRY(hipStreamWaitEvent(b->stream, staged, 0));
        else HIP_TRY(q);
        b->in_aside[b->in_at.arena] = false;
    }
    FitDone done{};
    BF_TRY(fit_impl(b, n_iters, hyper, flags, done));
    b->staged = false;
    if (done.on_lane) { b->fit_seq++; return BF_OK; }          // (the call's number is its place in its group)
    ResultArena &r = b->arena[b->cur];
    if (!b->in_at.on_lane) b->in_reader[b->in_at.arena] = b->fit_seq;       // (this fit's number, given to its arena below)
    BF_TRY(bf_masks_mark_used(b));            // (the arena these masks live in may be overwritten once this fit is done)
    if (b->in_at.host) { HIP_TRY(hipEventRecord(b->in[b->in_at.arena].ev, b->stream)); b->in[b->in_at.arena].pending = true; }   // (zero-copy: this fit read the pinned buffer)
    r.seq = b->fit_seq++;
    r.fetched = b->fetched;
    r.has_v = b->have_result;
    return BF_OK;
}

int bf_loss_grad(bf_batch *b, const bf_hyper *hyper, float *terms, float *grads) {
    if (!b) return fail(BF_ERR_INVALID, "bf_loss_grad: null batch");
    bf_model *m = b->m;
    HIP_TRY(hipSetDevice(m->device));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    int rc = ensure_adam_tab(b, h, 1);
    if (rc) return rc;
    HyperDev hd = bf_to_dev(h);
    rc = bf_guard_arena(b);
    if (rc) return rc;
    FrameIO io = bf_frame_io(b, true);
    if (m->kp_dense) { rc = bf_dense_loss_grad(b, h, hd, io); if (rc) return rc; }
    else HIP_TRY(bf_fit_launch(&m->fit, &io, &hd, 1, 1, b->adam_tab.p, 0, b->fit_smem, b->stream, nullptr));
    BF_TRY(bf_sync_all(b));
    if (terms) HIP_TRY(hipMemcpy(terms, b->terms.p, b->terms.n * sizeof(float), hipMemcpyDeviceToHost));
    if (grads) HIP_TRY(hipMemcpy(grads, b->grads.p, b->grads.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

int bf_dense_iter_grad(bf_batch *b, const bf_hyper *hyper, uint32_t flags, const float *dverts_extra, float *terms, float *grads) {
    if (!b) return fail(BF_ERR_INVALID, "bf_dense_iter_grad: null batch");
    if (flags & ~(uint32_t)(BF_DENSE_GRAD_LATE | BF_DENSE_GRAD_SUBMODEL)) return fail(BF_ERR_INVALID, "bf_dense_iter_grad: unknown flag");
    const bool late = flags & BF_DENSE_GRAD_LATE;
    if (b->scans_lost)
        return fail(BF_ERR_INVALID, "bf_dense_iter_grad: a scan this batch held was destroyed (bf_scan_destroy) - call bf_batch_set_scans again (NULL: go on without scans)");
    if (b->staged) return fail(BF_ERR_INVALID, "bf_dense_iter_grad: inputs were staged with bf_batch_stage_inputs - there are no current parameters before the next bf_fit");
    if (late && b->scans.empty() && !b->masks.on)
        return fail(BF_ERR_INVALID, "bf_dense_iter_grad: BF_DENSE_GRAD_LATE with neither scans nor silhouettes attached");
    bf_model *m = b->m;
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(bf_flush_tail(b));
    BF_TRY(bf_lanes_drain(b));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    BF_TRY(ensure_adam_tab(b, h, 1));
    HyperDev hd = bf_to_dev(h);
    BF_TRY(bf_guard_arena(b));
    FrameIO io = bf_frame_io(b, true);
    std::vector<float> t6(terms ? (size_t)b->F * 6 : 0);
    if (!m->kp_dense && !late && !dverts_extra) {
        // a model whose keypoint loss the fit kernel computes itself: bf_fit runs the iterations before the switch-on as plain fit
        // launches (bf_fit_with_scans' n_plain), with no mesh pass and no outside gradient blocks - and so does this call
        HIP_TRY(bf_fit_launch(&m->fit, &io, &hd, 1, 1, b->adam_tab.p, 0, b->fit_smem, b->stream, nullptr));
        BF_TRY(bf_sync_all(b));
        if (terms) {
            std::vector<float> t4((size_t)b->F * 4);
            HIP_TRY(hipMemcpy(t4.data(), b->terms.p, t4.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (int f = 0; f < b->F; ++f) std::copy(t4.begin() + (size_t)f * 4, t4.begin() + (size_t)f * 4 + 4, t6.begin() + (size_t)f * 6);
        }
    } else
        BF_TRY(bf_dense_iter_eval(b, h, hd, io, late, flags & BF_DENSE_GRAD_SUBMODEL, dverts_extra, terms ? t6.data() : nullptr));
    if (terms) std::copy(t6.begin(), t6.end(), terms);
    if (grads) HIP_TRY(hipMemcpy(grads, b->grads.p, b->grads.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

int bf_batch_sync(bf_batch *b) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_sync: null batch");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    return BF_OK;
}

/* The result of the fit issued BEFORE the last one, while the last one is still running: frame i's rtn_dict is read under
 * frame i+1's fit (the serial loop of apps/genebody_fitting.py:183-192 as a two-deep pipeline).  Needs both fits issued with
 * BF_FIT_RESET | BF_FIT_FETCH | BF_FIT_NOTIME on the keypoint-only path (their results then alternate between the two arenas);
 * waits only for that result's hand-over, never for the stream.  params[F,n_params] and the outputs of bf_batch_get_result. */
int bf_batch_get_previous(bf_batch *b, float *params, float *vertices, float *joints, float *full_pose, float *loss_terms) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_get_previous: null batch");
    const bf_model *m = b->m;
    HIP_TRY(hipSetDevice(m->device));
    const long long want = b->fit_seq - 2;
    // with fit lanes the fit before the last may be held by a lane, which keeps its group until its next launch (bf_lanes_find); else by a
    // batch arena - while a lane holds the last fit, the current one, which then holds the fit before it if that was not a lane fit
    BfLaneResult at;
    BF_TRY(bf_lanes_find(b, want, at));
    const bool on_lane = at.arena != nullptr, last_on_lane = bf_lanes_hold_last(b);
    if (!on_lane) {
        at.arena = &b->arena[last_on_lane ? b->cur : b->cur ^ 1];
        std::copy(b->res_off, b->res_off + 5, at.off);
    }
    const ResultArena &r = *at.arena;
    const bool have_it = on_lane || (r.seq == want && r.fetched), have_last = last_on_lane || b->arena[b->cur].seq == b->fit_seq - 1;
    if (b->fit_seq < 2 || !have_it || !have_last)
        return fail(BF_ERR_INVALID, "bf_batch_get_previous: the previous fit's result is not held in the other arena (both fits need "
                                    "BF_FIT_RESET | BF_FIT_FETCH | BF_FIT_NOTIME on the keypoint-only path)");
    if ((vertices || joints) && !r.has_v) return fail(BF_ERR_INVALID, "bf_batch_get_previous: no mesh was evaluated");       // (a lane's group always has its mesh)
    BF_TRY(bf_flush_tail(b));
    HIP_TRY(hipEventSynchronize(r.ev_copied));          // (only that result's hand-over: a lane's group, never the stream)
    const float *h = r.host;
    if (params) std::memcpy(params, h + at.off[0], b->res_cnt[0] * sizeof(float));
    if (loss_terms) std::memcpy(loss_terms, h + at.off[1], b->res_cnt[1] * sizeof(float));
    if (joints) std::memcpy(joints, h + at.off[3], b->res_cnt[3] * sizeof(float));
    if (vertices) std::memcpy(vertices, h + at.off[4], b->res_cnt[4] * sizeof(float));
    if (full_pose) full_pose_of(b, h + at.off[2], full_pose);
    return BF_OK;
}

int bf_batch_get_result(bf_batch *b, float *vertices, float *joints, float *full_pose, float *loss_terms) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_get_result: null batch");
    const bf_model *m = b->m;
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(bf_sync_all(b));
    if ((vertices || joints) && !b->have_result)
        return fail(BF_ERR_INVALID, "bf_batch_get_result: no mesh was evaluated (BF_FIT_NO_VERTICES or no bf_fit yet)");
    if (b->fetched) {
        if (vertices) std::memcpy(vertices, b->h_vout, b->vout.n * sizeof(float));
        if (joints) std::memcpy(joints, b->h_joints, b->joints.n * sizeof(float));
        if (loss_terms) std::memcpy(loss_terms, b->h_terms, b->terms.n * sizeof(float));
    } else {
        if (vertices) HIP_TRY(hipMemcpy(vertices, b->vout.p, b->vout.n * sizeof(float), hipMemcpyDeviceToHost));
        if (joints) HIP_TRY(hipMemcpy(joints, b->joints.p, b->joints.n * sizeof(float), hipMemcpyDeviceToHost));
        if (loss_terms) HIP_TRY(hipMemcpy(loss_terms, b->terms.p, b->terms.n * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (full_pose) {
        if (b->fetched) full_pose_of(b, b->h_state, full_pose);
        else {
            std::vector<float> st(b->state.n);
            HIP_TRY(hipMemcpy(st.data(), b->state.p, st.size() * sizeof(float), hipMemcpyDeviceToHost));
            full_pose_of(b, st.data(), full_pose);
        }
    }
    return BF_OK;
}

int bf_batch_export_params_dev(bf_batch *b, void *dst_dev) {
    if (!b || !dst_dev) return fail(BF_ERR_INVALID, "bf_batch_export_params_dev: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_lanes_drain(b));
    HIP_TRY(hipMemcpyAsync(dst_dev, b->params.p, b->params.n * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
    BF_TRY(bf_sync_all(b));
    return BF_OK;
}

int bf_batch_last_timing(bf_batch *b, float ms[4]) {
    if (!b || !ms) return fail(BF_ERR_INVALID, "bf_batch_last_timing: null argument");
    if (!b->timed) return fail(BF_ERR_INVALID, "bf_batch_last_timing: no bf_fit recorded yet");
    HIP_TRY(hipSetDevice(b->m->device));
    HIP_TRY(hipEventSynchronize(b->ev[3]));
    HIP_TRY(hipEventElapsedTime(&ms[0], b->ev[0], b->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], b->ev[1], b->ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms[2], b->ev[2], b->ev[3]));
    HIP_TRY(hipEventElapsedTime(&ms[3], b->ev[0], b->ev[3]));
    return BF_OK;
}

int bf_batch_timing_reset(bf_batch *b) {
    if (!b) return fail(BF_ERR_INVALID, "bf_batch_timing_reset: null batch");
    b->ring_n = 0;
    return BF_OK;
}

int bf_batch_timing_sum(bf_batch *b, float ms[4], int32_t *n_calls) {
    if (!b || !ms || !n_calls) return fail(BF_ERR_INVALID, "bf_batch_timing_sum: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    int n = std::min(b->ring_n, (int)bf_batch::kRing);
    double acc[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        hipEvent_t *e = b->ring.data() + (size_t)i * 4;
        float t01, t12, t23, t03;
        HIP_TRY(hipEventElapsedTime(&t01, e[0], e[1]));
        HIP_TRY(hipEventElapsedTime(&t12, e[1], e[2]));
        HIP_TRY(hipEventElapsedTime(&t23, e[2], e[3]));
        HIP_TRY(hipEventElapsedTime(&t03, e[0], e[3]));
        acc[0] += t01; acc[1] += t12; acc[2] += t23; acc[3] += t03;
    }
    for (int k = 0; k < 4; ++k) ms[k] = (float)acc[k];
    *n_calls = n;
    return BF_OK;
}

/* The full-mesh forward's OWN duration (bench.py's roofline_mesh): `reps` launches of the single-frame kernel on frame 0's pose state, each
 * leaving first-workgroup-start .. last-workgroup-end on the device's 100 MHz wall clock - no event record, no launch gap in the figure.
 * us[0..2] = mean / min / max in microseconds.  Single-frame SMPL-sized models only (the kernel bf_fit uses there). */
int bf_batch_mesh_span(bf_batch *b, int reps, float us[3]) {
    if (!b || reps <= 0 || !us) return fail(BF_ERR_INVALID, "bf_batch_mesh_span: bad argument");
    bf_model *m = b->m;
    if (bf_mesh_use_multi(m->npf, 1)) return fail(BF_ERR_UNSUPPORTED, "bf_batch_mesh_span: this model's single-frame forward is bf_mesh_multi_kernel");
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(bf_sync_all(b));
    DevBuf<unsigned long long> d_span;
    HIP_TRY(d_span.alloc(2));
    double sum = 0.0, lo = 1e30, hi = 0.0;
    for (int r = 0; r < reps; ++r) {
        const unsigned long long init[2] = {~0ull, 0ull};
        HIP_TRY(hipMemcpy(d_span.p, init, sizeof init, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(bf_mesh_span_kernel, dim3(m->mesh.n_tiles, 1), dim3(BF_MESH_TILE * 3 * BF_MESH_RG), m->mesh_smem, b->stream, m->mesh,
                           (const float *)b->state.p, b->vraw.p, b->vout.p, b->xpart.p, d_span.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(b->stream));
        unsigned long long got[2];
        HIP_TRY(hipMemcpy(got, d_span.p, sizeof got, hipMemcpyDeviceToHost));
        const double t = (double)(got[1] - got[0]) * 0.01;          // 100 MHz ticks -> us
        sum += t; lo = std::min(lo, t); hi = std::max(hi, t);
    }
    us[0] = (float)(sum / reps); us[1] = (float)lo; us[2] = (float)hi;
    return BF_OK;
}

/* test hook: the body vertices the last mesh pass left on the device */
int bf_batch_debug_vertices(bf_batch *b, float *vertices) {
    if (!b || !vertices) return fail(BF_ERR_INVALID, "bf_batch_debug_vertices: null argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(vertices, b->vout.p, b->vout.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

/* test hook: the first-iteration intermediates of frame 0 dumped by the last kernel launch */
int bf_batch_debug_dump(bf_batch *b, float *dst, int n) {
    if (!b || !dst || n <= 0 || n > 8192) return fail(BF_ERR_INVALID, "bf_batch_debug_dump: bad argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(dst, b->debug.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
