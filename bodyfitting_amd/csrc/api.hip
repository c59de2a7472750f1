// Host side of libbodyfit: the C ABI of include/bodyfit.h over the gfx950 kernels.
#include "bf_host.h"
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
int bf_smpl_forward(bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                    float *vertices, float *joints, float *joints_ori) {
    if (!m || n <= 0 || !betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, "bf_smpl_forward: bad argument");
    HIP_TRY(hipSetDevice(m->device));
    const int nj = m->nj, nb = m->nb, nv = m->nv;
    const size_t stride = bf_state_stride(nj, m->npf, nb);
    DevBuf<float> d_beta, d_or, d_bp, d_state, d_vraw, d_j, d_jo, d_xp;
    MeshScratch scratch;
    HIP_TRY(d_beta.upload(std::vector<float>(betas, betas + (size_t)n * nb)));
    HIP_TRY(d_or.upload(std::vector<float>(global_orient, global_orient + (size_t)n * 3)));
    HIP_TRY(d_bp.upload(std::vector<float>(body_pose, body_pose + (size_t)n * 3 * (nj - 1))));
    HIP_TRY(d_state.alloc((size_t)n * stride));
    HIP_TRY(d_vraw.alloc((size_t)n * nv * 3));
    HIP_TRY(d_xp.alloc((size_t)n * m->mesh.n_tiles * m->n_extra * 3));
    HIP_TRY(d_j.alloc((size_t)n * m->n_joint_map * 3));
    HIP_TRY(d_jo.alloc((size_t)n * (nj + m->n_selector) * 3));
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, 0, m->fit, (const float *)d_beta.p,
                       (const float *)d_or.p, (const float *)d_bp.p, (const float *)nullptr, d_state.p,
                       (const float *)nullptr, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    MeshPass mesh;
    mesh.scr = &scratch; mesh.n = n; mesh.state = d_state.p;
    mesh.vraw = d_vraw.p; mesh.xpart = d_xp.p; mesh.joints = d_j.p; mesh.joints_ori = d_jo.p;
    BF_TRY(bf_launch_mesh(m, mesh));
    HIP_TRY(hipDeviceSynchronize());
    if (vertices) HIP_TRY(hipMemcpy(vertices, d_vraw.p, (size_t)n * nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (joints) HIP_TRY(hipMemcpy(joints, d_j.p, d_j.n * sizeof(float), hipMemcpyDeviceToHost));
    if (joints_ori) HIP_TRY(hipMemcpy(joints_ori, d_jo.p, d_jo.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

// A small fetch as a kernel: device arena -> pinned host mirror with plain stores over PCIe (posted writes, visible to the
// host when the stream drains); a copy node costs ~20 us of fixed overhead for the same 90 KB.
__global__ void __launch_bounds__(256) __attribute__((visibility("hidden"))) bf_publish_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}


// Three ranges in one launch: a call's keypoints, initial parameters and view counts into their places in the [W F] arrays of a fit
// lane's input arena - from the slot's pinned staging buffer (PCIe reads) or from the batch's current inputs on the device.  The
// places of a slot are float-aligned only (n_params is 86): 4-byte accesses, coalesced.
struct BfSeg3 { const float *src[3]; float *dst[3]; unsigned n[3]; };
__global__ void __launch_bounds__(256) __attribute__((visibility("hidden"))) bf_publish3_kernel(BfSeg3 s) {
    for (int k = 0; k < 3; ++k) {
        const float *__restrict__ src = s.src[k];
        float *__restrict__ dst = s.dst[k];
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < s.n[k]; i += gridDim.x * 256) dst[i] = src[i];
    }
}


// Seven ranges in one launch: what a drain hands back from a lane's group to the batch - the five result slices of the group's last slot
// and its two Adam-moment rows, device to device (bf_lanes_drain).  Float-aligned places like the above: 4-byte accesses.
struct BfSeg7 { const float *src[7]; float *dst[7]; unsigned n[7]; };
__global__ void __launch_bounds__(256) __attribute__((visibility("hidden"))) bf_publish7_kernel(BfSeg7 s) {
    for (int k = 0; k < 7; ++k) {
        const float *__restrict__ src = s.src[k];
        float *__restrict__ dst = s.dst[k];
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < s.n[k]; i += gridDim.x * 256) dst[i] = src[i];
    }
}

}  // extern "C"
static int publish7(hipStream_t stream, const BfSeg7 &seg) {
    unsigned most = 1;
    for (int k = 0; k < 7; ++k) most = std::max(most, seg.n[k]);
    hipLaunchKernelGGL(bf_publish7_kernel, dim3(std::min((most + 255) / 256, 64u)), dim3(256), 0, stream, seg);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

static int publish3(hipStream_t stream, const BfSeg3 &seg) {
    const unsigned most = std::max(seg.n[0], std::max(seg.n[1], seg.n[2]));
    hipLaunchKernelGGL(bf_publish3_kernel, dim3(std::min(std::max((most + 255) / 256, 1u), 64u)), dim3(256), 0, stream, seg);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

static int publish(hipStream_t stream, float *dst, const float *src, size_t n_floats) {      // (slices are 256-byte multiples: float4 clean)
    const size_t n4 = n_floats / 4;
    hipLaunchKernelGGL(bf_publish_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 64)), dim3(256), 0, stream,
                       (const float4 *)src, (float4 *)dst, n4);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// the first n_floats of a result arena go to its pinned mirror: as a copy command (`big`: the caller's choice) or through the kernel above
static int hand_over(hipStream_t stream, ResultArena &r, size_t n_floats, bool big) {
    if (!big) return publish(stream, r.host, r.dev.p, n_floats);
    HIP_TRY(hipMemcpyAsync(r.host, r.dev.p, n_floats * sizeof(float), hipMemcpyDeviceToHost, stream));
    return BF_OK;
}

// the result mesh of a batch: vertices and mapped joints of its F frames from their pose states, on `stream` with that stream's owner's
// scratch; `after_mesh`: an event recorded between the mesh and the joints pass
// `mirror`: the arena's pinned mirror, for a pass that may hand its results over itself; *handed_over then says whether it did
static int result_mesh(bf_batch *b, MeshScratch *scr, const float *state, float *vraw, float *vout, float *xpart, float *joints,
                       hipStream_t stream, hipEvent_t after_mesh = nullptr, const BfHandOver *mirror = nullptr, bool *handed_over = nullptr) {
    MeshPass p;
    p.scr = scr; p.n = b->F; p.state = state; p.stream = stream;
    p.vraw = vraw; p.vout = vout; p.xpart = xpart; p.joints = joints;
    p.after_mesh = after_mesh;
    p.mirror = mirror;
    MeshPassDone did;
    const int rc = bf_launch_mesh(b->m, p, did);
    if (handed_over) *handed_over = did.handed_over;
    return rc;
}
// ... into the batch's current arena, on the batch stream
static int result_mesh(bf_batch *b, hipEvent_t after_mesh = nullptr) {
    return result_mesh(b, &b->scratch, b->state.p, b->vraw.p, b->vout.p, b->xpart.p, b->joints.p, b->stream, after_mesh);
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

// the tail of a fit: mesh, joints and hand-over of the first n_floats of result arena r on `stream` (scratch, vraw, xpart: that stream's
// owner's), then ev_copied.  `after`: the event the stream waits for first; with_mesh = false: the arena already holds its mesh.
// A whole-arena tail with its mesh (bf_flush_tail) lets the mesh and joints kernels store into the mirror themselves where tail_stores says
// so, and issues a hand-over only if the pass took kernels that do not (MeshPassDone::handed_over).
static int enqueue_tail(bf_batch *b, ResultArena &r, hipStream_t stream, MeshScratch *scr, float *vraw, float *xpart, size_t n_floats,
                        bool big, hipEvent_t after = nullptr, bool with_mesh = true) {
    if (after) HIP_TRY(hipStreamWaitEvent(stream, after, 0));
    float *d = r.dev.p;                              // (the arena's slices by address: the batch's views may be on another one)
    bool handed_over = false;
    if (with_mesh) {
        const BfHandOver ho = arena_mirror(b, r, b->res_off);
        const bool store = n_floats == b->res_total && tail_stores(b, n_floats * sizeof(float), b->F);
        BF_TRY(result_mesh(b, scr, d + b->res_off[2], vraw, d + b->res_off[4], xpart, d + b->res_off[3], stream, nullptr, store ? &ho : nullptr, &handed_over));
    }
    if (!handed_over) BF_TRY(hand_over(stream, r, n_floats, big));
    HIP_TRY(hipEventRecord(r.ev_copied, stream));
    return BF_OK;
}

// result arena k becomes the one the DevBuf views and the pinned mirrors point at
static void bf_use_arena(bf_batch *b, int k) {
    float *d = b->arena[k].dev.p, *h = b->arena[k].host;
    b->params.slice(d + b->res_off[0], b->res_cnt[0]); b->terms.slice(d + b->res_off[1], b->res_cnt[1]);
    b->state.slice(d + b->res_off[2], b->res_cnt[2]); b->joints.slice(d + b->res_off[3], b->res_cnt[3]);
    b->vout.slice(d + b->res_off[4], b->res_cnt[4]);
    b->h_params = h + b->res_off[0]; b->h_terms = h + b->res_off[1]; b->h_state = h + b->res_off[2];
    b->h_joints = h + b->res_off[3]; b->h_vout = h + b->res_off[4];
    b->cur = k;
}

// input arena k of the batch's own two becomes the one `keypoints`, `params0`, `ndiv` point at (host = true: at its pinned staging
// buffer itself)
static void bf_use_inputs(bf_batch *b, int k, bool host) {
    InputArena &in = b->in[k];
    float *base = host ? in.host : in.dev.p;
    const bf_model *m = b->m;
    b->keypoints.slice(base + b->in_off[0], (size_t)b->F * b->V * m->nl_loss * 3);
    b->params0.slice(base + b->in_off[1], (size_t)b->F * m->np);
    b->ndiv.slice((int *)(base + b->in_off[2]), (size_t)b->F);
    b->in_cur = k;
    b->in_slot = 0;
    b->in_pinned = false;
    b->in_host = host;
}

// where slot `slot` of a lane's input arena keeps its frames: keypoints, params0, ndiv
struct SlotPlace { float *kp, *p0; int *ndiv; };
static SlotPlace slot_place(const bf_batch *b, LaneInputs &in, int slot) {
    float *base = in.dev.p;
    return {base + bf_slot_off(b->gin, 0, slot), base + bf_slot_off(b->gin, 1, slot), (int *)(base + bf_slot_off(b->gin, 2, slot))};
}

// ... of input arena a of fit lane j (in_cur = 2 + 2 * j + a, in_slot = slot)
static void bf_use_lane_inputs(bf_batch *b, int j, int a, int slot) {
    const SlotPlace at = slot_place(b, b->lanes[j].in[a], slot);
    b->keypoints.slice(at.kp, (size_t)b->F * b->V * b->m->nl_loss * 3);
    b->params0.slice(at.p0, (size_t)b->F * b->m->np);
    b->ndiv.slice(at.ndiv, (size_t)b->F);
    b->in_cur = 2 + 2 * j + a;
    b->in_slot = slot;
    b->in_host = false;
}
// the lane arena the views are on (in_cur >= 2)
static LaneInputs &current_lane_inputs(bf_batch *b) { return b->lanes[(b->in_cur - 2) / 2].in[(b->in_cur - 2) % 2]; }

// a synchronous setter's write into the current input arena (the stream is idle)
static hipError_t write_input(bf_batch *b, void *dst, const void *src, size_t bytes) {
    if (b->in_host) { std::memcpy(dst, src, bytes); return hipSuccess; }
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
    const int rc = enqueue_tail(b, r, b->copy_stream, &b->scratch, b->vraw.p, b->xpart.p, b->res_total, b->tail_big, r.ev_done);
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

/* Fit lanes.  A frame-after-frame fit (the tail-aside conditions of fit_plan) is one workgroup per frame on one CU for ~380 us while
 * the other CUs idle, and the frames of a capture are independent (every call carries BF_FIT_RESET).  With n_lanes > 1 such a fit goes
 * to a lane: a stream of its own with its own Adam moments, result arena, mesh scratch and input arenas, so that fits of consecutive
 * calls run side by side on different CUs.  A lane's stream holds [input transfer] fit, mesh, joints, hand-over: its own work in order.
 * Lanes are ordered against each other and against the batch stream by HIP events only (no device-side waits): lanes that end up
 * sharing a hardware queue run one after another, never hang.
 *   - Lane GROUPS.  The lanes that run side by side are as many as the high-priority pool has hardware queues (four), but the fit kernel
 *     takes any number of independent frames, one workgroup each, in hardly more time.  So a lane call does not launch at once: it
 *     JOINS the open group of lane `lane_next` - slot after slot of that lane's input arena, up to W calls - and one launch of G F
 *     workgroups, one tail and one hand-over serve the G calls that joined (lane_launch).  The group goes out when a call joins while
 *     its lane is idle (a slow feeder gets G = 1 and no added latency) - unless the feeder is fast and the group young, see
 *     BF_FIT_LANE_HOLD_US below - when it is full (behind the lane's running group), when its calls would differ in iterations or
 *     hyper-parameters, and at every entry point that drains or reads.  Then `lane_next` moves on.
 *     BF_FIT_LANE_HOLD_US=<H> (default 100): a group that finds its lane idle is still held while the call before came less than H
 *     microseconds ago AND the group's first call joined less than H ago - a burst fills groups instead of sending its first calls out
 *     alone; a lone or slow caller never waits, and H bounds what a burst's frames can be held.  0: an idle lane always launches.
 *     BF_FIT_LANE_WIDTH=<n> caps W (default 32; 1: a launch per call, the call sequence before groups); a batch uses at most
 *     CUs / (lanes x frames).  BF_FIT_LANE_FILL=1 turns the idle rule off - groups fill to W or to a flush - so that tests can force
 *     group shapes.
 *   - Lanes take over (lanes_engage) behind everything on the batch stream.  Every entry point that is not a lane fit or a staging drains
 *     them first (bf_lanes_drain, from bf_sync_all / bf_guard_arena / fit_impl): it launches the open group, waits for the lane streams
 *     and leaves the last lane fit's result and Adam moments in the batch's own buffers - the state the tail-aside path leaves - so
 *     that continuing fits, setters, reads, the graph and dense paths run exactly as without lanes.
 *   - HOST-FED groups (W > 1).  bf_batch_stage_inputs issues no GPU work: it packs the call's inputs into the next slot of the open
 *     group's PINNED arena - laid out like the device arena, slot for slot (lane_slots.h; two arenas per lane, a group each) - and
 *     points the batch's views at the slot's place on the device.  lane_launch moves all the group's slots with ONE transfer ahead of
 *     the fit launch (lane_feed: a prefix of slots is three contiguous ranges), a slot staged past the last joined call with them, and
 *     records the arena's event behind it; a drain that finds only such a slot sends it alone, so that whoever reads the views on the
 *     device next - a plain fit, bf_loss_grad, a continuing fit - finds them filled.  The transfer is ordered behind this lane's fits
 *     that last read the arena by stream order and never behind a running fit of another lane.  The lane opens the arena again two of
 *     its groups later; the host waits then only if that transfer has not finished (lane_open).  The fit kernel always reads the device
 *     arena (large view counts and the table-driven instances read the keypoints inside the loop): no zero-copy here.
 *   - A call WITHOUT a staging of its own takes the batch's current inputs: by a host copy, pinned slot to pinned slot, while their
 *     pinned copy is valid (the usual re-fit: no device copy, no event, no wait between lanes - the views move to the new slot), and by
 *     a device-side copy on the lane's stream when they are in device memory only - after a synchronous setter, a device-side
 *     producer or a drain (bf_batch::in_pinned is cleared by every drain).  A group is host-fed or device-fed, never both: a call of
 *     the other kind launches the open group first.  A device-fed group gets no transfer at launch; the next transfer into an arena a
 *     device-side copy read from waits for that copy through the copying lane's event (LaneInputs::readers).
 *   - W = 1 keeps the call sequence before groups: a staging transfers its slot - the arena - at once on the lane's stream, and a call
 *     without a staging of its own reads the current inputs in place.
 * BF_FIT_LANES=<n> sets the lane count (1: no lanes, the single-stream path); a batch uses at most (CUs / frames) of them. */
static FrameIO bf_frame_io(bf_batch *b, bool want_grads);       // (the batch's own launch arguments: below, with the fit routes)
static int env_int(const char *name, int dflt, int lo, int hi) {
    const char *e = getenv(name);
    return std::max(lo, std::min(e ? atoi(e) : dflt, hi));
}
#ifndef BF_FIT_LANE_HOLD_US_DEFAULT
#define BF_FIT_LANE_HOLD_US_DEFAULT 100
#endif
static int fit_lanes_wanted() { static const int d = env_int("BF_FIT_LANES", 4, 1, 32); return d; }
static int fit_lane_width_wanted() { static const int d = env_int("BF_FIT_LANE_WIDTH", 32, 1, 64); return d; }
static bool fit_lane_fill() { static const bool d = env_int("BF_FIT_LANE_FILL", 0, 0, 1) == 1; return d; }
// H of the idle rule (fit_lane): a group that finds its lane idle is held while the feeder is fast - the call before this one less than H ago -
// and the group younger than H.  0: an idle lane always launches (the rule before the hold)
static std::chrono::microseconds fit_lane_hold() { static const int d = env_int("BF_FIT_LANE_HOLD_US", BF_FIT_LANE_HOLD_US_DEFAULT, 0, 10000000); return std::chrono::microseconds(d); }
// a group's hand-over from this size on is a copy command, below it the publish kernel: the threshold fit_plan uses for a call.  Measured
// for groups (profiles/fit_lane_groups.md): the publish kernel for full groups is the slowest, always copying no better than this
static constexpr size_t kLaneCopyBytes = (size_t)512 * 1024;

static void lanes_release(bf_batch *b) {
    if (!b->lanes) return;
    for (int j = 0; j < b->n_lanes; ++j)              // (a lane's fit may read another lane's input arena: all of them first)
        if (b->lanes[j].stream) (void)hipStreamSynchronize(b->lanes[j].stream);
    for (int j = 0; j < b->n_lanes; ++j)
        if (b->lanes[j].stream) (void)hipStreamDestroy(b->lanes[j].stream);
    b->lanes.reset();                     // (the lanes' buffers and arenas)
    if (b->ev_engage) { (void)hipEventDestroy(b->ev_engage); b->ev_engage = nullptr; }
}

static size_t up64(size_t n) { return bf_up64(n); }          // 256-byte slices

static int lanes_create(bf_batch *b) {
    if (b->lanes) return BF_OK;
    const bf_model *m = b->m;
    const size_t F = b->F, np = m->np, W = b->lane_w;
    size_t res_w = 0;                     // a result arena whose arrays hold W calls' frames (W = 1: the batch's res_total)
    for (int i = 0; i < 5; ++i) res_w += up64(W * b->res_cnt[i]);
    b->lanes.reset(new BfLane[b->n_lanes]);
    int least = 0, greatest = 0;
    bool ok = hipEventCreateWithFlags(&b->ev_engage, hipEventDisableTiming) == hipSuccess &&
              hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    for (int j = 0; j < b->n_lanes && ok; ++j) {
        BfLane &l = b->lanes[j];
        // the lane streams on the HIGHEST priority: the runtime keeps a pool of hardware queues per priority (GPU_MAX_HW_QUEUES each),
        // and in the normal pool the null stream and the batch stream already hold two of four - three lanes there ran as two,
        // four on the high pool run as four (profiles/fit_lanes.md)
        ok = hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, greatest) == hipSuccess &&
             l.adam_m.alloc(W * F * np) == hipSuccess && l.adam_v.alloc(W * F * np) == hipSuccess && l.vraw.alloc(W * b->vraw.n) == hipSuccess &&
             l.xpart.alloc(W * b->xpart.n) == hipSuccess && l.arena.create(res_w) == hipSuccess &&
             l.in[0].create(b->gin.total) == hipSuccess && l.in[1].create(b->gin.total) == hipSuccess &&
             (W == 1 || hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming) == hipSuccess);
    }
    if (ok && W > 1) ok = b->proj_rep.alloc(W * b->proj.n) == hipSuccess;
    b->proj_rep_stale = true;
    if (!ok) { lanes_release(b); return fail(BF_ERR_HIP, "fit lanes: creating a lane's stream or buffers failed"); }
    return BF_OK;
}

// the lanes take over behind everything on the batch stream (the inputs, parameters and cameras set there): a lane's stream waits for
// that point before its first work of the period (lane_begin)
static int lanes_engage(bf_batch *b) {
    if (b->lanes_on) return BF_OK;
    BF_TRY(lanes_create(b));
    BF_TRY(bf_flush_tail(b));
    if (b->lane_w > 1 && b->proj_rep_stale) {          // (the cameras change through a setter that drains: once per set_cameras)
        for (int w = 0; w < b->lane_w; ++w)
            HIP_TRY(hipMemcpyAsync(b->proj_rep.p + (size_t)w * b->proj.n, b->proj.p, b->proj.n * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
        b->proj_rep_stale = false;
    }
    HIP_TRY(hipEventRecord(b->ev_engage, b->stream));
    for (int j = 0; j < b->n_lanes; ++j) b->lanes[j].need_engage = true;
    b->lanes_on = true;
    return BF_OK;
}

static int lane_begin(bf_batch *b, BfLane &l) {
    if (l.need_engage) { HIP_TRY(hipStreamWaitEvent(l.stream, b->ev_engage, 0)); l.need_engage = false; }
    l.busy = true;
    return BF_OK;
}

// The one input transfer of a host-fed group of lane j: slots [0, n) of arena `in` - the G calls that joined and, if there is one, the slot
// staged past them; a prefix of slots is three contiguous ranges (bf_slot_prefix) - from the pinned buffer to their places on the device,
// on the lane's stream ahead of the fit, and the arena's event behind it.  This lane's earlier fits that read the arena are ahead in
// stream order; another lane's device-side copy of one of its slots (`readers`) is waited for through that lane's event.
static int lane_feed(bf_batch *b, int j, LaneInputs &in, int n) {
    BfLane &l = b->lanes[j];
    for (int r = 0; r < b->n_lanes; ++r)
        if (r != j && ((in.readers >> r) & 1u)) HIP_TRY(hipStreamWaitEvent(l.stream, b->lanes[r].ev_join, 0));
    in.readers = 0;
    BfRange rg[3];
    bf_slot_prefix(b->gin, n, rg);
    BfSeg3 seg;
    for (int k = 0; k < 3; ++k) { seg.src[k] = in.host + rg[k].off; seg.dst[k] = in.dev.p + rg[k].off; seg.n[k] = (unsigned)rg[k].n; }
    BF_TRY(publish3(l.stream, seg));
    HIP_TRY(hipEventRecord(in.ev, l.stream));
    in.pending = true;
    b->feed_transfers += 1;
    return BF_OK;
}

// The open group of lane j goes out: for a host-fed group its one input transfer, then ONE fit launch for the G F frames of the G calls
// that joined, the tail for all of them (ONE multi-frame mesh launch for calls below 16 frames, a pass per call above: MeshPass::per), one
// hand-over of the group's floats, ev_copied.
// The result arrays are packed for G F frames - FrameIO is array-major over n_frames - and their offsets stay with the group (`held`).
// The lane's group is closed whatever happens, and the next call joins the next lane.
static int lane_launch(bf_batch *b, int j) {
    BfLane &l = b->lanes[j];
    const int G = l.n_open;
    // a host-fed group: its slots [0, G) and a slot staged past the last joined call are in the pinned buffer only
    const int n_feed = (b->lane_w > 1 && l.open_host) ? G + (l.slot_staged ? 1 : 0) : 0;
    if (!G && !n_feed) return BF_OK;
    LaneInputs &in_open = l.in[l.open_a];
    l.open = false; l.n_open = 0; l.slot_staged = false;        // (a slot staged past the last call stays the batch's current inputs: the next call copies it)
    if (!G) return lane_feed(b, j, in_open, n_feed);            // (a drain with nothing joined: the staged slot alone, for whoever reads the views next)
    if (b->lane_next == j) b->lane_next = (j + 1) % b->n_lanes;
    bf_model *m = b->m;
    ResultArena &r = l.arena;
    BfLane::Held h;
    h.seq0 = l.open_seq0; h.G = G;
    for (int i = 0; i < 5; ++i) { h.off[i] = h.total; h.total += up64((size_t)G * b->res_cnt[i]); }
    l.held = BfLane::Held{};                                    // (a failure from here on: the arena holds nothing that may be read)
    r.seq = -1; r.fetched = r.has_v = false;
    float *d = r.dev.p;
    FrameIO io = bf_frame_io(b, false);
    io.n_frames = G * b->F;
    if (l.borrowed) { io.keypoints = l.bor_kp; io.params0 = l.bor_p0; io.ndiv = l.bor_ndiv; }
    else { const SlotPlace at = slot_place(b, l.in[l.open_a], 0); io.keypoints = at.kp; io.params0 = at.p0; io.ndiv = at.ndiv; }      // (re-arm inside the fit kernel)
    if (b->lane_w > 1) io.proj = b->proj_rep.p;
    io.params = d + h.off[0]; io.terms = d + h.off[1]; io.state = d + h.off[2];
    io.adam_m = l.adam_m.p; io.adam_v = l.adam_v.p;
    if (n_feed) BF_TRY(lane_feed(b, j, in_open, n_feed));
    HIP_TRY(bf_fit_launch(&m->fit, &io, &l.open_hd, l.open_iters, 0, b->adam_tab.p, 0, b->fit_smem, l.stream, nullptr));
    MeshPass p;
    p.scr = &l.scratch; p.n = G * b->F; p.per = b->F; p.state = d + h.off[2]; p.stream = l.stream;
    p.vraw = l.vraw.p; p.vout = d + h.off[4]; p.xpart = l.xpart.p; p.joints = d + h.off[3];
    // the group's hand-over: by the tail's own kernels where they store into the mirror (calls below 16 frames), else behind them
    const BfHandOver ho = arena_mirror(b, r, h.off);
    if (tail_stores(b, h.total * sizeof(float), G * b->F)) p.mirror = &ho;
    MeshPassDone did;
    BF_TRY(bf_launch_mesh(m, p, did));
    if (!did.handed_over) BF_TRY(hand_over(l.stream, r, h.total, h.total * sizeof(float) >= kLaneCopyBytes));
    HIP_TRY(hipEventRecord(r.ev_copied, l.stream));
    l.held = h;
    r.seq = h.seq0 + G - 1; r.fetched = r.has_v = true;         // (the arena's newest fit: what a trade in bf_lanes_drain hands on)
    b->lane_launches += 1;
    b->lane_max_g = std::max(b->lane_max_g, G);
    return BF_OK;
}

int bf_lanes_drain(bf_batch *b) {
    if (!b->lanes_on) return BF_OK;
    b->in_pinned = false;                 // (what follows a drain may write the device slot alone: a setter, a device-side producer)
    for (int j = 0; j < b->n_lanes; ++j) BF_TRY(lane_launch(b, j));       // (the open group, if calls have joined one)
    b->lanes_on = false;
    const int j = b->lane_last;
    b->lane_last = -1;
    // The last lane fit lands where the tail-aside path leaves a fit - in the result arena the previous fit did not use, with its Adam
    // moments as the batch's.
    const int k = b->cur ^ 1;
    ResultArena &r = b->arena[k];
    const bool by_kernel = j >= 0 && b->lane_w > 1 && b->lanes[j].held.G > 0;
    if (by_kernel) {
        // A group's arena is laid out for G calls: the last slot's five slices and its two Adam-moment rows are copied, device to device, by
        // ONE launch on the lane's own stream - behind that lane's fit, tail and hand-over, so it ends with the lane instead of starting a
        // chain of copy commands after every lane has been waited for (a bracket ends in exactly one drain: this is on its path).
        // Nothing on the device still uses arena k or the batch's moments when this launch runs:
        //  - the batch stream: lane j has fitted since the lanes took over, so its stream has waited for ev_engage (lane_begin), which
        //    lanes_engage recorded behind everything on the batch stream; and while the lanes are on nothing is issued there - every entry
        //    point but a lane fit or a staging comes through this drain first, and a staging with W > 1 issues no GPU work;
        //  - the second stream: a deferred tail is enqueued and a pipelined fetch of arena k waited for just below, on the host;
        //  - the other lanes use their own arenas and moments, and of the batch's only inputs, cameras and the Adam table - not written here.
        // And nothing reads them before this launch has finished: the lane's stream is waited for below, before this function returns.
        BfLane &l = b->lanes[j];
        BF_TRY(bf_flush_tail(b));
        if (r.copy_pending) { HIP_TRY(hipEventSynchronize(r.ev_copied)); r.copy_pending = false; }
        const BfLane::Held &h = l.held;
        const size_t s = h.G - 1, n_adam = (size_t)b->F * b->m->np;
        BfSeg7 seg;
        for (int i = 0; i < 5; ++i) {
            seg.src[i] = l.arena.dev.p + h.off[i] + s * b->res_cnt[i]; seg.dst[i] = r.dev.p + b->res_off[i]; seg.n[i] = (unsigned)b->res_cnt[i];
        }
        seg.src[5] = l.adam_m.p + s * n_adam; seg.dst[5] = b->adam_m.p; seg.n[5] = (unsigned)n_adam;
        seg.src[6] = l.adam_v.p + s * n_adam; seg.dst[6] = b->adam_v.p; seg.n[6] = (unsigned)n_adam;
        BF_TRY(publish7(l.stream, seg));
    }
    for (int q = 0; q < b->n_lanes; ++q)
        if (b->lanes[q].busy) { HIP_TRY(hipStreamSynchronize(b->lanes[q].stream)); b->lanes[q].busy = false; }
    if (j < 0) return BF_OK;              // (inputs staged, no lane fit since the lanes took over)
    BfLane &l = b->lanes[j];
    if (!by_kernel) {
        // (W = 1, or no group to hand back.)  Nothing on the device uses either side any more (the lane waited for the batch stream before its
        // fit and has finished; a pipelined fetch of arena k is waited for here).
        BF_TRY(bf_flush_tail(b));
        if (r.copy_pending) { HIP_TRY(hipEventSynchronize(r.ev_copied)); r.copy_pending = false; }
    }
    if (!l.held.G) {                      // (its launch failed: no result anywhere)
        b->fetched = b->have_result = false;
        return fail(BF_ERR_HIP, "fit lanes: the last lane fit was not launched");
    }
    if (b->lane_w == 1) {
        // equal-sized buffers: by trading them - the lane takes the batch's arena k and moments (its next fit overwrites them), no
        // copy; the graphs captured with the old addresses are dropped
        r.trade_buffers(l.arena);
        l.held = BfLane::Held{};
        std::swap(b->adam_m.p, l.adam_m.p);
        std::swap(b->adam_v.p, l.adam_v.p);
        if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
        for (auto &g : b->graph_pipe) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    } else {
        // ... and mirror to mirror on the host, now that the lane's hand-over has been waited for.  The group stays readable in the lane
        // (bf_batch_get_previous).
        const BfLane::Held &h = l.held;
        const size_t s = h.G - 1;
        for (int i = 0; i < 5; ++i)
            std::memcpy(r.host + b->res_off[i], l.arena.host + h.off[i] + s * b->res_cnt[i], b->res_cnt[i] * sizeof(float));
        r.seq = h.seq0 + (long long)s; r.fetched = r.has_v = true;
    }
    bf_use_arena(b, k);
    return BF_OK;
}

// bf_batch_stage_inputs on a batch with lanes: the next lane's other input arena, its transfer on that lane's stream
static int stage_lane(bf_batch *b, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose);

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
        auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
        const size_t n_kp = F * n_views * m->nl_loss * 3;
        b->in_off[0] = 0; b->in_off[1] = up(n_kp); b->in_off[2] = b->in_off[1] + up(F * np);
        b->in_total = b->in_off[2] + up(F);
        if (const char *e = getenv("BF_STAGE_MODE")) b->stage_zerocopy = !strcmp(e, "zerocopy");
        if (const char *e = getenv("BF_TAIL_HANDOVER"))          // (copy: the sequence before the kernels stored into the mirror)
            b->tail_handover = !strcmp(e, "copy") ? bf_batch::TailHandOver::COPY : !strcmp(e, "store") ? bf_batch::TailHandOver::STORE : bf_batch::TailHandOver::BY_SIZE;
        ok = ok && b->in[0].create(b->in_total) == hipSuccess && b->in[1].create(b->in_total) == hipSuccess;
        if (ok) bf_use_inputs(b, 0, false);
    }
    {
        auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };          // 256-byte slices
        const size_t n_par = F * np, n_terms = F * 4, n_state = F * bf_state_stride(m->nj, m->npf, m->nb),
                     n_joints = F * m->n_joint_map * 3, n_v = F * m->nv * 3;
        const size_t o_terms = up(n_par), o_state = o_terms + up(n_terms), o_joints = o_state + up(n_state),
                     o_v = o_joints + up(n_joints), total = o_v + up(n_v);
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
        // fit lanes (created on first use): one frame's fit per CU, so at most CUs / frames of them; not with zero-copy staging
        int n_cus = 0;
        (void)hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, m->device);
        if (n_cus > 0) b->n_cus = n_cus;
        const int d = std::min(fit_lanes_wanted(), std::max(n_cus, 1) / n_frames);
        b->n_lanes = (!b->stage_zerocopy && d > 1) ? d : 1;
        // ... and a lane launch carries up to W calls' frames, the lanes' groups together at most a frame per CU
        b->lane_w = std::min(fit_lane_width_wanted(), std::max(1, std::max(n_cus, 1) / (b->n_lanes * n_frames)));
        b->gin = bf_lane_layout(b->lane_w, n_frames, F * n_views * m->nl_loss * 3, m->np);      // (W = 1: in_off / in_total)
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
    for (int j = 0; b->lanes && j < b->n_lanes; ++j)          // (calls that joined a group were promised a fit: it goes out before the wait)
        if (b->lanes[j].n_open && hipSetDevice(b->m->device) == hipSuccess) (void)lane_launch(b, j);
    lanes_release(b);                     // (waits for the lanes' work: it reads the batch's inputs, cameras and Adam table)
    if (b->copy_stream) (void)hipStreamSynchronize(b->copy_stream);
    if (b->stream) { (void)hipStreamSynchronize(b->stream); (void)hipStreamDestroy(b->stream); }
    { std::lock_guard<std::mutex> lk(bf_scan_links()); bf_batch_unlink_scans(b); }      // (its scans outlive it: they forget this batch)
    if (b->graph_exec) (void)hipGraphExecDestroy(b->graph_exec);
    for (auto &e : b->ring) if (e) (void)hipEventDestroy(e);
    if (b->h_pc_weight) (void)hipHostFree(b->h_pc_weight);
    if (b->h_masks) (void)hipHostFree(b->h_masks);
    for (float *q : b->mk_retired) (void)hipFree(q);
    if (b->h_ccount) (void)hipHostFree(b->h_ccount);
    if (b->ev_masks) (void)hipEventDestroy(b->ev_masks);
    if (b->ev_masks_used) (void)hipEventDestroy(b->ev_masks_used);
    if (b->mk_stage.ev) (void)hipEventDestroy(b->mk_stage.ev);
    if (b->mk_stage.ev_used) (void)hipEventDestroy(b->mk_stage.ev_used);
    if (b->mk_stage.h_masks) (void)hipHostFree(b->mk_stage.h_masks);
    if (b->mk_stage.h_ccount) (void)hipHostFree(b->mk_stage.h_ccount);
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
    b->proj_rep_stale = true;
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

// net_output of smplify.py:103 -> the packed optimiser vector: transl = 0, scale = 1 (:126-128), body pose, betas, root orientation
// (bf_pack_init, lane_slots.h)
static BfInitMap init_map(const bf_model *m) { return {m->np, m->nb, m->fit.nbp, m->fit.off_pose, m->fit.off_beta, m->fit.off_orient}; }
static void pack_init(const bf_batch *b, const float *init_betas, const float *init_pose, float *dst) {
    bf_pack_init(init_map(b->m), b->F, init_betas, init_pose, dst);
}

// keypoints | params0 | ndiv of the next frame packed into a pinned staging buffer (`h`; `ev`, `pending`: its transfer), once its previous
// transfer has left it
static int pack_staging(const bf_batch *b, float *h, hipEvent_t ev, bool &pending, const float *keypoints, const int32_t *n_use_frames,
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
    if (b->n_lanes > 1) return stage_lane(b, keypoints, n_use_frames, init_betas, init_pose);
    const int k = b->in_cur ^ 1;
    InputArena &in = b->in[k];
    BF_TRY(pack_staging(b, in.host, in.ev, in.pending, keypoints, n_use_frames, init_betas, init_pose));      // (its last transfer: behind a fit that has long finished)
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
    BF_TRY(publish(stream, in.dev.p, in.host, b->in_total));
    HIP_TRY(hipEventRecord(in.ev, stream));
    in.pending = true;
    b->in_aside[k] = aside;
    bf_use_inputs(b, k, false);
    b->staged = true;
    return aside ? bf_flush_tail(b) : BF_OK;
}

// input arena `a` of lane l is opened for a new group.  Its pinned buffer may still be read by the transfer of the group it held - issued
// two of this lane's groups ago, behind fits that have normally long finished: the host waits only if that transfer has not completed
// (the back-pressure of a feeder that runs ahead of the device)
static int lane_open(bf_batch *b, BfLane &l, bool host_fed) {
    l.open = true;
    l.open_a = l.in_next;
    l.in_next ^= 1;
    l.open_host = host_fed;
    LaneInputs &in = l.in[l.open_a];
    if (host_fed && in.pending) {
        if (hipEventQuery(in.ev) != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(hipEventSynchronize(in.ev));
            b->feed_waits += 1;
        }
        in.pending = false;
    }
    return BF_OK;
}

static int stage_lane(bf_batch *b, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose) {
    BF_TRY(lanes_engage(b));
    if (b->lane_w > 1) {
        // Host-fed groups: NO GPU work here.  The call's inputs are packed into slot n_open of the open arena's pinned buffer - a second
        // staging before a fit rewrites the same slot - and the views point at the slot's place on the device, which the group's one
        // transfer fills when the group is launched (lane_launch; every drain comes through there, so whoever reads the views on the
        // device finds them filled).  Until then the pinned slot is the only valid copy: in_pinned.
        if (b->lanes[b->lane_next].n_open && !b->lanes[b->lane_next].open_host) BF_TRY(lane_launch(b, b->lane_next));   // (a device-fed group: it goes out first)
        const int j = b->lane_next;
        BfLane &l = b->lanes[j];
        BF_TRY(lane_begin(b, l));
        if (!l.open) BF_TRY(lane_open(b, l, true));
        bf_pack_slot(b->gin, l.in[l.open_a].host, l.n_open, init_map(b->m), b->F, b->V, keypoints, n_use_frames, init_betas, init_pose);
        bf_use_lane_inputs(b, j, l.open_a, l.n_open);
        b->in_pinned = true;
        l.slot_staged = true;
        b->staged = true;
        return BF_OK;
    }
    // W = 1, a launch per call: the slot is the arena, filled by a transfer of its own at once (the call sequence before groups)
    const int j = b->lane_next;             // (the lane the next frame-after-frame fit joins)
    BfLane &l = b->lanes[j];
    BF_TRY(lane_begin(b, l));
    if (!l.n_open) {                        // no call has joined: a group on the lane's other arena (a staging after a staging: no wait for the first one's transfer)
        l.open = true;
        l.open_a = l.in_next;
        l.in_next ^= 1;
    }
    const int a = l.open_a;
    LaneInputs &in = l.in[a];
    BF_TRY(pack_staging(b, in.host, in.ev, in.pending, keypoints, n_use_frames, init_betas, init_pose));      // (its last transfer: queued two of this lane's groups ago)
    // what read arena a since it was last filled: this lane's fits are ahead in its stream; another lane's fit that read it in place (a
    // call without a staging of its own) is waited for through that lane's event
    for (int r = 0; r < b->n_lanes; ++r)
        if (r != j && ((in.readers >> r) & 1u)) HIP_TRY(hipStreamWaitEvent(l.stream, b->lanes[r].arena.ev_copied, 0));
    in.readers = 0;
    BF_TRY(publish(l.stream, in.dev.p, in.host, b->in_total));
    HIP_TRY(hipEventRecord(in.ev, l.stream));
    in.pending = true;
    b->feed_transfers += 1;
    bf_use_lane_inputs(b, j, a, 0);
    l.slot_staged = true;
    b->staged = true;
    return BF_OK;
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

static FrameIO bf_frame_io(bf_batch *b, bool want_grads) {
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
// what the routes leave differently: the result is in the pinned mirror, it has vertices, the call's timing events were recorded
struct FitDone { bool fetched, has_v, timed; };

static FitCall fit_plan(const bf_batch *b, int n_iters, uint32_t flags) {
    FitCall c;
    const bool dense_losses = !b->scans.empty() || b->has_masks || b->m->kp_dense;
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
    if (tail_aside && b->n_lanes > 1) c.route = FitRoute::LANE;
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

// LANE: the call joins the open group of the next lane - its inputs are in the group's next slot: staged there, or copied from the
// batch's current inputs now, on the host where their pinned copy is valid and on the device otherwise - and the group is launched if
// its lane is idle or it is full (lane_launch).  A group is host-fed or device-fed, never both: a call of the other kind launches the
// open group first, as a call with other iterations or hyper-parameters does.
static int fit_lane(bf_batch *b, const FitCall &c, const HyperDev &hd, FitDone &done) {
    BF_TRY(lanes_engage(b));
    const int W = b->lane_w;
    {
        // one launch, one n_iters, one set of hyper-parameters and one way of feeding: a call that differs starts a group of its own
        BfLane &o = b->lanes[b->lane_next];
        const bool host_fed = o.slot_staged || b->in_pinned;
        if (o.n_open && (o.open_iters != c.n_iters || std::memcmp(&o.open_hd, &hd, sizeof hd) != 0 || (W > 1 && o.open_host != host_fed)))
            BF_TRY(lane_launch(b, b->lane_next));
    }
    const int j = b->lane_next;
    BfLane &l = b->lanes[j];
    BF_TRY(lane_begin(b, l));
    b->fetched = false; b->have_result = false;                 // (a failure from here on: nothing of this call may be read)
    const int slot = l.n_open;
    // the feed, for the idle rule below: ONE clock read per call
    const auto now = std::chrono::steady_clock::now();
    const std::chrono::microseconds H = fit_lane_hold();
    const bool fast_feed = b->lane_called && now - b->lane_t_call < H;
    b->lane_t_call = now; b->lane_called = true;
    if (slot == 0) { l.open_seq0 = b->fit_seq; l.open_iters = c.n_iters; l.open_hd = hd; l.borrowed = false; l.t_first = now; }
    if (!l.slot_staged && W == 1) {
        // a launch per call: the fit reads the current inputs in place.  Another lane's slot is read without a wait for its transfer,
        // as before groups (width 1 is that call sequence): the transfer went out on its lane ahead of a fit launch that has since
        // been issued
        l.borrowed = true;
        l.bor_kp = b->keypoints.p; l.bor_p0 = b->params0.p; l.bor_ndiv = b->ndiv.p;
        if (b->in_cur >= 2) current_lane_inputs(b).readers |= 1u << j;
    } else if (!l.slot_staged && b->in_pinned) {
        // No staging of its own, and the pinned mirror of the slot the views are on holds the current inputs (the usual re-fit): copied
        // on the host into this group's next slot - no device copy, no event - and the views move there.
        // INVARIANT: the source is the previous call's slot at the latest (every host-fed call leaves the views on its own slot), so its
        // arena belongs to the newest group of its lane or to the open one, and a pinned arena is rewritten only when its lane opens it
        // again two groups later - which takes calls that would have moved the views on.  The source is never the slot written here.
        if (!l.open) BF_TRY(lane_open(b, l, true));
        const LaneInputs &src = current_lane_inputs(b);
        LaneInputs &dst = l.in[l.open_a];
        assert(!(&src == &dst && b->in_slot == slot) && "a re-fit's pinned source is the previous call's slot, never the one it joins");
        bf_copy_slot(b->gin, dst.host, slot, src.host, b->in_slot);
        bf_use_lane_inputs(b, j, l.open_a, slot);
        b->in_pinned = true;
        b->feed_host_copies += 1;
    } else if (!l.slot_staged) {
        // no staging of its own, the current inputs in device memory only (after a synchronous setter, a device-side producer, a drain):
        // whatever keypoints / params0 / ndiv point at, copied on the lane's stream.  A lane slot they point at was filled before the
        // drain that left them there: nothing to wait for; its arena's next transfer waits for this copy (`readers`).
        if (!l.open) BF_TRY(lane_open(b, l, false));
        const SlotPlace at = slot_place(b, l.in[l.open_a], slot);
        if (at.kp != b->keypoints.p) {                          // (else they are this very slot's)
            if (b->in_cur >= 2 && (b->in_cur - 2) / 2 != j) current_lane_inputs(b).readers |= 1u << j;
            BF_TRY(publish3(l.stream, BfSeg3{{b->keypoints.p, b->params0.p, (const float *)b->ndiv.p}, {at.kp, at.p0, (float *)at.ndiv},
                                             {(unsigned)b->keypoints.n, (unsigned)b->params0.n, (unsigned)b->ndiv.n}}));
            HIP_TRY(hipEventRecord(l.ev_join, l.stream));
            b->feed_dev_copies += 1;
        }
    }
    l.open = true; l.slot_staged = false;
    l.n_open = slot + 1;
    b->lane_last = j;
    b->lane_calls += 1;
    done = {true, true, false};
    if (l.n_open >= W) return lane_launch(b, j);                // full: behind the lane's running group, in stream order
    if (!fit_lane_fill()) {
        // The lane is idle: now - a slow feeder waits for nobody, and a fast feeder's first call after a pause goes out alone - UNLESS the
        // feeder is fast (the call before this one came less than H ago) and the group is young (its first call joined less than H ago).
        // Then it is held exactly as a group behind a busy lane is: a burst fills groups instead of sending its first calls out one by
        // one, each a whole launch sequence and a lane cycle for one frame.  The group goes out when it is full, at the first call that
        // finds the feeder slow or the group H old, and at every read, drain, sync or destroy - H bounds what the rule adds to a burst's
        // frames.  W = 1 and H = 0: the idle rule alone.
        const bool hold = W > 1 && fast_feed && now - l.t_first < H;
        if (!hold) {
            const hipError_t q = hipEventQuery(l.arena.ev_copied);
            if (q == hipSuccess) return lane_launch(b, j);
            (void)hipGetLastError();
            if (q != hipErrorNotReady) HIP_TRY(q);
        }
    }
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
    const bf_graph_key key{c.n_iters, c.flags, k | (b->in_cur << 4) | ((int)b->in_host << 12) | (b->in_slot << 16), h};   // (the captured nodes hold the arenas' addresses)
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
    BF_TRY(enqueue_tail(b, r, b->copy_stream, &b->scratch, b->vraw.p, b->xpart.p, result_floats(b, c.want_v), true, r.ev_done, false));
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
    BF_TRY(enqueue_tail(b, r, b->copy_stream, &b->scratch, b->vraw.p, b->xpart.p, b->res_total, c.big_fetch, r.ev_done, false));
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

static int fit_impl(bf_batch *b, int n_iters, const bf_hyper *hyper, uint32_t flags) {
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
    FitDone done{};
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
    if (b->in_cur < 2 && b->in_aside[b->in_cur]) {
        // inputs staged aside: their transfer was queued on the second stream a few microseconds ago and runs under the fit in flight.
        // Waiting for it HERE, on the host, keeps a wait packet out of the batch stream (the fit in flight has hundreds of
        // microseconds to go); only if it does not show up in time does the stream wait for it.
        const hipEvent_t staged = b->in[b->in_cur].ev;
        hipError_t q = hipErrorNotReady;
        const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(500);
        while ((q = hipEventQuery(staged)) == hipErrorNotReady && std::chrono::steady_clock::now() < t_end) { }
        if (q == hipErrorNotReady) HIP_TRY(hipStreamWaitEvent(b->stream, staged, 0));
        else HIP_TRY(q);
        b->in_aside[b->in_cur] = false;
    }
    BF_TRY(fit_impl(b, n_iters, hyper, flags));
    b->staged = false;
    // (went to a lane - every other call drains the lanes first, which clears lane_last: the call's number is its place in its group)
    if (b->lane_last >= 0) { b->fit_seq++; return BF_OK; }
    ResultArena &r = b->arena[b->cur];
    if (b->in_cur < 2) b->in_reader[b->in_cur] = b->fit_seq;       // (this fit's number, given to its arena below)
    if (b->has_masks) {                       // (the arena these masks live in may be overwritten once this fit is done)
        if (!b->ev_masks_used) HIP_TRY(hipEventCreateWithFlags(&b->ev_masks_used, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->ev_masks_used, b->stream));
    }
    if (b->in_host) { HIP_TRY(hipEventRecord(b->in[b->in_cur].ev, b->stream)); b->in[b->in_cur].pending = true; }   // (zero-copy: this fit read the pinned buffer)
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
    if (late && b->scans.empty() && !b->has_masks)
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
    // with fit lanes the fit before the last may be held by a lane (which keeps its group until that lane's next launch) - in a
    // launched group, or in the open one, which then goes out now: slot `slot` of lane `lane`
    int lane = -1, slot = 0;
    for (int j = 0; b->lanes && want >= 0 && j < b->n_lanes; ++j) {
        BfLane &l = b->lanes[j];
        if (l.n_open && want >= l.open_seq0 && want < l.open_seq0 + l.n_open) BF_TRY(lane_launch(b, j));
        if (l.held.G && want >= l.held.seq0 && want < l.held.seq0 + l.held.G) { lane = j; slot = (int)(want - l.held.seq0); }
    }
    // (while a lane holds the last fit, the batch's current arena holds the fit before it, if that was not a lane fit)
    const ResultArena &r = lane >= 0 ? b->lanes[lane].arena : b->arena[b->lane_last >= 0 ? b->cur : b->cur ^ 1];
    const bool held = lane >= 0 || (r.seq == want && r.fetched), last_held = b->lane_last >= 0 || b->arena[b->cur].seq == b->fit_seq - 1;
    if (b->fit_seq < 2 || !held || !last_held)
        return fail(BF_ERR_INVALID, "bf_batch_get_previous: the previous fit's result is not held in the other arena (both fits need "
                                    "BF_FIT_RESET | BF_FIT_FETCH | BF_FIT_NOTIME on the keypoint-only path)");
    if ((vertices || joints) && lane < 0 && !r.has_v) return fail(BF_ERR_INVALID, "bf_batch_get_previous: no mesh was evaluated");
    BF_TRY(bf_flush_tail(b));
    HIP_TRY(hipEventSynchronize(r.ev_copied));          // (only that result's hand-over: a lane's group, never the stream)
    size_t off[5];
    for (int i = 0; i < 5; ++i) off[i] = lane >= 0 ? b->lanes[lane].held.off[i] + (size_t)slot * b->res_cnt[i] : b->res_off[i];
    const float *h = r.host;
    if (params) std::memcpy(params, h + off[0], b->res_cnt[0] * sizeof(float));
    if (loss_terms) std::memcpy(loss_terms, h + off[1], b->res_cnt[1] * sizeof(float));
    if (joints) std::memcpy(joints, h + off[3], b->res_cnt[3] * sizeof(float));
    if (vertices) std::memcpy(vertices, h + off[4], b->res_cnt[4] * sizeof(float));
    if (full_pose) {
        const size_t stride = bf_state_stride(m->nj, m->npf, m->nb);
        for (int f = 0; f < b->F; ++f) {
            StateView v = bf_state_view(const_cast<float *>(h) + off[2] + (size_t)f * stride, m->nj, m->npf, m->nb);
            std::memcpy(full_pose + (size_t)f * 3 * m->nj, v.theta, sizeof(float) * 3 * m->nj);
        }
    }
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
        const size_t stride = bf_state_stride(m->nj, m->npf, m->nb);
        std::vector<float> st((size_t)b->F * stride);
        if (b->fetched) std::memcpy(st.data(), b->h_state, st.size() * sizeof(float));
        else HIP_TRY(hipMemcpy(st.data(), b->state.p, st.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int f = 0; f < b->F; ++f) {
            StateView v = bf_state_view(st.data() + (size_t)f * stride, m->nj, m->npf, m->nb);
            std::memcpy(full_pose + (size_t)f * 3 * m->nj, v.theta, sizeof(float) * 3 * m->nj);
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

/* test hook: fit-lane groups since the batch was created - out[0] lane launches, out[1] lane calls, out[2] the largest group, out[3] W */
int bf_batch_lane_stats(bf_batch *b, int32_t out[4]) {
    if (!b || !out) return fail(BF_ERR_INVALID, "bf_batch_lane_stats: null argument");
    out[0] = b->lane_launches; out[1] = b->lane_calls; out[2] = b->lane_max_g; out[3] = b->n_lanes > 1 ? b->lane_w : 1;
    return BF_OK;
}

/* test hook: how the fit lanes were fed - out[0] input transfers, out[1] host-side slot copies, out[2] device-side slot copies, out[3] host
 * waits on a pinned arena */
int bf_batch_lane_feed_stats(bf_batch *b, int64_t out[4]) {
    if (!b || !out) return fail(BF_ERR_INVALID, "bf_batch_lane_feed_stats: null argument");
    out[0] = b->feed_transfers; out[1] = b->feed_host_copies; out[2] = b->feed_dev_copies; out[3] = b->feed_waits;
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
