// The fit lanes of a batch: frame-after-frame fits on streams of their own, in groups (interface: lanes.h; decisions: lane_policy.h;
// slot arithmetic: lane_slots.h).
#include "lanes.h"
#include "lane_policy.h"
#include "fit_kernels.h"
#include <cassert>

/* Fit lanes.  A frame-after-frame fit (the tail-aside conditions of fit_plan) is one workgroup per frame on one CU for ~380 us while
 * the other CUs idle, and the frames of a capture are independent (every call carries BF_FIT_RESET).  With more than one lane such a fit
 * goes to a lane: a stream of its own with its own Adam moments, result arena, mesh scratch and input arenas, so that fits of consecutive
 * calls run side by side on different CUs.  A lane's stream holds [input transfer] fit, mesh, joints, hand-over: its own work in order.
 * Lanes are ordered against each other and against the batch stream by HIP events only (no device-side waits): lanes that end up
 * sharing a hardware queue run one after another, never hang.
 *   - Lane GROUPS.  The lanes that run side by side are as many as the high-priority pool has hardware queues (four), but the fit kernel
 *     takes any number of independent frames, one workgroup each, in hardly more time.  So a lane call does not launch at once: it
 *     JOINS the open group of lane `next` - slot after slot of that lane's input arena, up to W calls - and one launch of G F
 *     workgroups, one tail and one hand-over serve the G calls that joined (lane_launch).  The group goes out when a call joins while
 *     its lane is idle (a slow feeder gets G = 1 and no added latency) - unless the feeder is fast and the group young, see
 *     BF_FIT_LANE_HOLD_US below - when it is full (behind the lane's running group), when its calls would differ in iterations or
 *     hyper-parameters, and at every entry point that drains or reads.  Then `next` moves on.
 *     BF_FIT_LANE_HOLD_US=<H> (default 100): a group that finds its lane idle is still held while the call before came less than H
 *     microseconds ago AND the group's first call joined less than H ago - a burst fills groups instead of sending its first calls out
 *     alone; a lone or slow caller never waits, and H bounds what a burst's frames can be held.  0: an idle lane always launches.
 *     BF_FIT_LANE_WIDTH=<n> caps W (default 32; 1: a launch per call, the call sequence before groups); a batch uses at most
 *     CUs / (lanes x frames).  BF_FIT_LANE_FILL=1 turns the idle rule off - groups fill to W or to a flush - so that tests can force
 *     group shapes.  (The rules as functions: lane_policy.h.)
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
 *     producer or a drain (InputCursor::pinned is cleared by every drain).  A group is host-fed or device-fed, never both: a call of
 *     the other kind launches the open group first.  A device-fed group gets no transfer at launch; the next transfer into an arena a
 *     device-side copy read from waits for that copy through the copying lane's event (InputArena::readers).
 *   - W = 1 keeps the call sequence before groups: a staging transfers its slot - the arena - at once on the lane's stream, and a call
 *     without a staging of its own reads the current inputs in place.
 * BF_FIT_LANES=<n> sets the lane count (1: no lanes, the single-stream path); a batch uses at most (CUs / frames) of them. */
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
// H of the idle rule (bf_lane_after_join): a group that finds its lane idle is held while the feeder is fast - the call before this one less
// than H ago - and the group younger than H.  0: an idle lane always launches (the rule before the hold)
static std::chrono::microseconds fit_lane_hold() { static const int d = env_int("BF_FIT_LANE_HOLD_US", BF_FIT_LANE_HOLD_US_DEFAULT, 0, 10000000); return std::chrono::microseconds(d); }
// a group's hand-over from this size on is a copy command, below it the publish kernel: the threshold fit_plan uses for a call.  Measured
// for groups (profiles/fit_lane_groups.md): the publish kernel for full groups is the slowest, always copying no better than this
static constexpr size_t kLaneCopyBytes = (size_t)512 * 1024;

// N ranges in one launch, from and to places that are float-aligned only (n_params is 86): 4-byte accesses, coalesced.
//   3: a call's keypoints, initial parameters and view counts into their places in the [W F] arrays of a lane's input arena - from the
//      arena's pinned buffer (PCIe reads; lane_feed) or from the batch's current inputs on the device (bf_lanes_fit);
//   7: what a drain hands back from a lane's group to the batch - the five result slices of the group's last slot and its two
//      Adam-moment rows, device to device (bf_lanes_drain).
template <int N> struct BfSegs { const float *src[N]; float *dst[N]; unsigned n[N]; };
template <int N>
__global__ void __launch_bounds__(256) __attribute__((visibility("hidden"))) bf_publish_segs_kernel(BfSegs<N> s) {
    for (int k = 0; k < N; ++k) {
        const float *__restrict__ src = s.src[k];
        float *__restrict__ dst = s.dst[k];
        for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < s.n[k]; i += gridDim.x * 256) dst[i] = src[i];
    }
}
template <int N>
static int publish_segs(hipStream_t stream, const BfSegs<N> &seg) {
    unsigned most = 1;
    for (int k = 0; k < N; ++k) most = std::max(most, seg.n[k]);
    hipLaunchKernelGGL(bf_publish_segs_kernel<N>, dim3(std::min((most + 255) / 256, 64u)), dim3(256), 0, stream, seg);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

void bf_lanes_configure(bf_batch *b, int n_cus) {
    // one frame's fit per CU, so at most CUs / frames lanes, not with zero-copy staging; and a lane launch carries up to W calls' frames,
    // the lanes' groups together at most a frame per CU
    const BfLaneSizing s = bf_lane_sizing(n_cus, b->F, fit_lanes_wanted(), fit_lane_width_wanted(), b->stage_zerocopy);
    b->lanes.n = s.n_lanes; b->lanes.W = s.W;
    b->lanes.gin = bf_lane_layout(s.W, b->F, (size_t)b->F * b->V * b->m->nl_loss * 3, b->m->np);      // (W = 1: in_off / in_total)
}

static void lanes_release(bf_batch *b) {
    BfLanes &L = b->lanes;
    if (!L.lane) return;
    for (int j = 0; j < L.n; ++j)              // (a lane's fit may read another lane's input arena: all of them first)
        if (L.lane[j].stream) (void)hipStreamSynchronize(L.lane[j].stream);
    for (int j = 0; j < L.n; ++j)
        if (L.lane[j].stream) (void)hipStreamDestroy(L.lane[j].stream);
    L.lane.reset();                       // (the lanes' buffers and arenas)
    if (L.ev_engage) { (void)hipEventDestroy(L.ev_engage); L.ev_engage = nullptr; }
}

static int lanes_create(bf_batch *b) {
    BfLanes &L = b->lanes;
    if (L.lane) return BF_OK;
    const bf_model *m = b->m;
    const size_t F = b->F, np = m->np, W = L.W;
    size_t res_w = 0;                     // a result arena whose arrays hold W calls' frames (W = 1: the batch's res_total)
    for (int i = 0; i < 5; ++i) res_w += bf_up64(W * b->res_cnt[i]);
    L.lane.reset(new BfLane[L.n]);
    int least = 0, greatest = 0;
    bool ok = hipEventCreateWithFlags(&L.ev_engage, hipEventDisableTiming) == hipSuccess &&
              hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    for (int j = 0; j < L.n && ok; ++j) {
        BfLane &l = L.lane[j];
        // the lane streams on the HIGHEST priority: the runtime keeps a pool of hardware queues per priority (GPU_MAX_HW_QUEUES each),
        // and in the normal pool the null stream and the batch stream already hold two of four - three lanes there ran as two,
        // four on the high pool run as four (profiles/fit_lanes.md)
        ok = hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, greatest) == hipSuccess &&
             l.adam_m.alloc(W * F * np) == hipSuccess && l.adam_v.alloc(W * F * np) == hipSuccess && l.vraw.alloc(W * b->vraw.n) == hipSuccess &&
             l.xpart.alloc(W * b->xpart.n) == hipSuccess && l.arena.create(res_w) == hipSuccess &&
             l.in[0].create(L.gin.total) == hipSuccess && l.in[1].create(L.gin.total) == hipSuccess &&
             (W == 1 || hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming) == hipSuccess);
    }
    if (ok && W > 1) ok = L.proj_rep.alloc(W * b->proj.n) == hipSuccess;
    L.proj_rep_stale = true;
    if (!ok) { lanes_release(b); return fail(BF_ERR_HIP, "fit lanes: creating a lane's stream or buffers failed"); }
    return BF_OK;
}

// the lanes take over behind everything on the batch stream (the inputs, parameters and cameras set there): a lane's stream waits for
// that point before its first work of the period (lane_begin)
static int lanes_engage(bf_batch *b) {
    BfLanes &L = b->lanes;
    if (L.on) return BF_OK;
    BF_TRY(lanes_create(b));
    BF_TRY(bf_flush_tail(b));
    if (L.W > 1 && L.proj_rep_stale) {          // (the cameras change through a setter that drains: once per set_cameras)
        for (int w = 0; w < L.W; ++w)
            HIP_TRY(hipMemcpyAsync(L.proj_rep.p + (size_t)w * b->proj.n, b->proj.p, b->proj.n * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
        L.proj_rep_stale = false;
    }
    HIP_TRY(hipEventRecord(L.ev_engage, b->stream));
    for (int j = 0; j < L.n; ++j) L.lane[j].need_engage = true;
    L.on = true;
    return BF_OK;
}

static int lane_begin(bf_batch *b, BfLane &l) {
    if (l.need_engage) { HIP_TRY(hipStreamWaitEvent(l.stream, b->lanes.ev_engage, 0)); l.need_engage = false; }
    l.busy = true;
    return BF_OK;
}

// where slot `slot` of a lane's input arena keeps its frames: keypoints, params0, ndiv
struct SlotPlace { float *kp, *p0; int *ndiv; };
static SlotPlace slot_place(const bf_batch *b, InputArena &in, int slot) {
    const BfLaneLayout &gin = b->lanes.gin;
    float *base = in.dev.p;
    return {base + bf_slot_off(gin, 0, slot), base + bf_slot_off(gin, 1, slot), (int *)(base + bf_slot_off(gin, 2, slot))};
}

// slot `slot` of input arena a of lane j becomes the one `keypoints`, `params0`, `ndiv` point at.  pinned: the slot's pinned mirror holds
// these inputs too (host-fed groups)
static void use_lane_inputs(bf_batch *b, int j, int a, int slot, bool pinned) {
    const SlotPlace at = slot_place(b, b->lanes.lane[j].in[a], slot);
    InputCursor c;
    c.on_lane = true; c.lane = j; c.arena = a; c.slot = slot; c.pinned = pinned;
    bf_set_inputs(b, c, at.kp, at.p0, at.ndiv);
}
// the lane arena the views are on (in_at.on_lane)
static InputArena &current_arena(bf_batch *b) { return b->lanes.lane[b->in_at.lane].in[b->in_at.arena]; }

// The input transfer of lane j out of the pinned buffer of its arena `in`, on the lane's stream ahead of the fit, and the arena's event
// behind it.  W > 1, the one transfer of a host-fed group: slots [0, n) - the G calls that joined and, if there is one, the slot staged
// past them; a prefix of slots is three contiguous ranges (bf_slot_prefix).  W = 1, at every staging: the arena is the slot, whole 256-byte
// slices.  This lane's earlier fits that read the arena are ahead in stream order; another lane that read it from outside (`readers`) is
// waited for through that lane's event: its device-side copy of one of the slots (W > 1, ev_join), or its fit that read the slot in place
// (W = 1, a call without a staging of its own: that lane's ev_copied).
static int lane_feed(bf_batch *b, int j, InputArena &in, int n) {
    BfLanes &L = b->lanes;
    BfLane &l = L.lane[j];
    for (int r = 0; r < L.n; ++r)
        if (r != j && ((in.readers >> r) & 1u)) HIP_TRY(hipStreamWaitEvent(l.stream, L.W > 1 ? L.lane[r].ev_join : L.lane[r].arena.ev_copied, 0));
    in.readers = 0;
    if (L.W > 1) {
        BfRange rg[3];
        bf_slot_prefix(L.gin, n, rg);
        BfSegs<3> seg;
        for (int k = 0; k < 3; ++k) { seg.src[k] = in.host + rg[k].off; seg.dst[k] = in.dev.p + rg[k].off; seg.n[k] = (unsigned)rg[k].n; }
        BF_TRY(publish_segs(l.stream, seg));
    } else
        BF_TRY(bf_publish(l.stream, in.dev.p, in.host, b->in_total));
    HIP_TRY(hipEventRecord(in.ev, l.stream));
    in.pending = true;
    L.feed_transfers += 1;
    return BF_OK;
}

// The open group of lane j goes out: for a host-fed group its one input transfer, then ONE fit launch for the G F frames of the G calls
// that joined, the tail for all of them (ONE multi-frame mesh launch for calls below 16 frames, a pass per call above: MeshPass::per), one
// hand-over of the group's floats, ev_copied (bf_enqueue_tail).
// The result arrays are packed for G F frames - FrameIO is array-major over n_frames - and their offsets stay with the group (`held`).
// The lane's group is closed whatever happens, and the next call joins the next lane.
static int lane_launch(bf_batch *b, int j) {
    BfLanes &L = b->lanes;
    BfLane &l = L.lane[j];
    const int G = l.n_open;
    // a host-fed group: its slots [0, G) and a slot staged past the last joined call are in the pinned buffer only
    const int n_feed = (L.W > 1 && l.open_host) ? G + (l.slot_staged ? 1 : 0) : 0;
    if (!G && !n_feed) return BF_OK;
    InputArena &in_open = l.in[l.open_a];
    l.open = false; l.n_open = 0; l.slot_staged = false;        // (a slot staged past the last call stays the batch's current inputs: the next call copies it)
    if (!G) return lane_feed(b, j, in_open, n_feed);            // (a drain with nothing joined: the staged slot alone, for whoever reads the views next)
    if (L.next == j) L.next = (j + 1) % L.n;
    ResultArena &r = l.arena;
    BfLane::Held h;
    h.seq0 = l.open_seq0; h.G = G;
    for (int i = 0; i < 5; ++i) { h.off[i] = h.total; h.total += bf_up64((size_t)G * b->res_cnt[i]); }
    l.held = BfLane::Held{};                                    // (a failure from here on: the arena holds nothing that may be read)
    r.seq = -1; r.fetched = r.has_v = false;
    float *d = r.dev.p;
    FrameIO io = bf_frame_io(b, false);
    io.n_frames = G * b->F;
    if (l.borrowed) { io.keypoints = l.bor_kp; io.params0 = l.bor_p0; io.ndiv = l.bor_ndiv; }
    else { const SlotPlace at = slot_place(b, in_open, 0); io.keypoints = at.kp; io.params0 = at.p0; io.ndiv = at.ndiv; }      // (re-arm inside the fit kernel)
    if (L.W > 1) io.proj = L.proj_rep.p;
    io.params = d + h.off[0]; io.terms = d + h.off[1]; io.state = d + h.off[2];
    io.adam_m = l.adam_m.p; io.adam_v = l.adam_v.p;
    if (n_feed) BF_TRY(lane_feed(b, j, in_open, n_feed));
    HIP_TRY(bf_fit_launch(&b->m->fit, &io, &l.open_hd, l.open_iters, 0, b->adam_tab.p, 0, b->fit_smem, l.stream, nullptr));
    // the group's hand-over: by the tail's own kernels where they store into the mirror (calls below 16 frames), else behind them
    BF_TRY(bf_enqueue_tail(b, r, h.off, G * b->F, b->F, {l.stream, &l.scratch, l.vraw.p, l.xpart.p}, h.total, true, true,
                           h.total * sizeof(float) >= kLaneCopyBytes));
    l.held = h;
    r.seq = h.seq0 + G - 1; r.fetched = r.has_v = true;         // (the arena's newest fit: what a trade in bf_lanes_drain hands on)
    L.launches += 1;
    L.max_g = std::max(L.max_g, G);
    return BF_OK;
}

// Every other entry point finds the last fit where the tail-aside path leaves one - in the result arena the previous fit did not use, with
// its Adam moments as the batch's - and the inputs the views name on the device.
int bf_lanes_drain(bf_batch *b) {
    BfLanes &L = b->lanes;
    if (!L.on) return BF_OK;
    b->in_at.pinned = false;              // (what follows a drain may write the device slot alone: a setter, a device-side producer)
    // 1. the open groups go out, where calls have joined one (or a slot was staged)
    for (int j = 0; j < L.n; ++j) BF_TRY(lane_launch(b, j));
    L.on = false;
    BfLane *const l = L.last >= 0 ? &L.lane[L.last] : nullptr;        // the lane that holds the last lane fit, in its newest group's last slot
    L.last = -1;
    const int k = b->cur ^ 1;
    ResultArena &r = b->arena[k];
    // (the second stream no longer uses arena k: a deferred tail is enqueued and a pipelined fetch of the arena waited for, on the host)
    auto release_arena_k = [&]() -> int {
        BF_TRY(bf_flush_tail(b));
        if (r.copy_pending) { HIP_TRY(hipEventSynchronize(r.ev_copied)); r.copy_pending = false; }
        return BF_OK;
    };
    // 2. (W > 1) A group's arena is laid out for G calls: the last slot's five slices and its two Adam-moment rows are copied, device to
    // device, by ONE launch on the lane's own stream - behind that lane's fit, tail and hand-over, so it ends with the lane instead of
    // starting a chain of copy commands after every lane has been waited for (a bracket ends in exactly one drain: this is on its path).
    // Nothing on the device still uses arena k or the batch's moments when this launch runs:
    //  - the batch stream: the lane has fitted since the lanes took over, so its stream has waited for ev_engage (lane_begin), which
    //    lanes_engage recorded behind everything on the batch stream; and while the lanes are on nothing is issued there - every entry
    //    point but a lane fit or a staging comes through this drain first, and a staging with W > 1 issues no GPU work;
    //  - the second stream: release_arena_k, just before;
    //  - the other lanes use their own arenas and moments, and of the batch's only inputs, cameras and the Adam table - not written here.
    // And nothing reads them before this launch has finished: the lane's stream is waited for in step 3, before this function returns.
    const bool by_kernel = l && L.W > 1 && l->held.G > 0;
    if (by_kernel) {
        BF_TRY(release_arena_k());
        const BfLane::Held &h = l->held;
        const size_t s = h.G - 1, n_adam = (size_t)b->F * b->m->np;
        BfSegs<7> seg;
        for (int i = 0; i < 5; ++i) {
            seg.src[i] = l->arena.dev.p + h.off[i] + s * b->res_cnt[i]; seg.dst[i] = r.dev.p + b->res_off[i]; seg.n[i] = (unsigned)b->res_cnt[i];
        }
        seg.src[5] = l->adam_m.p + s * n_adam; seg.dst[5] = b->adam_m.p; seg.n[5] = (unsigned)n_adam;
        seg.src[6] = l->adam_v.p + s * n_adam; seg.dst[6] = b->adam_v.p; seg.n[6] = (unsigned)n_adam;
        BF_TRY(publish_segs(l->stream, seg));
    }
    // 3. the lanes that were given work finish
    for (int q = 0; q < L.n; ++q)
        if (L.lane[q].busy) { HIP_TRY(hipStreamSynchronize(L.lane[q].stream)); L.lane[q].busy = false; }
    if (!l) return BF_OK;                 // (inputs staged, no lane fit since the lanes took over)
    // 4. the hand-back finishes on the host.  (W = 1, or no group to hand back: nothing on the device uses either side any more - the lane
    // waited for the batch stream before its fit and has finished.)
    if (!by_kernel) BF_TRY(release_arena_k());
    if (!l->held.G) {                     // (its launch failed: no result anywhere)
        b->fetched = b->have_result = false;
        return fail(BF_ERR_HIP, "fit lanes: the last lane fit was not launched");
    }
    if (L.W == 1) {
        // equal-sized buffers: by trading them - the lane takes the batch's arena k and moments (its next fit overwrites them), no
        // copy; the graphs captured with the old addresses are dropped
        r.trade_buffers(l->arena);
        l->held = BfLane::Held{};
        std::swap(b->adam_m.p, l->adam_m.p);
        std::swap(b->adam_v.p, l->adam_v.p);
        if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
        for (auto &g : b->graph_pipe) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    } else {
        // mirror to mirror, now that the lane's hand-over has been waited for.  The group stays readable in the lane (bf_lanes_find).
        const BfLane::Held &h = l->held;
        const size_t s = h.G - 1;
        for (int i = 0; i < 5; ++i)
            std::memcpy(r.host + b->res_off[i], l->arena.host + h.off[i] + s * b->res_cnt[i], b->res_cnt[i] * sizeof(float));
        r.seq = h.seq0 + (long long)s; r.fetched = r.has_v = true;
    }
    // 5. the batch's views and mirrors move to arena k
    bf_use_arena(b, k);
    return BF_OK;
}

// input arena `in_next` of lane l is opened for a new group.  Its pinned buffer may still be read by the transfer of the group it held -
// issued two of this lane's groups ago, behind fits that have normally long finished: the host waits only if that transfer has not
// completed (the back-pressure of a feeder that runs ahead of the device).  W = 1 leaves that wait to bf_pack_staging, unconditional and
// uncounted as before groups.
static int lane_open(bf_batch *b, BfLane &l, bool host_fed) {
    l.open = true; l.open_host = host_fed;
    l.open_a = l.in_next; l.in_next ^= 1;
    InputArena &in = l.in[l.open_a];
    if (host_fed && b->lanes.W > 1 && in.pending) {
        if (hipEventQuery(in.ev) != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(hipEventSynchronize(in.ev));
            b->lanes.feed_waits += 1;
        }
        in.pending = false;
    }
    return BF_OK;
}

int bf_lanes_stage(bf_batch *b, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose) {
    BF_TRY(lanes_engage(b));
    BfLanes &L = b->lanes;
    const int W = L.W;
    if (L.lane[L.next].n_open && bf_lane_feed_differs(W, L.lane[L.next].open_host, true)) BF_TRY(lane_launch(b, L.next));   // (a device-fed group: it goes out first)
    const int j = L.next;                   // (the lane the next frame-after-frame fit joins)
    BfLane &l = L.lane[j];
    BF_TRY(lane_begin(b, l));
    // W = 1: no call has joined (a launch per call: n_open is 0 between calls), and every staging takes the lane's other arena - a staging
    // after a staging does not wait for the first one's transfer.  W > 1: a second staging before a fit rewrites the same slot of the open arena.
    if (W == 1 ? !l.n_open : !l.open) BF_TRY(lane_open(b, l, true));
    InputArena &in = l.in[l.open_a];
    if (W > 1) {
        // Host-fed groups: NO GPU work here.  The call's inputs are packed into slot n_open of the open arena's pinned buffer and the
        // views point at the slot's place on the device, which the group's one transfer fills when the group is launched (lane_launch;
        // every drain comes through there, so whoever reads the views on the device finds them filled).  Until then the pinned slot is the
        // only valid copy: InputCursor::pinned.
        bf_pack_slot(L.gin, in.host, l.n_open, bf_init_map(b->m), b->F, b->V, keypoints, n_use_frames, init_betas, init_pose);
    } else {
        // a launch per call: the slot is the arena, filled by a transfer of its own at once (the call sequence before groups)
        BF_TRY(bf_pack_staging(b, in.host, in.ev, in.pending, keypoints, n_use_frames, init_betas, init_pose));      // (its last transfer: queued two of this lane's groups ago)
        BF_TRY(lane_feed(b, j, in, 1));
    }
    use_lane_inputs(b, j, l.open_a, l.n_open, W > 1);
    l.slot_staged = true;
    b->staged = true;
    return BF_OK;
}

// The call joins the open group of the next lane - its inputs are in the group's next slot: staged there, or copied from the batch's
// current inputs now, on the host where their pinned copy is valid and on the device otherwise - and the group is launched if its lane is
// idle or it is full (lane_launch).  A group is host-fed or device-fed, never both: a call of the other kind launches the open group
// first, as a call with other iterations or hyper-parameters does.
int bf_lanes_fit(bf_batch *b, int n_iters, const HyperDev &hd) {
    BF_TRY(lanes_engage(b));
    BfLanes &L = b->lanes;
    const int W = L.W;
    {
        BfLane &o = L.lane[L.next];
        if (o.n_open && bf_lane_close_first(W, o.open_iters, n_iters, &o.open_hd, &hd, sizeof hd, o.open_host, o.slot_staged || b->in_at.pinned))
            BF_TRY(lane_launch(b, L.next));
    }
    const int j = L.next;
    BfLane &l = L.lane[j];
    BF_TRY(lane_begin(b, l));
    b->fetched = false; b->have_result = false;                 // (a failure from here on: nothing of this call may be read)
    const int slot = l.n_open;
    // the feed, for the idle rule below: ONE clock read per call
    const auto now = std::chrono::steady_clock::now();
    const bool called_before = L.called;
    const auto t_prev = L.t_call;
    L.t_call = now; L.called = true;
    if (slot == 0) { l.open_seq0 = b->fit_seq; l.open_iters = n_iters; l.open_hd = hd; l.borrowed = false; l.t_first = now; }
    if (!l.slot_staged && W == 1) {
        // a launch per call: the fit reads the current inputs in place.  Another lane's slot is read without a wait for its transfer,
        // as before groups (width 1 is that call sequence): the transfer went out on its lane ahead of a fit launch that has since
        // been issued
        l.borrowed = true;
        l.bor_kp = b->keypoints.p; l.bor_p0 = b->params0.p; l.bor_ndiv = b->ndiv.p;
        if (b->in_at.on_lane) current_arena(b).readers |= 1u << j;
    } else if (!l.slot_staged && b->in_at.pinned) {
        // No staging of its own, and the pinned mirror of the slot the views are on holds the current inputs (the usual re-fit): copied
        // on the host into this group's next slot - no device copy, no event - and the views move there.
        // INVARIANT: the source is the previous call's slot at the latest (every host-fed call leaves the views on its own slot), so its
        // arena belongs to the newest group of its lane or to the open one, and a pinned arena is rewritten only when its lane opens it
        // again two groups later - which takes calls that would have moved the views on.  The source is never the slot written here.
        if (!l.open) BF_TRY(lane_open(b, l, true));
        const InputArena &src = current_arena(b);
        InputArena &dst = l.in[l.open_a];
        assert(!(&src == &dst && b->in_at.slot == slot) && "a re-fit's pinned source is the previous call's slot, never the one it joins");
        bf_copy_slot(L.gin, dst.host, slot, src.host, b->in_at.slot);
        use_lane_inputs(b, j, l.open_a, slot, true);
        L.feed_host_copies += 1;
    } else if (!l.slot_staged) {
        // no staging of its own, the current inputs in device memory only (after a synchronous setter, a device-side producer, a drain):
        // whatever keypoints / params0 / ndiv point at, copied on the lane's stream.  A lane slot they point at was filled before the
        // drain that left them there: nothing to wait for; its arena's next transfer waits for this copy (`readers`).
        if (!l.open) BF_TRY(lane_open(b, l, false));
        const SlotPlace at = slot_place(b, l.in[l.open_a], slot);
        if (at.kp != b->keypoints.p) {                          // (else they are this very slot's)
            if (b->in_at.on_lane && b->in_at.lane != j) current_arena(b).readers |= 1u << j;
            BF_TRY(publish_segs(l.stream, BfSegs<3>{{b->keypoints.p, b->params0.p, (const float *)b->ndiv.p}, {at.kp, at.p0, (float *)at.ndiv},
                                                    {(unsigned)b->keypoints.n, (unsigned)b->params0.n, (unsigned)b->ndiv.n}}));
            HIP_TRY(hipEventRecord(l.ev_join, l.stream));
            L.feed_dev_copies += 1;
        }
    }
    l.open = true; l.slot_staged = false;
    l.n_open = slot + 1;
    L.last = j;
    L.calls += 1;
    // Full: behind the lane's running group, in stream order.  Else the lane is idle: now - a slow feeder waits for nobody, and a fast
    // feeder's first call after a pause goes out alone - UNLESS the feeder is fast (the call before this one came less than H ago) and the
    // group is young (its first call joined less than H ago).  Then it is held exactly as a group behind a busy lane is: a burst fills
    // groups instead of sending its first calls out one by one, each a whole launch sequence and a lane cycle for one frame.  The group
    // goes out when it is full, at the first call that finds the feeder slow or the group H old, and at every read, drain, sync or
    // destroy - H bounds what the rule adds to a burst's frames.  W = 1 and H = 0: the idle rule alone.
    const BfLaneAfterJoin next = bf_lane_after_join(W, l.n_open, fit_lane_fill(), fit_lane_hold(), now, called_before, t_prev, l.t_first);
    if (next == BfLaneAfterJoin::LAUNCH) return lane_launch(b, j);
    if (next == BfLaneAfterJoin::IF_IDLE) {
        const hipError_t q = hipEventQuery(l.arena.ev_copied);
        if (q == hipSuccess) return lane_launch(b, j);
        (void)hipGetLastError();
        if (q != hipErrorNotReady) HIP_TRY(q);
    }
    return BF_OK;
}

int bf_lanes_find(bf_batch *b, long long seq, BfLaneResult &at) {
    BfLanes &L = b->lanes;
    at = BfLaneResult{};
    // a lane keeps its group until its next launch: the fit is in a launched group, or in the open one, which then goes out now
    for (int j = 0; L.lane && seq >= 0 && j < L.n; ++j) {
        BfLane &l = L.lane[j];
        if (l.n_open && seq >= l.open_seq0 && seq < l.open_seq0 + l.n_open) BF_TRY(lane_launch(b, j));
        if (l.held.G && seq >= l.held.seq0 && seq < l.held.seq0 + l.held.G) {
            at.arena = &l.arena;
            for (int i = 0; i < 5; ++i) at.off[i] = l.held.off[i] + (size_t)(seq - l.held.seq0) * b->res_cnt[i];
        }
    }
    return BF_OK;
}

void bf_lanes_destroy(bf_batch *b) {
    for (int j = 0; b->lanes.lane && j < b->lanes.n; ++j)          // (calls that joined a group were promised a fit: it goes out before the wait)
        if (b->lanes.lane[j].n_open && hipSetDevice(b->m->device) == hipSuccess) (void)lane_launch(b, j);
    lanes_release(b);                     // (waits for the lanes' work: it reads the batch's inputs, cameras and Adam table)
}

extern "C" {
/* test hook: fit-lane groups since the batch was created - out[0] lane launches, out[1] lane calls, out[2] the largest group, out[3] W */
int bf_batch_lane_stats(bf_batch *b, int32_t out[4]) {
    if (!b || !out) return fail(BF_ERR_INVALID, "bf_batch_lane_stats: null argument");
    const BfLanes &L = b->lanes;
    out[0] = L.launches; out[1] = L.calls; out[2] = L.max_g; out[3] = L.n > 1 ? L.W : 1;
    return BF_OK;
}

/* test hook: how the fit lanes were fed - out[0] input transfers, out[1] host-side slot copies, out[2] device-side slot copies, out[3] host
 * waits on a pinned arena */
int bf_batch_lane_feed_stats(bf_batch *b, int64_t out[4]) {
    if (!b || !out) return fail(BF_ERR_INVALID, "bf_batch_lane_feed_stats: null argument");
    const BfLanes &L = b->lanes;
    out[0] = L.feed_transfers; out[1] = L.feed_host_copies; out[2] = L.feed_dev_copies; out[3] = L.feed_waits;
    return BF_OK;
}
}  // extern "C"
