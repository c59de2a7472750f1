// Host side of bf_workspace_create / bf_workspace_destroy / bf_device_pointer_check / bf_dev_route_stats (include/bodyfit.h), of the
// workspace the *_dev entry points run on - grow-only device buffers, one event, no block cache - and of the call context both routes
// of an entry point share (BfRouteCall, dev_route.h).
#include "dev_route.h"

extern "C" int bf_workspace_create(int device, bf_workspace **out) {
    if (!out) return fail(BF_ERR_INVALID, "bf_workspace_create: bad argument");
    *out = nullptr;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<bf_workspace> ws(new bf_workspace);
    ws->device = device;
    HIP_TRY(hipEventCreateWithFlags(&ws->ev, hipEventDisableTiming));
    *out = ws.release();
    return BF_OK;
}

extern "C" void bf_workspace_destroy(bf_workspace *ws) {
    if (!ws) return;
    BfDeviceGuard keep;
    (void)hipSetDevice(ws->device);
    if (ws->used) (void)hipStreamSynchronize(ws->last);          // the last call's work: every earlier call is ordered in front of it
    for (void *p : ws->slot)
        if (p) (void)hipFree(p);
    if (ws->h_div) (void)hipHostFree(ws->h_div);
    if (ws->ev) (void)hipEventDestroy(ws->ev);
    delete ws;
}

int BfRouteCall::begin(int dev) {
    HIP_TRY(hipSetDevice(dev));
    device = dev;
    begun = true;
    if (!ws) return BF_OK;
    ws->plan.begin();
    if (bf_ws_must_wait(ws->used, ws->last, stream)) {
        HIP_TRY(hipStreamWaitEvent(stream, ws->ev, 0));
        ++bf_route_stats().switches;
    }
    return BF_OK;
}

int BfRouteCall::finish() {
    HIP_TRY(hipGetLastError());
    if (ws) return BF_OK;
    HIP_TRY(hipDeviceSynchronize());
    for (const Back &b : back) HIP_TRY(hipMemcpy(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost));
    return BF_OK;
}

BfRouteCall::~BfRouteCall() {
    if (!begun) return;
    if (!ws) {
        (void)hipDeviceSynchronize();         // whatever path leaves the call, no kernel still uses a block when it goes back to the cache
        for (const Owned &b : owned) bf_pool_free(b.p, b.bytes, device);
        return;
    }
    // (on a failed record the next call on another stream would wait for an older end: drain instead, once)
    if (hipEventRecord(ws->ev, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); }
    ws->used = true;
    ws->last = stream;
}

// the call's next buffer of `bytes` (contents undefined)
int BfRouteCall::block(size_t bytes, void **p) {
    if (!ws) {
        size_t got = 0;
        HIP_TRY(bf_pool_alloc(p, bytes, &got));
        owned.push_back({*p, got});
        return BF_OK;
    }
    bool grow = false;
    size_t alloc_bytes = 0;
    const size_t k = ws->plan.take(bytes, &grow, &alloc_bytes);
    if (k >= ws->slot.size()) ws->slot.resize(k + 1, nullptr);
    if (grow) {
        if (ws->slot[k]) {
            // its last user is an earlier call (a call takes every slot once): that call's stream has drained when this returns, and
            // a call in between on another stream waited for it
            if (ws->used) HIP_TRY(hipStreamSynchronize(ws->last));
            (void)hipFree(ws->slot[k]);
            ws->slot[k] = nullptr;
            ws->plan.lose(k);
        }
        HIP_TRY(hipMalloc(&ws->slot[k], alloc_bytes));
        ws->plan.commit(k, alloc_bytes);
        ++bf_route_stats().allocs;
    }
    *p = ws->slot[k];
    return BF_OK;
}

int bf_ws_divisor(bf_workspace *ws, hipStream_t stream, const int *divisor, size_t n, const int **dev) {
    if (ws->d_div.p && ws->div_sent.size() == n && std::equal(divisor, divisor + n, ws->div_sent.begin())) {
        *dev = ws->d_div.p;                   // (sent by an earlier call, which this one is ordered behind)
        return BF_OK;
    }
    // new values: the staging block and the device array are free once the previous call - the last that may read either - has ended
    if (ws->used) HIP_TRY(hipEventSynchronize(ws->ev));
    ws->div_sent.clear();
    if (ws->h_div_n < n) {
        if (ws->h_div) { (void)hipHostFree(ws->h_div); ws->h_div = nullptr; ws->h_div_n = 0; }
        HIP_TRY(hipHostMalloc((void **)&ws->h_div, n * sizeof(int)));
        ws->h_div_n = n;
        ws->d_div.release();
        HIP_TRY(ws->d_div.alloc(n));
        ++bf_route_stats().allocs;
    }
    std::memcpy(ws->h_div, divisor, n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(ws->d_div.p, ws->h_div, n * sizeof(int), hipMemcpyHostToDevice, stream));
    ws->div_sent.assign(divisor, divisor + n);
    *dev = ws->d_div.p;
    return BF_OK;
}

extern "C" int bf_device_pointer_check(int device, const void *p) {
    if (!p) return BF_ERR_INVALID;
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();              // (an address this runtime has never seen is an error there: not one to leave behind)
        return BF_ERR_INVALID;
    }
    return (a.type == hipMemoryTypeDevice && a.device == device) ? BF_OK : BF_ERR_INVALID;
}

extern "C" int bf_dev_route_stats(int64_t out[4]) {
    if (!out) return fail(BF_ERR_INVALID, "bf_dev_route_stats: bad argument");
    const BfRouteStats &S = bf_route_stats();
    out[0] = S.host; out[1] = S.dev; out[2] = S.allocs; out[3] = S.switches;
    return BF_OK;
}
