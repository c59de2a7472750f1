// The two routes of the stateless calls a torch loop goes through (model_grad_api.hip, kp_loss_api.hip, mesh_loss_api.hip), and the
// device route's workspace (include/bodyfit.h: bf_workspace_create, the *_dev entry points).  Each of those calls is ONE body that issues
// its kernels on a BfRouteCall; the call knows where the arrays live:
//   host route    (no workspace) host arrays, the NULL stream, buffers from the device's block cache, the device drained at the end
//   device route  (a workspace)  device arrays read and written where they lie, the caller's stream, scratch from the workspace - the
//                 scratch of ONE caller -, nothing drained and nothing copied to the host
// The block cache (BfPool) stays out of the device route: "nothing on the device still uses a block that is given back" is what a route
// that never synchronises cannot promise.  Defined in dev_route_api.hip.
#pragma once
#include "bf_host.h"
#include "workspace_policy.h"

struct bf_workspace {
    int device = 0;
    hipEvent_t ev = nullptr;            // recorded at the end of every call, on that call's stream
    bool used = false;                  // ... which `last` names
    hipStream_t last = nullptr;
    BfWsPlan plan;                      // which slot a request gets and when it grows (workspace_policy.h)
    std::vector<void *> slot;
    MeshScratch scratch;                // the mesh pass's matrix-core path: grown by bf_grow on the call's stream
    // the keypoint loss's divisor[n]: the one host array of that call, staged in pinned memory and sent on the call's stream.  What was
    // sent last is remembered: a loop's divisor does not change, and then nothing is sent.
    int *h_div = nullptr;
    size_t h_div_n = 0;
    DevBuf<int> d_div;
    std::vector<int> div_sent;
};
// divisor[n] on the device, behind `stream`'s earlier work
int bf_ws_divisor(bf_workspace *ws, hipStream_t stream, const int *divisor, size_t n, const int **dev);

// the thread's current device as the caller left it: with one HIP runtime in the process it is torch's too
struct BfDeviceGuard {
    int prev = -1;
    explicit BfDeviceGuard(bool on = true) { if (on && hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~BfDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// One call on either route, from begin() to finish(), and every buffer its kernels touch.  ws = NULL: the host route.
//   begin    host: the device is set, and stays set.  device: the device is set until the call ends, and `stream` waits for the
//            workspace's previous call when that ran on another stream
//   in       an array the kernels read       host: uploaded into a block of the cache      device: the array itself
//   out      an array the caller may want    host: a block, copied to dst by finish()       device: dst itself
//            dst NULL: nothing (the kernels read a NULL output as "not wanted"), or with `always` - the kernels write it whoever
//            wants it - a block / a workspace slot that goes nowhere
//   scratch  contents undefined              host: a block                                  device: the workspace's next slot
//   finish   host: the device is drained, then the noted copies.  device: nothing waits
// On every way out the host route drains the device before its blocks go back to the cache, and the device route records the
// workspace's event behind whatever the call queued.
struct BfRouteCall {
    bf_workspace *const ws;
    const hipStream_t stream;
    BfRouteCall(bf_workspace *w, hipStream_t s) : ws(w), stream(w ? s : nullptr), keep(w != nullptr) {}
    BfRouteCall(const BfRouteCall &) = delete;
    ~BfRouteCall();
    int begin(int device);
    int finish();
    MeshScratch *mesh_scratch() { return ws ? &ws->scratch : &own_scratch; }

    template <class T>
    int in(const T *src, size_t count, const T *&p) {
        p = src;
        if (ws || !src) return BF_OK;
        T *d = nullptr;
        BF_TRY(scratch(count, d));
        p = d;
        if (count) HIP_TRY(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
        return BF_OK;
    }
    template <class T>
    int out(T *dst, size_t count, T *&p, bool always = false) {
        p = ws ? dst : nullptr;
        if (p || (!dst && !always)) return BF_OK;
        BF_TRY(scratch(count, p));
        if (dst) back.push_back({dst, p, count * sizeof(T)});
        return BF_OK;
    }
    template <class T>
    int scratch(size_t count, T *&p) {
        void *v = nullptr;
        BF_TRY(block(std::max<size_t>(count, 1) * sizeof(T), &v));
        p = (T *)v;
        return BF_OK;
    }

private:
    struct Owned { void *p; size_t bytes; };
    struct Back { void *dst; const void *src; size_t bytes; };
    int block(size_t bytes, void **p);
    BfDeviceGuard keep;                 // (device route)
    bool begun = false;
    int device = 0;
    std::vector<Owned> owned;           // (host route) the cache's blocks of this call
    std::vector<Back> back;             // ... and the device-to-host copies finish() makes
    MeshScratch own_scratch;            // ... and the mesh pass's scratch, freed behind the destructor's drain
};

// what the *_dev entry points of mesh_loss_api.hip and scan_api.hip check before anything is queued: -> BF_OK, or the refusal
int bf_ml_check_count(const char *who, const char *what, int n);                // 0 < n <= 2^28 vertices, faces or points of one call
int bf_ml_dev_check(const char *who, const bf_workspace *ws, int device);      // a workspace, and one of that device
// the scan's ScanDev in device memory (scan_api.hip): resident, made once per scan / where the kernels of `c` read it
int bf_scan_resident(struct bf_scan *s, const ScanDev **out);
int bf_ml_scan_dev(BfRouteCall &c, struct bf_scan *s, const ScanDev *&d_s);
