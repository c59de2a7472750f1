// The device route's workspace (include/bodyfit.h: bf_workspace_create, the *_dev entry points): the scratch of ONE caller, on whatever
// stream that caller runs.  Defined in dev_route_api.hip, used by the *_dev entry points of model_grad_api.hip, kp_loss_api.hip and mesh_loss_api.hip.
// The block cache (BfPool) stays out of this route: "nothing on the device still uses a block that is given back" is what a route that
// never synchronises cannot promise.
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

// One call on a workspace, from its first buffer to its last launch: begin() makes `stream` wait for the workspace's previous call when
// that ran on another stream; the destructor records the workspace's event behind whatever the call queued, on every way out.
struct BfWsCall {
    bf_workspace *const ws;
    const hipStream_t stream;
    bool begun = false;
    BfWsCall(bf_workspace *w, hipStream_t s) : ws(w), stream(s) {}
    int begin();
    ~BfWsCall();
};
// the call's next buffer of `bytes` (contents undefined)
int bf_ws_take(bf_workspace *ws, size_t bytes, void **p);
// divisor[n] on the device, behind `stream`'s earlier work
int bf_ws_divisor(bf_workspace *ws, hipStream_t stream, const int *divisor, size_t n, const int **dev);

// the thread's current device as the caller left it: with one HIP runtime in the process it is torch's too
struct BfDeviceGuard {
    int prev = -1;
    BfDeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~BfDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
