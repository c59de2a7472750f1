// The decisions of a device-route workspace (bf_workspace, dev_route.h) as plain C++: which of its slots a call's buffers land in, when
// a slot has to be replaced, and when a call has to wait for the one before it.  No HIP in here: tests/test_workspace_policy.py compiles
// this with a main of its own.
//
// A call asks for its buffers one after another; the k-th request of a call gets slot k, whatever entry point the call is.  A slot only
// grows: it is replaced when a request is larger than what it holds, and then holds that request rounded up to 256 bytes.  Entry points
// that share a workspace (a model's forward and its reverse) ask for different sizes in the same position, so every slot settles at the
// largest request it has met: from the second round of the same calls on nothing is allocated.
#pragma once
#include <cstddef>
#include <vector>

struct BfWsPlan {
    std::vector<size_t> have;       // bytes slot k holds (0: nothing yet)
    size_t cursor = 0;              // the slot the next request of the call in progress gets

    void begin() { cursor = 0; }
    static size_t rounded(size_t bytes) { return ((bytes ? bytes : 1) + 255) & ~(size_t)255; }
    // the next request of the call: -> its slot; *grow: the slot has to be replaced by one of *alloc_bytes first (then `commit` it)
    size_t take(size_t bytes, bool *grow, size_t *alloc_bytes) {
        const size_t k = cursor++;
        if (k >= have.size()) have.resize(k + 1, 0);
        *grow = have[k] < bytes || have[k] == 0;
        *alloc_bytes = *grow ? rounded(bytes) : have[k];
        return k;
    }
    void commit(size_t k, size_t alloc_bytes) { have[k] = alloc_bytes; }       // the replacement succeeded
    void lose(size_t k) { have[k] = 0; }                                       // ... or failed after the old block was given up
};

// A call on `stream` behind a call that ended on `last`: on another stream it first waits for the event recorded at that call's end.
inline bool bf_ws_must_wait(bool used, const void *last, const void *stream) { return used && last != stream; }
