// A device-route workspace's decisions (bodyfitting_amd/csrc/workspace_policy.h) run through the call sequences of a torch loop, with
// plain vectors standing for the device blocks: built under AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_workspace_policy.py.  Prints one "ok <name>" line per property.
#include "workspace_policy.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// a workspace as dev_route_api.hip keeps one: a block per slot, replaced when the plan says so
struct Ws {
    BfWsPlan plan;
    std::vector<std::vector<char>> block;
    int allocations = 0;
    void call(const std::vector<size_t> &requests) {
        plan.begin();
        for (size_t bytes : requests) {
            bool grow = false;
            size_t alloc = 0;
            const size_t k = plan.take(bytes, &grow, &alloc);
            if (k >= block.size()) block.resize(k + 1);
            if (grow) { block[k].assign(alloc, 0); plan.commit(k, alloc); ++allocations; }
            CHECK(block[k].size() >= bytes && block[k].size() >= 1);
            if (bytes) block[k][bytes - 1] = 1;           // (the sanitizer watches the last byte the call may touch)
        }
    }
};

int main() {
    const std::vector<size_t> forward = {4096, 83 * 1024, 0, 600, 540}, reverse = {4096, 83 * 1024, 83 * 1024, 83 * 1024, 288, 500000, 1500, 288, 40};
    {   // a loop of forward and reverse calls: every allocation happens in the first round
        Ws w;
        w.call(forward); w.call(reverse);
        const int first = w.allocations;
        CHECK(first >= (int)reverse.size());
        for (int i = 0; i < 10; ++i) { w.call(forward); w.call(reverse); }
        CHECK(w.allocations == first);
        std::printf("ok settles\n");
    }
    {   // grow-only: a smaller call behind a larger one keeps the blocks, a larger one replaces exactly the slots that are too small
        Ws w;
        w.call({1000, 1000, 1000});
        CHECK(w.allocations == 3);
        w.call({10, 10});
        CHECK(w.allocations == 3);
        w.call({1000, 1025, 1000, 7});
        CHECK(w.allocations == 5);                        // slot 1 (1024 held: 1000 rounded up) and the new slot 3
        CHECK(w.plan.have[1] == 1280 && w.plan.have[0] == 1024);
        std::printf("ok grow_only\n");
    }
    {   // sizes are rounded up to 256 bytes, an empty request still gets a block, a request that fits exactly does not grow
        CHECK(BfWsPlan::rounded(0) == 256 && BfWsPlan::rounded(1) == 256 && BfWsPlan::rounded(256) == 256 && BfWsPlan::rounded(257) == 512);
        Ws w;
        w.call({0}); w.call({256}); w.call({0});
        CHECK(w.allocations == 1);
        std::printf("ok rounding\n");
    }
    {   // a replacement that failed leaves the slot empty: the next call allocates it again
        BfWsPlan p;
        bool grow = false;
        size_t alloc = 0;
        p.begin();
        size_t k = p.take(100, &grow, &alloc);
        CHECK(grow && alloc == 256);
        p.commit(k, alloc);
        p.begin();
        k = p.take(1000, &grow, &alloc);
        CHECK(grow && k == 0);
        p.lose(k);                                        // (the old block was given up, the new one did not come)
        p.begin();
        k = p.take(10, &grow, &alloc);
        CHECK(grow && alloc == 256);
        std::printf("ok failed_growth\n");
    }
    {   // the stream switch: only a call behind another call, on another stream, waits
        int a = 0, b = 0;
        CHECK(!bf_ws_must_wait(false, nullptr, &a));      // the first call
        CHECK(!bf_ws_must_wait(true, &a, &a));
        CHECK(bf_ws_must_wait(true, &a, &b));
        CHECK(bf_ws_must_wait(true, &a, nullptr) && bf_ws_must_wait(true, nullptr, &a));      // (the null stream is a stream)
        CHECK(!bf_ws_must_wait(true, nullptr, nullptr));
        std::printf("ok stream_switch\n");
    }
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
