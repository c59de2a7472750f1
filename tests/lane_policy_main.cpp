// Host-only run of the fit lanes' decisions (bodyfitting_amd/csrc/lane_policy.h), built with the host compiler under
// -fsanitize=address,undefined by tests/test_lane_policy.py.  The program only EVALUATES the three functions over the case lists below and
// prints one line per case - inputs, "->", result; the test works the expected results out itself from the rules as the issue states them
// and holds every line to them.
//   size  n_cus F lanes_wanted width_wanted zerocopy -> n_lanes W
//   close W iters_differ hyper_differ feed_differs -> 0 | 1        (and "feed W open_host host_fed -> 0 | 1" for bf_lane_feed_differs alone)
//   join  W n_open fill H_us called_before gap_prev_ns gap_first_ns -> launch | if_idle | hold
#include "lane_policy.h"

#include <cstdio>
#include <set>

int main() {
    const int Fs[] = {1, 2, 7, 8, 9, 32, 33, 64, 128, 129, 256, 300}, wanted_lanes[] = {1, 4, 32}, wanted_width[] = {1, 32, 64};
    for (int n_cus : {256, 0})          // 0: the attribute could not be read
        for (int F : Fs) for (int lanes : wanted_lanes) for (int width : wanted_width) for (int zc = 0; zc < 2; ++zc) {
            const BfLaneSizing s = bf_lane_sizing(n_cus, F, lanes, width, zc != 0);
            std::printf("size %d %d %d %d %d -> %d %d\n", n_cus, F, lanes, width, zc, s.n_lanes, s.W);
        }

    // hyper-parameters as the caller holds them: a struct compared as bytes; the difference is in the last byte alone
    struct Hyper { float a[8]; unsigned char tail[4]; };
    const Hyper h0{{1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f}, {1, 2, 3, 4}};
    for (int W : {1, 2, 32})
        for (int di = 0; di < 2; ++di) for (int dh = 0; dh < 2; ++dh) for (int df = 0; df < 2; ++df) for (int open_host = 0; open_host < 2; ++open_host) {
            Hyper h1 = h0;
            if (dh) h1.tail[3] ^= 0x80;
            const bool host_fed = df ? !open_host : open_host != 0;
            std::printf("close %d %d %d %d -> %d\n", W, di, dh, df, (int)bf_lane_close_first(W, 100, di ? 99 : 100, &h0, &h1, sizeof h0, open_host != 0, host_fed));
            std::printf("feed %d %d %d -> %d\n", W, open_host, (int)host_fed, (int)bf_lane_feed_differs(W, open_host != 0, host_fed));
        }

    const BfLaneTime base = BfLaneTime() + std::chrono::hours(1);
    const char *names[] = {"launch", "if_idle", "hold"};
    for (int W : {1, 2, 32}) {
        const std::set<int> n_opens = {1, std::max(W - 1, 1), W};
        for (int n_open : n_opens) for (int fill = 0; fill < 2; ++fill) for (long long H : {0ll, 100ll}) {
            // gaps of 0, H - 1 us, H, H + 1 us, and a nanosecond either side of H: the comparisons are strict at the clock's own resolution
            std::set<long long> gaps = {0, H * 1000, (H + 1) * 1000, H * 1000 + 1};
            if (H > 0) { gaps.insert((H - 1) * 1000); gaps.insert(H * 1000 - 1); }
            for (int called = 0; called < 2; ++called) for (long long gp : gaps) for (long long gf : gaps) {
                const BfLaneTime now = base + std::chrono::seconds(1);
                const BfLaneAfterJoin r = bf_lane_after_join(W, n_open, fill != 0, std::chrono::microseconds(H), now, called != 0,
                                                             now - std::chrono::nanoseconds(gp), now - std::chrono::nanoseconds(gf));
                std::printf("join %d %d %d %lld %d %lld %lld -> %s\n", W, n_open, fill, H, called, gp, gf, names[(int)r]);
            }
        }
    }
    return 0;
}
