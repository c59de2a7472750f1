// The decisions that shape a fit-lane bracket - plain C++, no HIP, no clock reads (time points come in as arguments): lanes.hip calls each
// at the one place the decision is taken, tests/lane_policy_main.cpp checks them on the host alone under the sanitizers.
//   bf_lane_sizing       how many lanes a batch gets and how many calls a lane launch carries at most (bf_lanes_configure)
//   bf_lane_close_first  whether the open group must go out before a call joins (bf_lanes_fit; bf_lane_feed_differs alone: bf_lanes_stage)
//   bf_lane_after_join   what happens to the group a call has just joined (bf_lanes_fit)
#pragma once
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>

// One frame's fit per CU: at most CUs / frames lanes, and none with zero-copy staging; a lane launch carries up to W calls' frames, the
// lanes' groups together at most a frame per CU.  n_cus <= 0 (the attribute could not be read) counts as one CU.
struct BfLaneSizing { int n_lanes, W; };
inline BfLaneSizing bf_lane_sizing(int n_cus, int F, int lanes_wanted, int width_wanted, bool zerocopy) {
    const int cus = std::max(n_cus, 1);
    const int d = std::min(lanes_wanted, cus / F);
    const int n_lanes = (!zerocopy && d > 1) ? d : 1;
    return {n_lanes, std::min(width_wanted, std::max(1, cus / (n_lanes * F)))};
}

// A group is host-fed or device-fed, never both (W = 1 has no such kinds: its one call reads a slot of its own or the current inputs in place)
inline bool bf_lane_feed_differs(int W, bool open_host, bool host_fed) { return W > 1 && open_host != host_fed; }

// One launch, one n_iters, one set of hyper-parameters (`hyper_bytes` bytes each, compared as bytes) and one way of feeding: a call that
// differs from the open group in any of them starts a group of its own - the open one goes out first.
inline bool bf_lane_close_first(int W, int open_iters, int n_iters, const void *open_hyper, const void *hyper, size_t hyper_bytes,
                                bool open_host, bool host_fed) {
    return open_iters != n_iters || std::memcmp(open_hyper, hyper, hyper_bytes) != 0 || bf_lane_feed_differs(W, open_host, host_fed);
}

// What becomes of a group of `n_open` calls (W at most) right after a call has joined it.  Full: it is launched, behind the lane's running
// group.  Otherwise the idle rule - the group goes out if its lane is idle, which the caller finds out (IF_IDLE) - with two exceptions:
// `fill` (BF_FIT_LANE_FILL) turns the rule off, and with W > 1 the group is held while the feeder is fast (there was a call before this
// one, less than H before `now`) AND the group is young (its first call joined at t_first, less than H before `now`).  Both comparisons are
// strict: H = 0 never holds.
enum class BfLaneAfterJoin { LAUNCH, IF_IDLE, HOLD };
using BfLaneTime = std::chrono::steady_clock::time_point;
inline BfLaneAfterJoin bf_lane_after_join(int W, int n_open, bool fill, std::chrono::microseconds H, BfLaneTime now, bool called_before,
                                          BfLaneTime t_prev, BfLaneTime t_first) {
    if (n_open >= W) return BfLaneAfterJoin::LAUNCH;
    if (fill) return BfLaneAfterJoin::HOLD;
    const bool fast_feed = called_before && now - t_prev < H;
    return (W > 1 && fast_feed && now - t_first < H) ? BfLaneAfterJoin::HOLD : BfLaneAfterJoin::IF_IDLE;
}
