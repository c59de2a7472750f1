// The fit lanes of a batch (lanes.hip) as the rest of the host code sees them: every use of bf_batch::lanes outside lanes.hip goes through
// these functions.  The protocol is described at the top of lanes.hip, the decisions that shape a bracket are lane_policy.h.
#pragma once
#include "bf_host.h"

// at batch creation: lane count, width and the lane arenas' layout from the device's CU count (n_cus <= 0: unknown), the batch's frames
// and views, BF_FIT_LANES / BF_FIT_LANE_WIDTH and the staging mode.  The lanes themselves are created on first use.
void bf_lanes_configure(bf_batch *b, int n_cus);
// frame-after-frame fits of this batch go to lanes (fit_plan's LANE route, bf_batch_stage_inputs)
inline bool bf_lanes_enabled(const bf_batch *b) { return b->lanes.n > 1; }
// new cameras: the group launches' copy of the projection table is refreshed when the lanes next take over
inline void bf_lanes_cameras_changed(bf_batch *b) { b->lanes.proj_rep_stale = true; }
// a lane holds the newest fit (the last call took the LANE route; any other entry point drains first)
inline bool bf_lanes_hold_last(const bf_batch *b) { return b->lanes.last >= 0; }

// bf_batch_stage_inputs on a batch with lanes: the call's inputs into the next slot of the next lane's open group
int bf_lanes_stage(bf_batch *b, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose);
// the LANE route of bf_fit: the call joins the next lane's open group, which is launched when the rules say so.  The call's fit number
// (bf_batch::fit_seq) is its place in its group; the caller counts it.
int bf_lanes_fit(bf_batch *b, int n_iters, const HyperDev &hd);
// (declared in bf_host.h) int bf_lanes_drain(bf_batch *b);

// Where fit number `seq` is while a lane holds it: the lane's arena - wait for its ev_copied, then read the pinned mirror - and the float
// offsets of that call's params, terms, state, joints and vertices in it.  A call still in an open group is launched first.
// arena = nullptr: no lane holds that fit.
struct BfLaneResult { const ResultArena *arena = nullptr; size_t off[5] = {0, 0, 0, 0, 0}; };
int bf_lanes_find(bf_batch *b, long long seq, BfLaneResult &at);

// bf_batch_destroy: the open groups go out (calls that joined one were promised a fit), the lanes' work is waited for, everything is freed
void bf_lanes_destroy(bf_batch *b);
// (bf_batch_lane_stats and bf_batch_lane_feed_stats of include/bodyfit.h are defined in lanes.hip)
