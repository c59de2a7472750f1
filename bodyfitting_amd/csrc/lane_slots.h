// Slot arithmetic and packing of a fit lane's input arena - plain C++, no HIP: lanes.hip includes it for the device arena and its pinned
// mirror, tests/lane_pack_main.cpp for a host-only check under the sanitizers.
//
// An arena holds the frames of up to W calls, array-major like FrameIO: [W F] keypoints | [W F] params0 | [W F] ndiv, every array on a
// 256-byte slice.  Slot s - call s of the group - owns one contiguous range in each of the three arrays, so any prefix of slots is three
// contiguous ranges.  The pinned mirror of an arena has the same layout: slot s of the one mirrors slot s of the other array by array.
// W = 1 is the batch's own packed layout (bf_batch::in_off / in_total).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

struct BfLaneLayout {
    size_t off[3] = {0, 0, 0};      // float offsets of the keypoint, params0 and ndiv arrays
    size_t cnt[3] = {0, 0, 0};      // floats of ONE slot in each array: F V L 3, F np, F (ndiv: int32, one per float)
    size_t total = 0;               // floats of the arena
    int W = 0;
};
struct BfRange { size_t off = 0, n = 0; };        // floats

inline size_t bf_up64(size_t n) { return (n + 63) & ~(size_t)63; }          // 256-byte slices

// the arena of W calls of F frames: n_kp floats of keypoints per call (F V L 3), np parameters per frame
inline BfLaneLayout bf_lane_layout(int W, int F, size_t n_kp, int np) {
    BfLaneLayout L;
    L.W = W;
    L.cnt[0] = n_kp; L.cnt[1] = (size_t)F * np; L.cnt[2] = (size_t)F;
    L.off[0] = 0;
    L.off[1] = bf_up64((size_t)W * L.cnt[0]);
    L.off[2] = L.off[1] + bf_up64((size_t)W * L.cnt[1]);
    L.total = L.off[2] + bf_up64((size_t)W * L.cnt[2]);
    return L;
}

// where slot `slot` keeps array k (0 keypoints, 1 params0, 2 ndiv)
inline size_t bf_slot_off(const BfLaneLayout &L, int k, int slot) { return L.off[k] + (size_t)slot * L.cnt[k]; }

// the three ranges that hold slots [0, n_slots): what one transfer moves for a group of G calls and a slot staged past them (n = G + 1)
inline void bf_slot_prefix(const BfLaneLayout &L, int n_slots, BfRange out[3]) {
    for (int k = 0; k < 3; ++k) { out[k].off = L.off[k]; out[k].n = (size_t)n_slots * L.cnt[k]; }
}

// where the packed optimiser vector keeps what an initial estimate sets (FitTab's offsets)
struct BfInitMap { int np = 0, nb = 0, nbp = 0, off_pose = 0, off_beta = 0, off_orient = 0; };

// net_output of smplify.py:103 -> the packed optimiser vector: transl = 0, scale = 1 (:126-128), body pose, betas, root orientation
inline void bf_pack_init(const BfInitMap &m, int F, const float *init_betas, const float *init_pose, float *dst) {
    const int pose_stride = 72;                  // net_output poses are [F,72] for both model kinds (smplify.py:108-112)
    std::memset(dst, 0, (size_t)F * m.np * sizeof(float));
    for (int f = 0; f < F; ++f) {
        float *q = dst + (size_t)f * m.np;
        q[3] = 1.0f;                                                             // body_scale = 1, transl = 0
        std::memcpy(q + m.off_pose, init_pose + (size_t)f * pose_stride + 3, sizeof(float) * m.nbp);
        std::memcpy(q + m.off_beta, init_betas + (size_t)f * m.nb, sizeof(float) * m.nb);
        std::memcpy(q + m.off_orient, init_pose + (size_t)f * pose_stride, sizeof(float) * 3);
    }
}

// the views each frame's keypoint loss divides by: the caller's, or all V
inline void bf_fill_ndiv(int32_t *dst, int F, const int32_t *n_use_frames, int V) {
    for (int f = 0; f < F; ++f) dst[f] = n_use_frames ? n_use_frames[f] : V;
}

// one call's keypoints, packed initial estimate and view counts into slot `slot` of the arena at `base` - exactly that slot's three ranges
inline void bf_pack_slot(const BfLaneLayout &L, float *base, int slot, const BfInitMap &m, int F, int V, const float *keypoints,
                         const int32_t *n_use_frames, const float *init_betas, const float *init_pose) {
    std::memcpy(base + bf_slot_off(L, 0, slot), keypoints, L.cnt[0] * sizeof(float));
    bf_pack_init(m, F, init_betas, init_pose, base + bf_slot_off(L, 1, slot));
    bf_fill_ndiv((int32_t *)(base + bf_slot_off(L, 2, slot)), F, n_use_frames, V);
}

// slot `from` of the arena at `src` copied into slot `to` of the arena at `dst` (both of layout L; not the same slot of the same arena)
inline void bf_copy_slot(const BfLaneLayout &L, float *dst, int to, const float *src, int from) {
    for (int k = 0; k < 3; ++k) std::memcpy(dst + bf_slot_off(L, k, to), src + bf_slot_off(L, k, from), L.cnt[k] * sizeof(float));
}
