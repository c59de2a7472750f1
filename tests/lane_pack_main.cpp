// Host-only check of a fit lane's slot arithmetic and packing (bodyfitting_amd/csrc/lane_slots.h), built with the host compiler under
// -fsanitize=address,undefined by tests/test_lane_pack.py.  For every (F, V, W, np) it fills each slot of an exactly-sized arena and
// holds the slot against what the single-call packing (the batch's own [keypoints | params0 | ndiv] buffer) produces for the same
// inputs, checks that nothing outside the slot's three ranges was written, and that the ranges one transfer moves for a group of G
// calls and a slot staged past them are exactly slots [0, G + staged).  One "ok F V W np" line per case; any failure exits non-zero.
#include "lane_slots.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static const int kLandmarks = 25;                       // keypoints per view in the fit's loss
static const uint32_t kCanary = 0x7fc0beefu;            // a NaN payload no packing produces

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float canary() { float x; std::memcpy(&x, &kCanary, 4); return x; }

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static float rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((rng_state >> 40) & 0xffff) / 65536.0f - 0.5f;
}

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

// the packing of one call as the batch's own input arena has always had it: [keypoints | params0 | ndiv] on 256-byte slices
struct Single { std::vector<float> buf; size_t off[3]; };
static Single pack_single(const BfInitMap &m, int F, int V, size_t n_kp, const float *kp, const int32_t *n_use, const float *betas, const float *pose) {
    Single s;
    s.off[0] = 0; s.off[1] = bf_up64(n_kp); s.off[2] = s.off[1] + bf_up64((size_t)F * m.np);
    s.buf.assign(s.off[2] + bf_up64((size_t)F), 0.f);
    std::memcpy(s.buf.data() + s.off[0], kp, n_kp * sizeof(float));
    float *dst = s.buf.data() + s.off[1];
    std::memset(dst, 0, (size_t)F * m.np * sizeof(float));
    for (int f = 0; f < F; ++f) {
        float *q = dst + (size_t)f * m.np;
        q[3] = 1.0f;
        std::memcpy(q + m.off_pose, pose + (size_t)f * 72 + 3, sizeof(float) * m.nbp);
        std::memcpy(q + m.off_beta, betas + (size_t)f * m.nb, sizeof(float) * m.nb);
        std::memcpy(q + m.off_orient, pose + (size_t)f * 72, sizeof(float) * 3);
    }
    int *nd = (int *)(s.buf.data() + s.off[2]);
    for (int f = 0; f < F; ++f) nd[f] = n_use ? n_use[f] : V;
    return s;
}

// every float of the arena outside slot `slot`'s three ranges still is the canary; the ranges equal the single-call packing
static bool slot_alone_written(const BfLaneLayout &L, const float *arena, int slot, const Single &want) {
    std::vector<char> mine(L.total, 0);
    for (int k = 0; k < 3; ++k) {
        const size_t at = bf_slot_off(L, k, slot);
        CHECK(at + L.cnt[k] <= L.total, "slot %d array %d leaves the arena", slot, k);
        CHECK(std::memcmp(arena + at, want.buf.data() + want.off[k], L.cnt[k] * sizeof(float)) == 0, "slot %d array %d differs from the single-call packing", slot, k);
        for (size_t i = 0; i < L.cnt[k]; ++i) mine[at + i] = 1;
    }
    for (size_t i = 0; i < L.total; ++i)
        if (!mine[i]) CHECK(bits(arena[i]) == kCanary, "float %zu outside slot %d was written", i, slot);
    return true;
}

static bool one_case(int F, int V, int W, int np) {
    BfInitMap m;
    m.np = np; m.nb = np - 76; m.nbp = 69; m.off_pose = 4; m.off_beta = 73; m.off_orient = 73 + m.nb;      // transl 3 | scale | pose 69 | betas | orient 3
    const size_t n_kp = (size_t)F * V * kLandmarks * 3;
    const BfLaneLayout L = bf_lane_layout(W, F, n_kp, np);
    CHECK(L.W == W && L.cnt[0] == n_kp && L.cnt[1] == (size_t)F * np && L.cnt[2] == (size_t)F, "slot sizes");
    for (int k = 0; k < 3; ++k) CHECK(L.off[k] % 64 == 0, "array %d is not on a 256-byte slice", k);
    CHECK(L.off[1] >= (size_t)W * L.cnt[0] && L.off[2] >= L.off[1] + (size_t)W * L.cnt[1] && L.total >= L.off[2] + (size_t)W * L.cnt[2], "arrays overlap");
    if (W == 1) {           // the batch's own layout
        CHECK(L.off[1] == bf_up64(n_kp) && L.off[2] == L.off[1] + bf_up64((size_t)F * np) && L.total == L.off[2] + bf_up64((size_t)F), "W = 1 is not the single-call layout");
    }
    std::vector<float> kp(n_kp), betas((size_t)F * m.nb), pose((size_t)F * 72);
    std::vector<int32_t> n_use(F);
    std::unique_ptr<float[]> arena(new float[L.total]), other(new float[L.total]);       // exactly sized: a write past the end is the sanitizer's
    for (int slot = 0; slot < W; ++slot) {
        for (int with_counts = 0; with_counts < 2; ++with_counts) {
            for (auto &x : kp) x = rnd() * 512.f;
            for (auto &x : betas) x = rnd();
            for (auto &x : pose) x = rnd();
            for (int f = 0; f < F; ++f) n_use[f] = 1 + (f + slot) % V;
            const int32_t *counts = with_counts ? n_use.data() : nullptr;
            for (size_t i = 0; i < L.total; ++i) arena[i] = other[i] = canary();
            bf_pack_slot(L, arena.get(), slot, m, F, V, kp.data(), counts, betas.data(), pose.data());
            const Single want = pack_single(m, F, V, n_kp, kp.data(), counts, betas.data(), pose.data());
            if (!slot_alone_written(L, arena.get(), slot, want)) return false;
            // a second packing into the same slot (two stagings before one fit) replaces the first entirely
            for (auto &x : kp) x = rnd() * 512.f;
            for (auto &x : pose) x = rnd();
            bf_pack_slot(L, arena.get(), slot, m, F, V, kp.data(), counts, betas.data(), pose.data());
            const Single again = pack_single(m, F, V, n_kp, kp.data(), counts, betas.data(), pose.data());
            if (!slot_alone_written(L, arena.get(), slot, again)) return false;
            // a re-fit's host copy: this slot into every slot of another arena writes that slot alone, and leaves the source as it was
            for (int to = 0; to < W; ++to) {
                for (size_t i = 0; i < L.total; ++i) other[i] = canary();
                bf_copy_slot(L, other.get(), to, arena.get(), slot);
                if (!slot_alone_written(L, other.get(), to, again)) return false;
            }
            if (!slot_alone_written(L, arena.get(), slot, again)) return false;
        }
    }
    // the one transfer of a launched group: G joined calls and possibly a slot staged past them -> exactly slots [0, G + staged)
    for (int G = 0; G <= W; ++G)
        for (int staged = 0; staged < 2; ++staged) {
            const int n = G + staged;
            if (n < 1 || n > W) continue;
            BfRange rg[3];
            bf_slot_prefix(L, n, rg);
            std::vector<char> moved(L.total, 0), wanted(L.total, 0);
            for (int k = 0; k < 3; ++k) {
                CHECK(rg[k].off + rg[k].n <= L.total, "G %d staged %d: range %d leaves the arena", G, staged, k);
                for (size_t i = 0; i < rg[k].n; ++i) { CHECK(!moved[rg[k].off + i], "ranges overlap"); moved[rg[k].off + i] = 1; }
            }
            for (int s = 0; s < n; ++s)
                for (int k = 0; k < 3; ++k)
                    for (size_t i = 0; i < L.cnt[k]; ++i) wanted[bf_slot_off(L, k, s) + i] = 1;
            CHECK(moved == wanted, "G %d staged %d: the transfer's ranges are not slots [0, %d)", G, staged, n);
        }
    return true;
}

int main() {
    // 87: the kid model's odd stride; V = 5: 375 keypoint floats per frame, no 16-byte multiple; F = 16: the batch that takes the GEMM mesh
    const int Fs[] = {1, 4, 16}, Vs[] = {1, 5, 12, 50}, Ws[] = {1, 3, 8}, nps[] = {86, 87};
    int bad = 0;
    for (int F : Fs) for (int V : Vs) for (int W : Ws) for (int np : nps) {
        if (one_case(F, V, W, np)) std::printf("ok %d %d %d %d\n", F, V, W, np);
        else { std::printf("bad %d %d %d %d\n", F, V, W, np); ++bad; }
    }
    return bad ? 1 : 0;
}
