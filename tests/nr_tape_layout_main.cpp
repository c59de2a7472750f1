// tests/test_nr_tape_layout.py: bodyfitting_amd/csrc/nr_tape_layout.h swept on the host alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer.  is 1 .. 8192 (every value), nrec from 1 to 2^31 - 1, nv from 0 to 2^28, every flag combination, lit,
// has_rgb and directional on and off.  Sizes are checked against what nr_api.hip's host route allocates for the same render
// (NrFrame::alloc, nr_keep_geometry's blocks): npx * 5, nrec * 20, nrec * 3, nv * 3 twice, npx * 3 twice.
#include "nr_tape_layout.h"

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
    const int nrecs[] = {1, 2, 3, 63, 64, 65, 13776, 163840, (1 << 24) + 1, INT_MAX / 6, INT_MAX - 1, INT_MAX};
    const int nvs[] = {0, 1, 21, 22, 6890, 1 << 28};
    long long layouts = 0;
    for (int is = 1; is <= 8192; ++is)
        for (int nrec : nrecs) {
            // (the full product at the sizes' edges, a thinner one in between: 8192 x 12 x 6 x 32 layouts are more than a test needs)
            const bool edge = is <= 70 || is >= 8190 || (is & (is - 1)) == 0 || is % 509 == 0;
            for (int nv : nvs) {
                if (!edge && nv != 6890) continue;
                for (int bits = 0; bits < 32; ++bits) {
                    const int flags = bits & 3;
                    const bool lit = bits & 4, has_rgb = bits & 8, directional = bits & 16;
                    BfNrTapeLayout L;
                    CHECK(bf_nr_tape_layout_of(is, nrec, nv, lit, flags, has_rgb, directional, &L), "is %d nrec %d nv %d bits %d", is, nrec, nv, bits);
                    ++layouts;
                    const unsigned __int128 npx = (unsigned __int128)is * is;
                    const bool geo = flags & 2;
                    const unsigned __int128 want[BF_NR_SEG_COUNT] = {
                        22, npx * 5, (unsigned __int128)nrec * 20, lit ? (unsigned __int128)nrec * 3 : 0, geo ? (unsigned __int128)nv * 3 : 0,
                        geo ? (unsigned __int128)nv * 3 : 0, geo && has_rgb ? npx * 3 : 0, geo && has_rgb && lit && directional ? npx * 3 : 0};
                    unsigned __int128 total = 0;
                    for (int k = 0; k < BF_NR_SEG_COUNT; ++k) {
                        CHECK((unsigned __int128)L.size[k] == want[k], "segment %d of is %d nrec %d nv %d bits %d: %zu", k, is, nrec, nv, bits, L.size[k]);
                        CHECK(L.off[k] % 64 == 0 && (L.off[k] * sizeof(float)) % 256 == 0, "offset %d of is %d nrec %d: %zu", k, is, nrec, L.off[k]);
                        CHECK((unsigned __int128)L.off[k] == total, "segment %d of is %d nrec %d nv %d bits %d starts at %zu", k, is, nrec, nv, bits, L.off[k]);
                        for (int j = 0; j < k; ++j)                       // no two present segments overlap
                            CHECK(!L.size[j] || !L.size[k] || L.off[j] + L.size[j] <= L.off[k], "segments %d and %d overlap (is %d nrec %d)", j, k, is, nrec);
                        total += (want[k] + 63) / 64 * 64;
                    }
                    CHECK((unsigned __int128)L.total == total, "total of is %d nrec %d nv %d bits %d: %zu", is, nrec, nv, bits, L.total);
                    CHECK(total * sizeof(float) <= (unsigned __int128)SIZE_MAX, "bytes overflow size_t (is %d nrec %d)", is, nrec);
                    CHECK(L.off[BF_NR_SEG_COUNT - 1] + L.size[BF_NR_SEG_COUNT - 1] <= L.total, "the last segment ends behind the total");
                }
            }
        }
    std::printf("%s sweep (%lld layouts)\n", failures ? "FAILED" : "ok", layouts);
    // refusals: out of range, and nothing written through a null pointer
    BfNrTapeLayout L;
    const bool refused = !bf_nr_tape_layout_of(0, 1, 1, false, 0, false, false, &L) && !bf_nr_tape_layout_of(8193, 1, 1, false, 0, false, false, &L) &&
                         !bf_nr_tape_layout_of(16, 0, 1, false, 0, false, false, &L) && !bf_nr_tape_layout_of(16, 1, -1, false, 0, false, false, &L) &&
                         !bf_nr_tape_layout_of(16, 1, 1, false, 4, false, false, &L) && !bf_nr_tape_layout_of(16, 1, 1, false, 0, false, false, nullptr);
    std::printf("%s refusals\n", refused ? "ok" : "FAILED");
    return failures || !refused ? 1 : 0;
}
