// Host-only check of the mesh pass's kernel choice (bodyfitting_amd/csrc/mesh_choice.h), built with the host compiler under
// -fsanitize=address,undefined by tests/test_mesh_choice.py.  For calls of `per` frames in groups of G, on the SMPL and SMPL-X
// pose-feature sizes, with and without a sub-model table and the 32-frame kernel: a group of calls below 16 frames is ONE launch of the
// multi-frame kernel over all G x per frames, a lone single-frame SMPL call keeps bf_mesh_kernel, and from 16 frames on every call keeps a
// pass of its own with the kernel it gets alone.  One "ok per G npf" line per case; any failure exits non-zero.
#include "mesh_choice.h"

#include <cstdio>

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

static const char *name(BfMeshKernel k) {
    switch (k) {
    case BfMeshKernel::PLAIN: return "plain";
    case BfMeshKernel::MULTI: return "multi";
    case BfMeshKernel::BATCH32: return "batch32";
    case BfMeshKernel::GEMM: return "gemm";
    }
    return "?";
}

// what a call of n frames gets alone, written out from the rules of bf_launch_mesh's comment rather than through the function under test
static BfMeshKernel alone(int n, int npf, bool tab, unsigned flags) {
    if (n >= 16 && !tab) {
        const bool b32 = n <= 64 && !(flags & BF_MESH_CHOICE_VPOSED) && (flags & BF_MESH_CHOICE_BATCH32_FITS);
        return b32 ? BfMeshKernel::BATCH32 : BfMeshKernel::GEMM;
    }
    return (n >= 2 || npf > 208) ? BfMeshKernel::MULTI : BfMeshKernel::PLAIN;
}

static bool one(int per, int G, int npf) {
    const int n = per * G;
    for (int tab = 0; tab < 2; ++tab)
        for (unsigned flags = 0; flags < 4; ++flags) {
            // the group as the fit lanes pass it (per = F, n = G F), and a lone call both ways it can be written (per = n, per = 0)
            const BfMeshChoice ch = bf_mesh_choice(per, n, npf, tab != 0, flags);
            CHECK(ch.passes >= 1 && ch.frames >= 1 && ch.passes * ch.frames == n, "per %d G %d npf %d tab %d flags %u: %d passes of %d frames do not cover %d",
                  per, G, npf, tab, flags, ch.passes, ch.frames, n);
            if (G == 1) {
                const BfMeshChoice c0 = bf_mesh_choice(0, n, npf, tab != 0, flags);
                CHECK(c0.kernel == ch.kernel && c0.passes == ch.passes && c0.frames == ch.frames, "per %d npf %d: per = n and per = 0 differ", per, npf);
                CHECK(ch.passes == 1 && ch.kernel == alone(n, npf, tab != 0, flags), "per %d G 1 npf %d tab %d flags %u: %s x %d", per, npf, tab, flags,
                      name(ch.kernel), ch.passes);
                if (per == 1 && npf <= 208) CHECK(ch.kernel == BfMeshKernel::PLAIN, "a lone single-frame call keeps bf_mesh_kernel, got %s", name(ch.kernel));
            } else if (per < 16) {
                CHECK(ch.kernel == BfMeshKernel::MULTI && ch.passes == 1 && ch.frames == n, "per %d G %d npf %d tab %d flags %u: one multi launch expected, got %s x %d",
                      per, G, npf, tab, flags, name(ch.kernel), ch.passes);
            } else {
                CHECK(ch.passes == G && ch.frames == per && ch.kernel == alone(per, npf, tab != 0, flags),
                      "per %d G %d npf %d tab %d flags %u: a pass per call with the call's own kernel expected, got %s x %d of %d", per, G, npf, tab, flags,
                      name(ch.kernel), ch.passes, ch.frames);
                if (!tab) CHECK(ch.kernel == BfMeshKernel::BATCH32 || ch.kernel == BfMeshKernel::GEMM, "per %d: a matrix-core kernel expected", per);
            }
        }
    return true;
}

static bool singles() {
    CHECK(!bf_mesh_choice_multi(207, 1) && !bf_mesh_choice_multi(208, 1) && bf_mesh_choice_multi(209, 1) && bf_mesh_choice_multi(486, 1) && bf_mesh_choice_multi(207, 2),
          "the single-frame kernel by pose-feature size");
    return true;
}

int main() {
    const int pers[] = {1, 2, 4, 15, 16, 32}, groups[] = {1, 2, 8, 9, 32}, npfs[] = {207, 486};          // 9 x 23 (SMPL), 9 x 54 (SMPL-X)
    bool all = true;
    for (int npf : npfs)
        for (int per : pers)
            for (int G : groups) {
                const bool ok = one(per, G, npf);
                if (ok) std::printf("ok %d %d %d\n", per, G, npf);
                all = all && ok;
            }
    all = all && singles();
    return all ? 0 : 1;
}
