// Which kernel a forward mesh pass takes and in how many launches - plain C++, no HIP: api.hip (bf_launch_mesh) includes it and issues
// what it says, tests/mesh_choice_main.cpp checks it on the host alone under the sanitizers.
//
// A pass is `n` frames; with 0 < per < n they are the frames of n / per independent calls of `per` frames each (a fit-lane group, MeshPass::per)
// and every frame must get the bits it would get in a pass of its call alone.  bf_mesh_kernel (one frame per workgroup) and every instance of
// bf_mesh_multi_kernel (up to eight frames per workgroup, the tile's posedirs slice streamed ONCE for them) do the same arithmetic in the
// same order per frame, so a group of calls below the matrix-core threshold is ONE multi-frame launch over all n frames - the call
// boundaries need not fall on the kernel's 8-frame blocks.  The matrix-core kernels produce other bits: a group of calls of 16 frames or
// more keeps a pass per call, each the kernel that call would get alone.
#pragma once

enum class BfMeshKernel {
    PLAIN,          // bf_mesh_kernel, grid (tiles, frames)
    MULTI,          // bf_mesh_multi_kernel, grid (tiles, ceil(frames / frames per workgroup))
    BATCH32,        // bf_mesh_batch32_kernel: pose blend on the matrix cores with the epilogue behind the accumulators
    GEMM,           // the pose-blend GEMM and the per-frame epilogue kernel behind it
};

struct BfMeshChoice {
    BfMeshKernel kernel;
    int passes;     // passes of `frames` frames each, one after the other through the state / vertex / extra-joint arrays
    int frames;
};

constexpr int kBfMeshMfmaMinFrames = 16;        // = BF_MFMA_MIN_FRAMES (bf_internal.h; api.hip holds the two together)
constexpr int kBfMeshBatch32MaxFrames = 64;     // = BF_BATCH32_MAX_FRAMES
constexpr int kBfMeshPlainRows = 208;           // pose-feature rows bf_mesh_kernel keeps in flight (BF_MESH_PF x BF_MESH_RG; bf_mesh_use_multi)

enum : unsigned {
    BF_MESH_CHOICE_VPOSED = 1u,                 // the posed-but-unskinned vertices are asked for (the 32-frame kernel does not write them)
    BF_MESH_CHOICE_BATCH32_FITS = 2u,           // bf_mesh_batch32_fits: the model's tables fit the 32-frame kernel
};

// the multi-frame kernel for 2..15 frames, and for one frame of a model with more pose-feature rows than bf_mesh_kernel holds
inline bool bf_mesh_choice_multi(int npf, int n) { return n >= 2 || npf > kBfMeshPlainRows; }

// `tab`: the pass runs on a sampled sub-model's table (the matrix-core kernels know the model's own table only)
inline BfMeshChoice bf_mesh_choice(int per, int n, int npf, bool tab, unsigned flags) {
    const bool group = per > 0 && per < n;
    const int n_sel = group ? per : n;
    if (group && n_sel < kBfMeshMfmaMinFrames) return {BfMeshKernel::MULTI, 1, n};
    const int passes = group ? n / per : 1;
    if (n_sel >= kBfMeshMfmaMinFrames && !tab) {
        const bool b32 = n_sel <= kBfMeshBatch32MaxFrames && !(flags & BF_MESH_CHOICE_VPOSED) && (flags & BF_MESH_CHOICE_BATCH32_FITS);
        return {b32 ? BfMeshKernel::BATCH32 : BfMeshKernel::GEMM, passes, n_sel};
    }
    return {bf_mesh_choice_multi(npf, n_sel) ? BfMeshKernel::MULTI : BfMeshKernel::PLAIN, passes, n_sel};
}
