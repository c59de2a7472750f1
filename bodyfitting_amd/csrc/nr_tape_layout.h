// Where the buffers of one taped render lie inside ONE float32 allocation (bf_nr_render_dev: the tape borrows a tensor the caller
// allocated).  Plain C++, no HIP: the library (nr_api.hip, exported as bf_nr_tape_layout) and tests/test_nr_tape_layout.py compile
// this one function, so the caller's allocation and the library's pointers cannot disagree.  Sizes and offsets are in floats; every
// offset is a multiple of 64 floats (256 bytes); an absent segment has size 0 and the offset of whatever follows it.
#pragma once
#include <cstddef>

#define BF_NR_TAPE_REC_FLOATS 20          // = BF_TEX_REC (tex_bodies.h; nr_api.hip asserts it)
#define BF_NR_TAPE_VIEW_FLOATS 22         // = sizeof(TexView) / 4: R[9] t[3] K[9] orig
#define BF_NR_TAPE_ALIGN_FLOATS 64

enum BfNrTapeSegment {
    BF_NR_SEG_VIEW = 0,     // the packed TexView of the render                                   always
    BF_NR_SEG_PIX,          // pixel map [is][is][5]                                              always
    BF_NR_SEG_FREC,         // face records [nrec][BF_TEX_REC]                                    always
    BF_NR_SEG_LIGHT,        // light rows [nrec][3]                                               lit
    BF_NR_SEG_VERTS,        // the render's vertices [nv][3]                                      geometry
    BF_NR_SEG_PV,           // ... projected [nv][3]                                              geometry
    BF_NR_SEG_RGBMAP,       // super-sampled colours [is][is][3]                                  geometry, has_rgb
    BF_NR_SEG_UNLIT,        // unlit samples [is][is][3]                                          geometry, has_rgb, lit, directional
    BF_NR_SEG_COUNT
};

struct BfNrTapeLayout {
    size_t off[BF_NR_SEG_COUNT], size[BF_NR_SEG_COUNT], total;
};

// flags: BF_NR_TAPE_TEXTURES (1) | BF_NR_TAPE_GEOMETRY (2); flags 0: a render without a tape, which still needs the first four.
// -> false when an argument is out of range (is in [1, 8192], nrec >= 1, nv >= 0) - nothing else can overflow a 64-bit size_t:
// the largest segment is nrec * 20 < 2^36 floats.
inline bool bf_nr_tape_layout_of(int is, int nrec, int nv, bool lit, int flags, bool has_rgb, bool directional, BfNrTapeLayout *L) {
    if (!L || is < 1 || is > 8192 || nrec < 1 || nv < 0 || (flags & ~3)) return false;
    const size_t npx = (size_t)is * (size_t)is;
    const bool geo = (flags & 2) != 0;
    for (int k = 0; k < BF_NR_SEG_COUNT; ++k) L->size[k] = 0;
    L->size[BF_NR_SEG_VIEW] = BF_NR_TAPE_VIEW_FLOATS;
    L->size[BF_NR_SEG_PIX] = npx * 5;
    L->size[BF_NR_SEG_FREC] = (size_t)nrec * BF_NR_TAPE_REC_FLOATS;
    if (lit) L->size[BF_NR_SEG_LIGHT] = (size_t)nrec * 3;
    if (geo) {
        L->size[BF_NR_SEG_VERTS] = (size_t)nv * 3;
        L->size[BF_NR_SEG_PV] = (size_t)nv * 3;
        if (has_rgb) {
            L->size[BF_NR_SEG_RGBMAP] = npx * 3;
            if (lit && directional) L->size[BF_NR_SEG_UNLIT] = npx * 3;
        }
    }
    size_t at = 0;
    for (int k = 0; k < BF_NR_SEG_COUNT; ++k) {
        L->off[k] = at;
        at += (L->size[k] + BF_NR_TAPE_ALIGN_FLOATS - 1) / BF_NR_TAPE_ALIGN_FLOATS * BF_NR_TAPE_ALIGN_FLOATS;
    }
    L->total = at;
    return true;
}
