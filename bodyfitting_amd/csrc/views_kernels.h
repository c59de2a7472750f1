// What views_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct VwJob {
    long long img_off;            // the crop's first image byte in the row buffer; rows W * 3 bytes apart
    long long msk_off;            // the crop's first mask byte in the mask buffer; rows W bytes apart
    int ch, cw, mask_slot;        // mask_slot >= 0: the resized mask goes to out_masks[mask_slot]
};

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_views_bbox_init_kernel(int n, int *bbox);
extern "C" __global__ void bf_views_bbox_kernel(int H, int W, long long stride, const uint8_t *masks, int *bbox);
extern "C" __global__ void bf_views_prepare_kernel(int L, int W, const VwJob *jobs, const uint8_t *crops, const uint8_t *masks, uint8_t *out_images,
                                                   uint8_t *out_masks, unsigned long long *sums);
#pragma GCC visibility pop
