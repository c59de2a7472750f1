// The per-crop descriptor the OpenPose hand kernels (openpose_hand_kernels.hip) and their host side (openpose_hand_api.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define OH_NMAP 22                   // handpose_model's maps; the last (background) is averaged but never picked
#define OH_NPART 21

// one crop at one scale.  The crop is img[y:y+bh, x:x+bw] of view `view` (the reference's oriImg, a numpy view: resizes replicate
// the crop's own edges); rh x rw is its resized size, Hp x Wp the padded network input every crop of one launch shares.
struct OhBox {
    int view, x, y, bw, bh;
    int rh, rw, Hp, Wp, pad_;
    double inv;                      // 1 / scale: the uint8 resize's source step
    double sy2, sx2;                 // 1 / (bh / rh), 1 / (bw / rw): the source steps of the resize back to bh x bw
    long long px;                    // this crop's first pixel in the per-crop maps laid end to end (the sum of earlier bh * bw)
};

// the kernels of openpose_hand_kernels.hip, declared once for the definitions and the host file that launches them
#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_oh_input_kernel(int n, int Hp, int Wp, int H, int W, const OhBox *boxes, const uint8_t *views, float4 *out);
extern "C" __global__ void bf_oh_up8_kernel(int hq, int wq, long long up_stride, const OhBox *boxes, const float *out, float *up);
extern "C" __global__ void bf_oh_maps_kernel(long long up_stride, const OhBox *boxes, const float *up, double *heat);
extern "C" __global__ void bf_oh_gauss_kernel(int axis, int src_c, const OhBox *boxes, const double *src, double *dst);
extern "C" __global__ void bf_oh_pick_kernel(const OhBox *boxes, long long px0, const double *bl, const double *heat, int *iscr, double *dscr, int *peaks,
                                             double *scores, int *found);
extern "C" __global__ void bf_oh_label_kernel(int H, int W, const uint8_t *binary, int *iscr, int *labels, int *counts);
#pragma GCC visibility pop
