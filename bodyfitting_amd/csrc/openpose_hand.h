// The per-crop descriptor the OpenPose hand kernels (openpose_hand_kernels.hip) and their host side (openpose_hand_api.hip) share.
#pragma once

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
