// One axis of cv2.resize INTER_LINEAR on 8-bit data, shared by the HMR resize (hmr_kernels.hip) and the GeneBody view preparation
// (views_kernels.hip): `scale` is OpenCV's 1 / (n_dst / n_src) in double, formed by the caller; the source coordinate
// (d + 0.5) * scale - 0.5 rounded to float and floored, 11-bit coefficients.  Columns clamp coordinate and weight at the borders
// (clamp_weight), rows only the index.  Compiled under the including file's -ffp-contract setting, which is meant.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void bf_resize_axis(int d, double scale, int n_src, int clamp_weight, int *s0, int *s1, int *a0, int *a1) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp_weight) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    }
    *a0 = (int)rintf((1.f - f) * 2048.f);
    *a1 = (int)rintf(f * 2048.f);
    *s0 = min(max(s, 0), n_src - 1);
    *s1 = min(max(s + 1, 0), n_src - 1);
}
