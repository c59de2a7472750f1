// Device helpers shared by the OpenPose body (openpose_kernels.hip) and hand (openpose_hand_kernels.hip) kernels: OpenCV's
// INTER_CUBIC coefficients and source taps, and the Gaussian filter's border rule.  Both files compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

// scipy.ndimage mode 'reflect' (d c b a | a b c d | d c b a), one reflection: index i of a line of n
__device__ __forceinline__ int op_reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// interpolateCubic(x, coeffs), A = -0.75, in float
__device__ __forceinline__ void op_cubic(float x, float c[4]) {
    const float A = -0.75f;
    const float x1 = x + 1.f;
    c[0] = ((A * x1 - 5.f * A) * x1 + 8.f * A) * x1 - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    const float y = 1.f - x;
    c[2] = ((A + 2.f) * y - (A + 3.f)) * y * y + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// one destination index of a cubic resize: the source coordinate (float)((d + 0.5) * scale - 0.5), floored; taps s - 1 .. s + 2
// clamped to the source (OpenCV replicates the border); coefficients of the fraction
__device__ __forceinline__ void op_axis(int d, double scale, int n, int idx[4], float c[4]) {
    float f = (float)((d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    op_cubic(f, c);
    for (int j = 0; j < 4; ++j) idx[j] = min(max(s - 1 + j, 0), n - 1);
}
