// The fit-check overlay (reference smplify/body_fitting.py:34-42 check_smpl_fitting): every vertex of the fitted body projected into
// every selected view by cv2.projectPoints and stamped as cv2.circle(r=1, thickness=-1) draws it.  Host side: overlay_api.hip; the
// Rodrigues round trip and the numpy restatement: bodyfitting_amd/overlay.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "overlay_kernels.h"

#define OV_THREADS 256

// per view, doubles: R'[9] (row-major, the rotation cv2.projectPoints rebuilds from rvec), t[3], K[9]
#define OV_CAM 21

__device__ __forceinline__ void ov_put(uint8_t *img, int W, int x, int y) {
    uint8_t *p = img + ((long long)y * W + x) * 3;
    p[0] = 0;                                     // the colour (0, 255, 0): every stamp writes the same bytes
    p[1] = 255;
    p[2] = 0;
}

// one thread per (vertex, view).  images: n views of H * W * 3 bytes; verts: [nv][3] float32 (the reference's verts.astype(float32))
extern "C" __global__ __launch_bounds__(OV_THREADS) void bf_overlay_stamp_kernel(int nv, int H, int W, const float *__restrict__ verts,
                                                                                  const double *__restrict__ cams, uint8_t *images) {
    const int i = blockIdx.x * OV_THREADS + threadIdx.x;
    if (i >= nv) return;
    const double *c = cams + (long long)blockIdx.y * OV_CAM;
    const double *R = c, *t = c + 9, *K = c + 12;
    const double X = verts[i * 3], Y = verts[i * 3 + 1], Z = verts[i * 3 + 2];
    // cvProjectPoints2Internal in its order with the distortion k[0..13] = 0.  Its zero terms (cdist = 1 + 0 * r2 ..., the identity
    // tilt) are exact identities while r2 = x * x + y * y is finite; past that (|x| or |y| > 1e154) OpenCV's NaN and the float32
    // overflow here both fail the bounds test for any focal length above 1e-115.
    double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    z = z != 0.0 ? 1. / z : 1;
    x *= z;
    y *= z;
    // m = xd * fx + cx with fx = K[0][0], cx = K[0][2], fy = K[1][1], cy = K[1][2]; the double result goes out as float32 (the dtype of
    // the float32 object points)
    const float px = (float)(x * K[0] + K[2]);
    const float py = (float)(y * K[4] + K[5]);
    // 0 <= p < W on the float32 values, then int() truncates
    if (!(px >= 0.0f && px < (float)W && py >= 0.0f && py < (float)H)) return;
    const int cx = (int)px, cy = (int)py;
    // OpenCV's Circle(radius 1, fill): the row cy from cx - 1 to cx + 1 clipped to the image, and (cx, cy - 1), (cx, cy + 1) when in it
    uint8_t *img = images + (long long)blockIdx.y * H * W * 3;
    ov_put(img, W, cx, cy);
    if (cx > 0) ov_put(img, W, cx - 1, cy);
    if (cx + 1 < W) ov_put(img, W, cx + 1, cy);
    if (cy > 0) ov_put(img, W, cx, cy - 1);
    if (cy + 1 < H) ov_put(img, W, cx, cy + 1);
}
