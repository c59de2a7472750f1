// Host side of the fit-check overlay (reference smplify/body_fitting.py:34-42): the views go up once, every vertex of every view is
// stamped in one launch, the views come back.  Kernel: overlay_kernels.hip; cameras: bodyfitting_amd/overlay.py.
#include "bf_host.h"
#include "overlay_kernels.h"

#define OV_CAM 21

extern "C" {

int bf_overlay_stamp(int device, int n, int H, int W, const uint8_t *const *images, int nv, const float *verts, const double *cams,
                     uint8_t *out) {
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (long long)H * W > (1LL << 28) || nv < 0 || !images || (nv > 0 && !verts) || !cams ||
        !out)
        return fail(BF_ERR_INVALID, "bf_overlay_stamp: bad argument (1 <= n <= 65535 views of H * W <= 2^28 pixels)");
    for (int i = 0; i < n; ++i)
        if (!images[i]) return fail(BF_ERR_INVALID, "bf_overlay_stamp: view " + std::to_string(i) + " has no image");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_overlay_stamp: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const size_t view = (size_t)H * W * 3;
    DevBuf<uint8_t> img;
    DevBuf<float> v;
    DevBuf<double> c;
    HIP_TRY(img.alloc(view * n));
    HIP_TRY(v.alloc((size_t)nv * 3));
    HIP_TRY(c.alloc((size_t)n * OV_CAM));
    for (int i = 0; i < n; ++i) HIP_TRY(hipMemcpy(img.p + i * view, images[i], view, hipMemcpyHostToDevice));
    if (nv > 0) HIP_TRY(hipMemcpy(v.p, verts, (size_t)nv * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c.p, cams, (size_t)n * OV_CAM * sizeof(double), hipMemcpyHostToDevice));
    if (nv > 0) {
        hipLaunchKernelGGL(bf_overlay_stamp_kernel, dim3((unsigned)((nv + 255) / 256), (unsigned)n), dim3(256), 0, nullptr, nv, H, W,
                           (const float *)v.p, (const double *)c.p, img.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpy(out, img.p, view * n, hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
