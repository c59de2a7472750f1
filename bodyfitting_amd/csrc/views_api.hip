// Host side of the GeneBody view preparation (reference apps/genebody_fitting.py:111-142, utils/io_utils.py:97-136): the resident
// masks, the crop buffer, the outputs (all grown to the largest frame seen) and the launch sequence.  Kernels: views_kernels.hip.
// The crop rectangle itself is image_cropping's scalar arithmetic and stays on the host (bodyfitting_amd/genebody.py).
#include "bf_host.h"
#include "views_kernels.h"

struct bf_views {
    int device = 0, L = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    DevBuf<uint8_t> masks, crops, out_img, out_msk;
    DevBuf<int> bbox;
    DevBuf<VwJob> jobs;
    DevBuf<unsigned long long> sums;
    std::vector<VwJob> host_jobs;
    int n = 0, H = 0, W = 0;                     // the resident masks (n = 0: none)
    long long stride = 0;
    float ms[6] = {0, 0, 0, 0, 0, 0};
    int64_t bytes[3] = {0, 0, 0};
};

namespace {
// grow a buffer to `count` elements; the stream is drained first (the old block may still be read by queued work)
template <class T>
hipError_t vw_reserve(bf_views *v, DevBuf<T> &b, size_t count) {
    if (b.p && b.n >= count) return hipSuccess;
    hipError_t e = hipStreamSynchronize(v->stream);
    if (e != hipSuccess) return e;
    b.release();
    return b.alloc(count);
}
inline size_t vw_blocks(long long work, long long per_block) { return (size_t)((work + per_block - 1) / per_block); }
}  // namespace

extern "C" {

void bf_views_destroy(bf_views *v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->stream) { (void)hipStreamSynchronize(v->stream); (void)hipStreamDestroy(v->stream); }
    for (hipEvent_t &e : v->ev)
        if (e) (void)hipEventDestroy(e);
    delete v;
}

int bf_views_create(int device, int max_views, int max_h, int max_w, int L, bf_views **out) {
    if (!out || max_views < 0 || max_h < 0 || max_w < 0 || L < 1 || L > 8192) return fail(BF_ERR_INVALID, "bf_views_create: bad argument (1 <= L <= 8192)");
    *out = nullptr;
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_views_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto *v = new bf_views();
    v->device = device; v->L = L;
    bool ok = hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) == hipSuccess;
    for (hipEvent_t &e : v->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    // the sizes given are where the buffers start; a larger frame grows them
    const size_t nv = (size_t)max_views, hw = (size_t)max_h * max_w;
    if (ok && nv > 0) {
        ok = vw_reserve(v, v->bbox, nv * 4) == hipSuccess && vw_reserve(v, v->sums, nv) == hipSuccess &&
             vw_reserve(v, v->jobs, nv) == hipSuccess && vw_reserve(v, v->out_img, nv * L * L * 3) == hipSuccess &&
             vw_reserve(v, v->out_msk, nv * L * L) == hipSuccess;
        if (ok && hw > 0)
            ok = vw_reserve(v, v->masks, nv * ((hw + 15) & ~(size_t)15)) == hipSuccess && vw_reserve(v, v->crops, nv * hw * 3) == hipSuccess;
    }
    if (!ok) { bf_views_destroy(v); return fail(BF_ERR_HIP, "bf_views_create: device allocation failed"); }
    *out = v;
    return BF_OK;
}

int bf_views_bbox(bf_views *v, int n, int H, int W, const uint8_t *const *masks, int *bbox) {
    if (!v || n < 1 || H < 1 || W < 1 || !masks || !bbox) return fail(BF_ERR_INVALID, "bf_views_bbox: bad argument");
    for (int i = 0; i < n; ++i)
        if (!masks[i]) return fail(BF_ERR_INVALID, "bf_views_bbox: view " + std::to_string(i) + " has no mask");
    HIP_TRY(hipSetDevice(v->device));
    v->n = 0;
    const long long hw = (long long)H * W, stride = (hw + 15) & ~15LL;
    HIP_TRY(vw_reserve(v, v->masks, (size_t)(n * stride)));
    HIP_TRY(vw_reserve(v, v->bbox, (size_t)n * 4));
    hipStream_t s = v->stream;
    HIP_TRY(hipEventRecord(v->ev[0], s));
    for (int i = 0; i < n; ++i) HIP_TRY(hipMemcpyAsync(v->masks.p + i * stride, masks[i], (size_t)hw, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(v->ev[1], s));
    hipLaunchKernelGGL(bf_views_bbox_init_kernel, dim3((unsigned)vw_blocks(4LL * n, 256)), dim3(256), 0, s, n, v->bbox.p);
    HIP_TRY(hipGetLastError());
    // four 16-byte chunks per thread
    const size_t per_view = std::min<size_t>(vw_blocks(stride >> 4, 256 * 4), 65535);
    hipLaunchKernelGGL(bf_views_bbox_kernel, dim3((unsigned)per_view, (unsigned)n), dim3(256), 0, s, H, W, stride,
                       (const uint8_t *)v->masks.p, v->bbox.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(v->ev[2], s));
    HIP_TRY(hipMemcpyAsync(bbox, v->bbox.p, (size_t)n * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(v->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&v->ms[k], v->ev[k], v->ev[k + 1]));
    v->bytes[0] = n * hw;
    // utils/io_utils.py:98-102: np.min of an empty np.where raises ValueError
    for (int i = 0; i < n; ++i)
        if (bbox[i * 4 + 2] < 0) return fail(BF_ERR_INVALID, "bf_views_bbox: view " + std::to_string(i) + ": the mask is empty (no pixel != 0)");
    v->n = n; v->H = H; v->W = W; v->stride = stride;
    return BF_OK;
}

int bf_views_prepare(bf_views *v, int n, const int *rects, const uint8_t *const *images, const int *mask_view, uint8_t *out_images,
                     uint8_t *out_masks, int64_t *sums) {
    if (!v || !rects || !images || !out_images || !sums) return fail(BF_ERR_INVALID, "bf_views_prepare: bad argument");
    if (v->n < 1 || n != v->n) return fail(BF_ERR_INVALID, "bf_views_prepare: n must be the view count of the last successful bf_views_bbox");
    const int H = v->H, W = v->W, L = v->L;
    v->host_jobs.resize(n);
    long long at = 0;
    bool any_mask = false;
    for (int i = 0; i < n; ++i) {
        const int top = rects[i * 4], left = rects[i * 4 + 1], bottom = rects[i * 4 + 2], right = rects[i * 4 + 3];
        if (!(0 <= top && top < bottom && bottom <= H && 0 <= left && left < right && right <= W))
            return fail(BF_ERR_INVALID, "bf_views_prepare: view " + std::to_string(i) + ": the crop rectangle is empty or outside the " +
                                            std::to_string(H) + " x " + std::to_string(W) + " view");
        if (!images[i]) return fail(BF_ERR_INVALID, "bf_views_prepare: view " + std::to_string(i) + " has no image");
        const bool m = mask_view && mask_view[i];
        any_mask = any_mask || m;
        VwJob &j = v->host_jobs[i];
        j.img_off = at + (long long)left * 3; j.msk_off = i * v->stride + (long long)top * W + left;
        j.ch = bottom - top; j.cw = right - left; j.mask_slot = m ? i : -1;
        at += (long long)j.ch * W * 3;
    }
    if (any_mask && !out_masks) return fail(BF_ERR_INVALID, "bf_views_prepare: mask views need out_masks");
    HIP_TRY(hipSetDevice(v->device));
    const size_t LL = (size_t)L * L;
    HIP_TRY(vw_reserve(v, v->crops, (size_t)at));
    HIP_TRY(vw_reserve(v, v->jobs, (size_t)n));
    HIP_TRY(vw_reserve(v, v->sums, (size_t)n));
    HIP_TRY(vw_reserve(v, v->out_img, n * LL * 3));
    if (any_mask) HIP_TRY(vw_reserve(v, v->out_msk, n * LL));
    hipStream_t s = v->stream;
    HIP_TRY(hipEventRecord(v->ev[4], s));
    // only the crop's rows go up, whole: one contiguous copy per view.  The 2-D copy of the rectangle alone (hipMemcpy2DAsync with
    // the view's pitch) moves 30 % fewer bytes but ran at 1 GB/s from pageable memory against 50 GB/s for these (profiles/genebody_bench.md)
    for (int i = 0; i < n; ++i) {
        const VwJob &j = v->host_jobs[i];
        const size_t row0 = (size_t)rects[i * 4] * W * 3;
        HIP_TRY(hipMemcpyAsync(v->crops.p + j.img_off - (long long)rects[i * 4 + 1] * 3, images[i] + row0, (size_t)j.ch * W * 3,
                               hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(v->jobs.p, v->host_jobs.data(), n * sizeof(VwJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(v->ev[5], s));
    HIP_TRY(hipMemsetAsync(v->sums.p, 0, n * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(bf_views_prepare_kernel, dim3((unsigned)vw_blocks((long long)LL, 256), (unsigned)n), dim3(256), 0, s, L, W,
                       (const VwJob *)v->jobs.p, (const uint8_t *)v->crops.p, (const uint8_t *)v->masks.p, v->out_img.p,
                       any_mask ? v->out_msk.p : (uint8_t *)nullptr, v->sums.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(v->ev[6], s));
    HIP_TRY(hipMemcpyAsync(out_images, v->out_img.p, n * LL * 3, hipMemcpyDeviceToHost, s));
    int64_t down = (int64_t)(n * LL * 3 + n * sizeof(int64_t));
    for (int i = 0; i < n && any_mask; ++i)
        if (v->host_jobs[i].mask_slot >= 0) {
            HIP_TRY(hipMemcpyAsync(out_masks + i * LL, v->out_msk.p + i * LL, LL, hipMemcpyDeviceToHost, s));
            down += (int64_t)LL;
        }
    HIP_TRY(hipMemcpyAsync(sums, v->sums.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(v->ev[7], s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&v->ms[3 + k], v->ev[4 + k], v->ev[5 + k]));
    v->bytes[1] = at + (int64_t)(n * sizeof(VwJob));
    v->bytes[2] = down;
    return BF_OK;
}

int bf_views_last_timing(bf_views *v, float *ms, int64_t *bytes) {
    if (!v || !ms || !bytes) return fail(BF_ERR_INVALID, "bf_views_last_timing: bad argument");
    for (int k = 0; k < 6; ++k) ms[k] = v->ms[k];
    for (int k = 0; k < 3; ++k) bytes[k] = v->bytes[k];
    return BF_OK;
}

}  // extern "C"
