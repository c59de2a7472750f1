// Host side of bf_silhouette_* (include/bodyfit.h): multview_mask_loss (smplify/loss.py:85-130) on vertices the caller holds, as one
// call on host arrays for a user's own torch loop.  The object keeps the views' masks and contours on the device and the call's
// buffers between calls; an evaluation is one upload (projection rows + vertices), three launches (silhouette_kernels.hip) and one
// read-back (loss, view terms, gradient), with no host wait in between.  Everything runs on the NULL stream, like the host route
// of the stateless calls (dev_route.h) - whose buffers, unlike this object's, come from the block cache call by call.
//
// The device route (bf_silhouette_create_dev, bf_silhouette_contours_dev, bf_silhouette_loss_dev) takes masks, vertices and cameras
// as device arrays on the caller's stream: the masks are binarised and checked by a kernel (only M + 1 flags are read back, once per
// object), the projection rows come from a kernel instead of the host loop, the scratch from a bf_workspace, and the evaluation's
// three launches are the host entry's - ONE function, bf_sil_launch, issues them for both.
#include "bf_host.h"
#include "dev_route.h"
#include "silhouette_kernels.h"

struct bf_silhouette {
    int device = 0, M = 0, H = 0, W = 0;
    int cmax = 1, longest = 0;
    std::vector<int> counts;               // [M] contour lengths
    size_t total = 0;                      // their sum
    DevBuf<unsigned char> masks;           // [M][H][W], 1 = foreground
    DevBuf<int> view, cstart, ccount;      // [M]: identity, offsets into cxy, lengths
    DevBuf<float> cxy;                     // [total + 1][2] (one pair of padding: a view without points still reads one)
    // the call's buffers, kept and only grown
    DevBuf<float> in, uvi, duvb, part, out;
    DevBuf<unsigned long long> acc;
    std::vector<float> h_in, h_out;
};

namespace {
constexpr int BF_SIL_MAX_VERTS = 1 << 28;          // index * 3 stays inside an int

// max(|epsilon|, 1) x longest contour x 2^BF_ACC_SHIFT <= 2^60: |du|, |dv| of one (view, vertex) - a sum of `longest` unit-vector
// components weighted by 1 or epsilon - stays a factor of 8 inside the 63 bits of the fixed-point sums
bool bf_sil_sums_fit(float epsilon, int longest) {
    static_assert(BF_ACC_SHIFT + 20 + 3 == 63, "BF_SIL_MAX_SUM: 2^20 x 2^BF_ACC_SHIFT is 1/8 of 2^63");
    return std::max((double)std::fabs(epsilon), 1.0) * (double)longest <= (double)BF_SIL_MAX_SUM;
}

// the external borders of s->masks followed on the device, the one `contour_select` names kept: counts, total, cxy
int bf_sil_follow(bf_silhouette *s, const char *who, int contour_select) {
    const int M = s->M;
    std::vector<int> half;
    DevBuf<float> slab;
    int cap = 0;
    BF_TRY(bf_contours_on_device(s->masks.p, M, s->H, s->W, contour_select, s->counts, half, slab, cap));
    for (int i = 0; i < M; ++i) {
        if (s->counts[i] > BF_SIL_MAX_CONTOUR) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": a contour of more than " + std::to_string(BF_SIL_MAX_CONTOUR) + " points");
        s->total += (size_t)s->counts[i];
    }
    if (s->total > (size_t)INT32_MAX) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 contour points in all");
    HIP_TRY(s->cxy.alloc((s->total + 1) * 2));
    size_t o = 0;
    for (int i = 0; i < M; ++i) {
        if (s->counts[i] > 0)
            HIP_TRY(hipMemcpy(s->cxy.p + o * 2, slab.p + ((size_t)i * 2 + half[i]) * cap * 2, (size_t)s->counts[i] * 2 * sizeof(float), hipMemcpyDeviceToDevice));
        o += (size_t)s->counts[i];
    }
    HIP_TRY(hipDeviceSynchronize());               // (the slab is freed on return)
    return BF_OK;
}

// the padding pair behind the contours and the per-view tables; the device is drained: the object is complete for any stream
int bf_sil_seal(bf_silhouette *s) {
    const int M = s->M;
    std::vector<int> start(M), ident(M);
    HIP_TRY(hipMemset(s->cxy.p + s->total * 2, 0, 2 * sizeof(float)));
    size_t o = 0;
    for (int i = 0; i < M; ++i) {
        start[i] = (int)o; ident[i] = i; o += (size_t)s->counts[i];
        s->longest = std::max(s->longest, s->counts[i]);
    }
    s->cmax = std::max(1, s->longest);
    HIP_TRY(s->cstart.upload(start)); HIP_TRY(s->ccount.upload(s->counts)); HIP_TRY(s->view.upload(ident));
    HIP_TRY(hipDeviceSynchronize());
    return BF_OK;
}

// what both loss entries refuse, before anything is queued
int bf_sil_loss_check(const char *who, const bf_silhouette *s, int n_verts, int stride, const float *verts, const float *w2c, const float *K,
                      float imsize, float epsilon) {
    if (!s || !verts || !w2c || !K) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    if (n_verts < 1 || stride < 1) return fail(BF_ERR_INVALID, std::string(who) + ": n_verts and stride must be positive");
    if (!std::isfinite(imsize) || !std::isfinite(epsilon) || !(imsize > 0.f))
        return fail(BF_ERR_INVALID, std::string(who) + ": imsize must be finite and positive, epsilon finite");
    if (n_verts > BF_SIL_MAX_VERTS) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(BF_SIL_MAX_VERTS) + " vertices");
    if (!bf_sil_sums_fit(epsilon, s->longest))
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": max(|epsilon|, 1) x the longest contour (" + std::to_string(s->longest) + " points) exceeds " +
                                            std::to_string(BF_SIL_MAX_SUM) + ": the fixed-point gradient sums could overflow");
    return BF_OK;
}

// rows[M][12] = K [R|t] from device arrays w2c[M][16], K[M][9]: the device route's twin of bf_silhouette_loss' host loop
void bf_sil_rows_launch(hipStream_t st, int M, const float *w2c, const float *K, float *rows) {
    hipLaunchKernelGGL(bf_sil_rows_kernel, dim3((unsigned)((M * 12 + 255) / 256)), dim3(256), 0, st, K, w2c, M, rows);
}

// the sizes of one evaluation, the same on both routes
struct SilShape {
    int M, ns, pblocks, cblocks;
    size_t nv3, n_terms, vm;
    SilShape(const bf_silhouette *s, int n_verts, int stride)
        : M(s->M), ns((n_verts + stride - 1) / stride), pblocks((ns + 255) / 256), cblocks((s->cmax * 16 + 255) / 256), nv3((size_t)n_verts * 3),
          n_terms(1 + 2 * (size_t)s->M), vm((size_t)s->M * ns) {}
};

// The three launches of one evaluation, on `st`, for both routes: d_proj[M][12] and d_verts[n_verts][3] in, terms[1 + 2M] and
// dverts[n_verts][3] (or null) out, uvi[vm][4], duvb[vm][2], acc[vm][2] and part[M][pblocks + cblocks] scratch - every element of
// them that is read is written here first (the project kernel zeroes the sums: no memset).
int bf_sil_launch(const bf_silhouette *s, hipStream_t st, const SilShape &z, int n_verts, int stride, float imsize, float epsilon, int cdist_form,
                  const float *d_proj, const float *d_verts, float *uvi, float *duvb, unsigned long long *acc, float *part, float *terms,
                  float *dverts) {
    const int M = z.M;
    MaskIO Q{};
    Q.nv = n_verts; Q.ns = z.ns; Q.n_views = M; Q.n_masks = M; Q.H = s->H; Q.W = s->W; Q.cmax = s->cmax;
    Q.part_stride = z.pblocks + z.cblocks; Q.proj_blocks = z.pblocks;
    Q.cdist = cdist_form != 0; Q.sstride = stride;
    Q.imsize = imsize; Q.eps = epsilon; Q.weight = 1.f;
    Q.view_index = s->view.p; Q.masks = s->masks.p;
    Q.contour_start = s->cstart.p; Q.contour_count = s->ccount.p; Q.contour_xy = s->cxy.p;
    Q.acc = acc;
    hipLaunchKernelGGL(bf_sil_project_kernel, dim3(z.pblocks, M), dim3(256), 0, st, Q, d_verts, d_proj, uvi, duvb, part);
    hipLaunchKernelGGL(bf_sil_contour_kernel, dim3(z.cblocks, M), dim3(256), 0, st, Q, (const float *)uvi, part);
    const unsigned vblocks = dverts ? (unsigned)((n_verts + 255) / 256) : 0u;
    hipLaunchKernelGGL(bf_sil_finish_kernel, dim3(vblocks + 1), dim3(256), 0, st, Q, d_proj, (const float *)uvi, (const float *)duvb,
                       (const float *)part, terms, dverts);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}
}  // namespace

extern "C" int bf_silhouette_create(int device, int n_views, int H, int W, const uint8_t *masks, const int32_t *contour_count,
                                    const float *contour_xy, int contour_select, bf_silhouette **out) {
    const char *who = "bf_silhouette_create";
    if (!out) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    *out = nullptr;
    if (!masks || n_views < 1 || H < 1 || W < 1) return fail(BF_ERR_INVALID, std::string(who) + ": no masks / a size below 1");
    if (n_views > BF_SIL_MAX_VIEWS || H > BF_SIL_MAX_SIDE || W > BF_SIL_MAX_SIDE)
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(BF_SIL_MAX_VIEWS) + " views or a side beyond " + std::to_string(BF_SIL_MAX_SIDE));
    const int M = n_views;
    std::unique_ptr<bf_silhouette> s(new bf_silhouette);
    s->device = device; s->M = M; s->H = H; s->W = W;
    s->counts.assign(M, 0);
    if (contour_count) {
        for (int i = 0; i < M; ++i) {
            if (contour_count[i] < 0) return fail(BF_ERR_INVALID, std::string(who) + ": negative contour count");
            if (contour_count[i] > BF_SIL_MAX_CONTOUR) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": a contour of more than " + std::to_string(BF_SIL_MAX_CONTOUR) + " points");
            s->counts[i] = contour_count[i];
            s->total += (size_t)contour_count[i];
        }
        if (s->total > 0 && !contour_xy) return fail(BF_ERR_INVALID, std::string(who) + ": contour_count without contour_xy");
    } else if (contour_select < 0 || contour_select > 2)
        return fail(BF_ERR_INVALID, std::string(who) + ": bad contour_select");
    if (bf_device_count() <= device || device < 0) return fail(BF_ERR_NO_DEVICE, std::string(who) + ": no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)M * H * W;
    std::vector<unsigned char> bin(npix);
    for (size_t i = 0; i < npix; ++i) bin[i] = masks[i] != 0;
    HIP_TRY(s->masks.upload(bin));
    if (contour_count) {
        if (s->total > (size_t)INT32_MAX) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 contour points in all");
        HIP_TRY(s->cxy.alloc((s->total + 1) * 2));
        if (s->total > 0) HIP_TRY(hipMemcpy(s->cxy.p, contour_xy, s->total * 2 * sizeof(float), hipMemcpyHostToDevice));
    } else
        BF_TRY(bf_sil_follow(s.get(), who, contour_select));
    BF_TRY(bf_sil_seal(s.get()));
    *out = s.release();
    return BF_OK;
}

extern "C" int bf_silhouette_create_dev(int device, int n_views, int H, int W, const void *masks, int mask_dtype, int contour_select,
                                        void *stream, bf_silhouette **out) {
    const char *who = "bf_silhouette_create_dev";
    if (!out) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    *out = nullptr;
    if (!masks || n_views < 1 || H < 1 || W < 1) return fail(BF_ERR_INVALID, std::string(who) + ": no masks / a size below 1");
    if (n_views > BF_SIL_MAX_VIEWS || H > BF_SIL_MAX_SIDE || W > BF_SIL_MAX_SIDE)
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(BF_SIL_MAX_VIEWS) + " views or a side beyond " + std::to_string(BF_SIL_MAX_SIDE));
    if (mask_dtype != BF_MASK_UINT8 && mask_dtype != BF_MASK_FLOAT32) return fail(BF_ERR_INVALID, std::string(who) + ": bad mask_dtype");
    if (contour_select < 0 || contour_select > 2) return fail(BF_ERR_INVALID, std::string(who) + ": bad contour_select");
    if (bf_device_count() <= device || device < 0) return fail(BF_ERR_NO_DEVICE, std::string(who) + ": no such HIP device");
    if (bf_device_pointer_check(device, masks) != BF_OK) return fail(BF_ERR_INVALID, std::string(who) + ": masks is not memory of that device");
    const int M = n_views;
    const hipStream_t st = (hipStream_t)stream;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<bf_silhouette> s(new bf_silhouette);
    s->device = device; s->M = M; s->H = H; s->W = W;
    s->counts.assign(M, 0);
    const size_t npix = (size_t)M * H * W, words = (npix + 3) / 4;
    HIP_TRY(s->masks.alloc(words * 4));
    DevBuf<int> d_flags;
    HIP_TRY(d_flags.alloc((size_t)M + 1));
    ++bf_route_stats().dev;
    HIP_TRY(hipMemsetAsync(d_flags.p, 0, ((size_t)M + 1) * sizeof(int), st));
    hipLaunchKernelGGL(bf_sil_ingest_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, masks, mask_dtype == BF_MASK_FLOAT32 ? 1 : 0,
                       (unsigned long long)npix, (unsigned)((size_t)H * W), (unsigned *)s->masks.p, d_flags.p, M);
    HIP_TRY(hipGetLastError());
    // the one wait of the object's life: the flags are the only thing of the masks the host sees
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> flags((size_t)M + 1);
    HIP_TRY(hipMemcpy(flags.data(), d_flags.p, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (flags[M]) return fail(BF_ERR_INVALID, std::string(who) + ": masks must hold 0 / 1 only");
    for (int i = 0; i < M; ++i)
        if (!flags[i]) {
            (void)fail(BF_ERR_INVALID, std::string(who) + ": mask " + std::to_string(i) + " has no foreground");
            return BF_SIL_EMPTY_VIEW + i;
        }
    BF_TRY(bf_sil_follow(s.get(), who, contour_select));
    BF_TRY(bf_sil_seal(s.get()));
    *out = s.release();
    return BF_OK;
}

extern "C" void bf_silhouette_destroy(bf_silhouette *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
}

extern "C" int bf_silhouette_contours(const bf_silhouette *s, int32_t *counts, float *xy) {
    if (!s || !counts) return fail(BF_ERR_INVALID, "bf_silhouette_contours: bad argument");
    for (int i = 0; i < s->M; ++i) counts[i] = s->counts[i];
    if (xy && s->total > 0) {
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipMemcpy(xy, s->cxy.p, s->total * 2 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return BF_OK;
}

extern "C" int bf_silhouette_contours_dev(const bf_silhouette *s, float *xy, void *stream) {
    if (!s || !xy) return fail(BF_ERR_INVALID, "bf_silhouette_contours_dev: bad argument");
    ++bf_route_stats().dev;
    if (s->total == 0) return BF_OK;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(xy, s->cxy.p, s->total * 2 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BF_OK;
}

extern "C" int bf_silhouette_loss(bf_silhouette *s, int n_verts, int stride, const float *verts, const float *w2c, const float *K,
                                  float imsize, float epsilon, int cdist_form, float *loss, float *view_terms, float *dverts) {
    BF_TRY(bf_sil_loss_check("bf_silhouette_loss", s, n_verts, stride, verts, w2c, K, imsize, epsilon));
    ++bf_route_stats().host;
    if (!loss && !view_terms && !dverts) return BF_OK;
    HIP_TRY(hipSetDevice(s->device));
    const SilShape z(s, n_verts, stride);
    const int M = z.M;
    const size_t nv3 = z.nv3, n_terms = z.n_terms, vm = z.vm;
    HIP_TRY(bf_grow(nullptr, s->in, (size_t)M * 12 + nv3));
    HIP_TRY(bf_grow(nullptr, s->uvi, vm * 4)); HIP_TRY(bf_grow(nullptr, s->duvb, vm * 2)); HIP_TRY(bf_grow(nullptr, s->acc, vm * 2));
    HIP_TRY(bf_grow(nullptr, s->part, (size_t)M * (z.pblocks + z.cblocks)));
    // (terms padded to a multiple of 4 floats: the gradient behind them starts 16-byte aligned)
    const size_t o_dv = (n_terms + 3) & ~(size_t)3;
    HIP_TRY(bf_grow(nullptr, s->out, o_dv + nv3));
    // the 3 x 4 rows K [R|t] per view, in double like bf_batch_set_cameras, and the vertices behind them: one upload
    // (the device route's rows come from bf_sil_rows_kernel, the same expression)
    s->h_in.resize((size_t)M * 12 + nv3);
    for (int i = 0; i < M; ++i) {
        const float *k = K + (size_t)i * 9, *w = w2c + (size_t)i * 16;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                s->h_in[(size_t)i * 12 + r * 4 + c] = (float)((double)k[r * 3] * w[c] + (double)k[r * 3 + 1] * w[4 + c] + (double)k[r * 3 + 2] * w[8 + c]);
    }
    std::memcpy(s->h_in.data() + (size_t)M * 12, verts, nv3 * sizeof(float));
    HIP_TRY(hipMemcpy(s->in.p, s->h_in.data(), s->h_in.size() * sizeof(float), hipMemcpyHostToDevice));
    BF_TRY(bf_sil_launch(s, nullptr, z, n_verts, stride, imsize, epsilon, cdist_form, s->in.p, s->in.p + (size_t)M * 12, s->uvi.p, s->duvb.p, s->acc.p,
                         s->part.p, s->out.p, dverts ? s->out.p + o_dv : (float *)nullptr));
    s->h_out.resize(dverts ? o_dv + nv3 : n_terms);
    HIP_TRY(hipMemcpy(s->h_out.data(), s->out.p, s->h_out.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (loss) loss[0] = s->h_out[0];
    if (view_terms) std::memcpy(view_terms, s->h_out.data() + 1, 2 * (size_t)M * sizeof(float));
    if (dverts) std::memcpy(dverts, s->h_out.data() + o_dv, nv3 * sizeof(float));
    return BF_OK;
}

extern "C" int bf_silhouette_rows_dev(int device, int n_views, const float *w2c, const float *K, float *rows, void *stream) {
    const char *who = "bf_silhouette_rows_dev";
    if (!w2c || !K || !rows) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    if (n_views < 1) return fail(BF_ERR_INVALID, std::string(who) + ": n_views must be positive");
    if (n_views > BF_SIL_MAX_VIEWS) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(BF_SIL_MAX_VIEWS) + " views");
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(device));
    bf_sil_rows_launch((hipStream_t)stream, n_views, w2c, K, rows);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_silhouette_loss_dev(bf_silhouette *s, int n_verts, int stride, const float *verts, const float *w2c, const float *K,
                                      float imsize, float epsilon, int cdist_form, float *terms, float *dverts, bf_workspace *ws, void *stream) {
    const char *who = "bf_silhouette_loss_dev";
    BF_TRY(bf_sil_loss_check(who, s, n_verts, stride, verts, w2c, K, imsize, epsilon));
    BF_TRY(bf_ml_dev_check(who, ws, s->device));
    ++bf_route_stats().dev;
    if (!terms && !dverts) return BF_OK;
    BfRouteCall c(ws, (hipStream_t)stream);
    BF_TRY(c.begin(s->device));
    const SilShape z(s, n_verts, stride);
    float *d_proj = nullptr, *uvi = nullptr, *duvb = nullptr, *part = nullptr, *d_terms = nullptr;
    unsigned long long *acc = nullptr;
    BF_TRY(c.scratch((size_t)z.M * 12, d_proj));
    BF_TRY(c.scratch(z.vm * 4, uvi)); BF_TRY(c.scratch(z.vm * 2, duvb)); BF_TRY(c.scratch(z.vm * 2, acc));
    BF_TRY(c.scratch((size_t)z.M * (z.pblocks + z.cblocks), part));
    BF_TRY(c.out(terms, z.n_terms, d_terms, true));          // (the finish kernel's last block writes them whoever wants them)
    // the one `if` between the routes: where the rows come from
    bf_sil_rows_launch(c.stream, z.M, w2c, K, d_proj);
    BF_TRY(bf_sil_launch(s, c.stream, z, n_verts, stride, imsize, epsilon, cdist_form, d_proj, verts, uvi, duvb, acc, part, d_terms, dverts));
    return c.finish();
}
