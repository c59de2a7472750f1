// Host side of the LBAM texture inpainter (reference models/inpaint.py Inpainter / LBAMModel(4, 3), smplify/texture_fitting.py
// TextureFitting.inpaint): the layer list and packed-weight offsets, the buffers (sized at creation by max_batch x max_h x max_w),
// the split-K plan and the launch sequence.  Kernels: inpaint_kernels.hip.
#include "bf_host.h"
#include "inpaint.h"


namespace {
const int ENC[8] = {4, 64, 128, 256, 512, 512, 512, 512};        // ec1..ec7: ENC[l - 1] -> ENC[l] (ec1's input padded 4, mask 3 -> 4)
const int REV[7] = {4, 64, 128, 256, 512, 512, 512};             // reverseConv1..6 (the 3-channel 1 - mask padded to 4)
const int DEC[7][2] = {{512, 512}, {1024, 512}, {1024, 512}, {1024, 256}, {512, 128}, {256, 64}, {128, 3}};
const int IP_SIDE = 128;                                         // seven halvings
const int IP_SPLIT_WG = 512;                                     // a split layer aims at this many workgroups
const size_t IP_PART_PER_IMAGE = (size_t)IP_SPLIT_WG * 128 * 128;  // split partials per image, floats (ip_plan's bound)

inline unsigned ip_blocks(long long total) { return (unsigned)((total + 255) / 256); }
inline int ip_pad4(int c) { return (c + 3) / 4 * 4; }

// The packed layout bodyfitting_amd/inpaint.py pack() writes: reverseConv1..6, ec1..7 (conv, maskConv), dc1..7 (four phases each),
// then the clamped GaussActivation parameters of reverseConv1..6 and ec1..7
struct IpLayout {
    size_t rc[6], ec[7], em[7], dc[7], gauss, total;
    IpLayout() {
        size_t at = 0;
        for (int l = 1; l <= 6; ++l) { rc[l - 1] = at; at += (size_t)16 * REV[l - 1] * REV[l]; }
        for (int l = 1; l <= 7; ++l) {
            ec[l - 1] = at; at += (size_t)16 * ENC[l - 1] * ENC[l];
            em[l - 1] = at; at += (size_t)16 * ENC[l - 1] * ENC[l];
        }
        for (int t = 1; t <= 7; ++t) { dc[t - 1] = at; at += (size_t)16 * DEC[t - 1][0] * ip_pad4(DEC[t - 1][1]); }
        gauss = at;
        total = at + 13 * 4;
    }
};
}  // namespace

struct bf_inpaint {
    int device = 0, max_batch = 0, max_h = 0, max_w = 0;
    hipStream_t stream = nullptr;
    IpLayout lay;
    float gauss[13][4];                                          // rc1..6, ec1..7
    DevBuf<float> w, xin, mk, rmk, cat[6], e7, rmap[6], mq[2], part, out;
    DevBuf<uint8_t> img, msk, q8, qm, e8, em, dm, sel;
    DevBuf<float> uv;
    DevBuf<int> err;
};

// the split count of a layer from its per-image shape (P GEMM rows per phase per image), never the batch: K is cut when the layer's
// tiles would leave most of the 256 CUs idle, into chunks of a multiple of 16 no shorter than 128
static void ip_plan(int P, int cout, int K, int bn, int phases, int *splits, int *kper) {
    const int tiles = (P + 127) / 128 * ((cout + bn - 1) / bn) * phases;
    int s = 1;
    if (tiles < 256 && K >= 1024) s = std::max(1, std::min(IP_SPLIT_WG / tiles, K / 128));
    int kp = (K + s - 1) / s;
    kp = (kp + 15) / 16 * 16;
    *kper = kp;
    *splits = (K + kp - 1) / kp;
}

static int ip_launch(hipStream_t s, IpConv c, float *part, size_t part_floats) {
    const bool dual = c.xm != nullptr;
    const int bn = dual || c.cout <= 64 ? 64 : 128;
    const int phases = c.deconv ? 4 : 1;
    const int P = c.deconv ? c.Hi * c.Wi : c.Ho * c.Wo, M = c.n * P, K = c.cin * (c.deconv ? 4 : 16);
    ip_plan(P, c.cout, K, bn, phases, &c.splits, &c.kper);
    if ((size_t)M * c.coutp * 4 >= ((size_t)1 << 31) || (size_t)c.n * c.Hi * c.Wi * std::max(c.ldx, c.ldxm) >= ((size_t)1 << 31))
        return fail(BF_ERR_UNSUPPORTED, "bf_inpaint: a layer outside what the kernels index");
    if (c.splits > 1) {
        const size_t need = (size_t)c.splits * phases * M * c.coutp * (dual ? 2 : 1);
        if (need > part_floats) return fail(BF_ERR_UNSUPPORTED, "bf_inpaint: split-K partials exceed the workspace");
        c.part = part;
    }
    const dim3 grid((unsigned)((M + 127) / 128), (unsigned)((c.cout + bn - 1) / bn), (unsigned)(c.splits * phases));
    if (dual) hipLaunchKernelGGL(bf_ip_enc_kernel, grid, dim3(256), 0, s, c);
    else if (c.deconv) hipLaunchKernelGGL(bn == 128 ? bf_ip_dec128_kernel : bf_ip_dec64_kernel, grid, dim3(256), 0, s, c);
    else hipLaunchKernelGGL(bn == 128 ? bf_ip_rev128_kernel : bf_ip_rev64_kernel, grid, dim3(256), 0, s, c);
    HIP_TRY(hipGetLastError());
    if (c.splits > 1) {
        hipLaunchKernelGGL(bf_ip_reduce_kernel, dim3(ip_blocks((long long)phases * M * c.cout)), dim3(256), 0, s, c, dual ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    return BF_OK;
}

static IpConv ip_conv(int n, int Hi, int Wi, int deconv) {
    IpConv c;
    std::memset(&c, 0, sizeof(c));
    c.n = n; c.Hi = Hi; c.Wi = Wi; c.deconv = deconv;
    c.Ho = deconv ? 2 * Hi : Hi / 2; c.Wo = deconv ? 2 * Wi : Wi / 2;
    c.splits = 1;
    return c;
}

static void ip_gauss(IpConv &c, const float *g) { c.ga = g[0]; c.gmu = g[1]; c.gs1 = g[2]; c.gs2 = g[3]; }

// LBAMModel.forward (inpaint.py:335-357) on h->xin / mk / rmk (n x H x W) -> h->out (n x H x W x 3, Inpainter's blend included).
// The reverse chain runs first, so the encoder's mask updates reuse its ping-pong buffers.  LeakyReLU(skip * forwardMap) - the
// first half of every decoder output - is the same float32 product as the encoder's own features ef, so the encoder writes ef once,
// into channels [0, C) of the decoder's concatenated output at its level, and the next encoder level reads it from there; skip and
// forwardMap never go to memory.
static int ip_network(bf_inpaint *h, int n, int H, int W) {
    hipStream_t s = h->stream;
    const float *Wt = h->w.p;
    const size_t pf = h->part.n;
    const float *r = h->rmk.p;
    int ldr = 4;
    for (int l = 1; l <= 6; ++l) {
        IpConv c = ip_conv(n, H >> (l - 1), W >> (l - 1), 0);
        c.x = r; c.ldx = ldr; c.cin = REV[l - 1]; c.cout = c.coutp = REV[l]; c.w = Wt + h->lay.rc[l - 1];
        c.epi = IP_EPI_REV; ip_gauss(c, h->gauss[l - 1]);
        c.y0 = h->rmap[l - 1].p; c.ld0 = REV[l];
        c.y1 = l < 6 ? h->mq[l & 1].p : nullptr; c.ld1 = REV[l];
        if (int rc = ip_launch(s, c, h->part.p, pf)) return rc;
        r = c.y1; ldr = REV[l];
    }
    const float *x = h->xin.p, *m = h->mk.p;
    int ldx = 4, ldm = 4;
    for (int l = 1; l <= 7; ++l) {
        IpConv c = ip_conv(n, H >> (l - 1), W >> (l - 1), 0);
        c.x = x; c.ldx = ldx; c.xm = m; c.ldxm = ldm; c.cin = ENC[l - 1]; c.cout = c.coutp = ENC[l];
        c.w = Wt + h->lay.ec[l - 1]; c.wm = Wt + h->lay.em[l - 1];
        c.epi = IP_EPI_ENC; ip_gauss(c, h->gauss[6 + l - 1]);
        c.y0 = l < 7 ? h->cat[l - 1].p : h->e7.p; c.ld0 = l < 7 ? 2 * ENC[l] : ENC[l];
        c.y1 = l < 7 ? h->mq[l & 1].p : nullptr; c.ld1 = ENC[l];          // ec7's mask update is unused
        if (int rc = ip_launch(s, c, h->part.p, pf)) return rc;
        x = c.y0; ldx = c.ld0; m = c.y1; ldm = ENC[l];
    }
    const float *d = h->e7.p;
    int ldd = 512;
    for (int t = 1; t <= 6; ++t) {
        const int l = 7 - t;                                              // dc_t writes the second half of level l's concat
        IpConv c = ip_conv(n, H >> (l + 1), W >> (l + 1), 1);
        c.x = d; c.ldx = ldd; c.cin = DEC[t - 1][0]; c.cout = c.coutp = DEC[t - 1][1]; c.w = Wt + h->lay.dc[t - 1];
        c.epi = IP_EPI_DEC;
        c.y0 = h->cat[l - 1].p + ENC[l]; c.ld0 = 2 * ENC[l];
        c.aux0 = h->rmap[l - 1].p; c.ldaux = REV[l];
        if (int rc = ip_launch(s, c, h->part.p, pf)) return rc;
        d = h->cat[l - 1].p; ldd = 2 * ENC[l];
    }
    IpConv c = ip_conv(n, H >> 1, W >> 1, 1);
    c.x = d; c.ldx = ldd; c.cin = DEC[6][0]; c.cout = 3; c.coutp = 4; c.w = Wt + h->lay.dc[6];
    c.epi = IP_EPI_OUT; c.y0 = h->out.p; c.ld0 = 3; c.aux0 = h->xin.p; c.aux1 = h->mk.p; c.ldaux = 4;
    return ip_launch(s, c, h->part.p, pf);
}

static int ip_check(bf_inpaint *h, int n, int H, int W, const char *what) {
    if (!h) return fail(BF_ERR_INVALID, std::string(what) + ": no handle");
    if (n < 1 || n > h->max_batch)
        return fail(BF_ERR_INVALID, std::string(what) + ": " + std::to_string(n) + " images, the handle takes 1 .. " + std::to_string(h->max_batch));
    if (H < IP_SIDE || W < IP_SIDE || H % IP_SIDE || W % IP_SIDE || H > h->max_h || W > h->max_w)
        return fail(BF_ERR_INVALID, std::string(what) + ": " + std::to_string(H) + " x " + std::to_string(W) +
                                        " is not a multiple of 128 on each side within the maximum " + std::to_string(h->max_h) + " x " +
                                        std::to_string(h->max_w));
    return BF_OK;
}

// prepare + network on images already in h->img / h->msk
static int ip_run_resident(bf_inpaint *h, int n, int H, int W) {
    const long long npx = (long long)n * H * W;
    hipLaunchKernelGGL(bf_ip_prepare_kernel, dim3(ip_blocks(npx)), dim3(256), 0, h->stream, npx, (const uint8_t *)h->img.p,
                       (const uint8_t *)h->msk.p, (float4 *)h->xin.p, (float4 *)h->mk.p, (float4 *)h->rmk.p);
    HIP_TRY(hipGetLastError());
    return ip_network(h, n, H, W);
}

// the face test and the fill of h->img (one image) into h->msk; *bad = a sample index outside the image
static int ip_hole_mask(bf_inpaint *h, int H, int W, int n_faces, const float *uv, bool *bad) {
    hipStream_t s = h->stream;
    *bad = false;
    HIP_TRY(hipMemsetAsync(h->msk.p, 0, (size_t)H * W * 3, s));
    if (n_faces == 0) return BF_OK;
    if (h->uv.n < (size_t)n_faces * 6) { HIP_TRY(hipStreamSynchronize(s)); h->uv.release(); HIP_TRY(h->uv.alloc((size_t)n_faces * 6)); }
    if (h->sel.n < (size_t)n_faces) { HIP_TRY(hipStreamSynchronize(s)); h->sel.release(); HIP_TRY(h->sel.alloc((size_t)n_faces)); }
    HIP_TRY(hipMemcpyAsync(h->uv.p, uv, (size_t)n_faces * 6 * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(h->err.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(bf_ip_faces_kernel, dim3(ip_blocks(n_faces)), dim3(256), 0, s, n_faces, H, W, (const uint8_t *)h->img.p,
                       (const float *)h->uv.p, h->sel.p, h->err.p);
    HIP_TRY(hipGetLastError());
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, h->err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) { *bad = true; return BF_OK; }
    hipLaunchKernelGGL(bf_ip_fill_kernel, dim3(ip_blocks(n_faces)), dim3(256), 0, s, n_faces, H, W, (const float *)h->uv.p,
                       (const uint8_t *)h->sel.p, h->msk.p);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

static int ip_morph(hipStream_t s, int op, int k, int n, int H, int W, int C, const uint8_t *in, uint8_t *out) {
    hipLaunchKernelGGL(bf_ip_morph_kernel, dim3(ip_blocks((long long)n * H * W * C)), dim3(256), 0, s, op, k, n, H, W, C, in, out);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

static int ip_fail_faces(const char *what) {
    return fail(BF_ERR_INVALID, std::string(what) + ": a face sample lies outside the image (numpy would raise IndexError)");
}

extern "C" {

int64_t bf_inpaint_n_weights(void) { return (int64_t)IpLayout().total; }

void bf_inpaint_destroy(bf_inpaint *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    delete h;
}

int bf_inpaint_create(int device, const float *weights, int64_t n_weights, int max_batch, int max_h, int max_w, bf_inpaint **out) {
    if (!out || !weights || max_batch < 1 || max_batch > 64 || max_h < IP_SIDE || max_w < IP_SIDE || max_h > 4096 || max_w > 4096)
        return fail(BF_ERR_INVALID, "bf_inpaint_create: bad argument");
    *out = nullptr;
    IpLayout lay;
    if (n_weights != (int64_t)lay.total)
        return fail(BF_ERR_INVALID, "bf_inpaint_create: " + std::to_string(n_weights) + " packed weights, the network has " + std::to_string(lay.total));
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_inpaint_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto *h = new bf_inpaint();
    h->device = device; h->max_batch = max_batch; h->max_h = max_h; h->max_w = max_w; h->lay = lay;
    std::memcpy(h->gauss, weights + lay.gauss, sizeof(h->gauss));
    const size_t px = (size_t)max_batch * max_h * max_w;
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              h->w.upload(weights, lay.gauss) == hipSuccess &&
              h->xin.alloc(px * 4) == hipSuccess && h->mk.alloc(px * 4) == hipSuccess && h->rmk.alloc(px * 4) == hipSuccess &&
              h->e7.alloc((px >> 14) * 512) == hipSuccess && h->mq[0].alloc(px * 16) == hipSuccess && h->mq[1].alloc(px * 16) == hipSuccess &&
              h->part.alloc(IP_PART_PER_IMAGE * max_batch) == hipSuccess && h->out.alloc(px * 3) == hipSuccess &&
              h->img.alloc(px * 3) == hipSuccess && h->msk.alloc(px * 3) == hipSuccess && h->err.alloc(1) == hipSuccess;
    for (int l = 1; l <= 6 && ok; ++l)
        ok = h->cat[l - 1].alloc((px >> (2 * l)) * 2 * ENC[l]) == hipSuccess && h->rmap[l - 1].alloc((px >> (2 * l)) * REV[l]) == hipSuccess;
    const size_t tex = (size_t)max_h * max_w * 3;
    ok = ok && h->q8.alloc(tex) == hipSuccess && h->qm.alloc(tex) == hipSuccess && h->e8.alloc(tex) == hipSuccess &&
         h->em.alloc(tex) == hipSuccess && h->dm.alloc(tex) == hipSuccess;
    if (!ok) { bf_inpaint_destroy(h); return fail(BF_ERR_HIP, "bf_inpaint_create: device allocation failed"); }
    *out = h;
    return BF_OK;
}

int bf_inpaint_run(bf_inpaint *h, int n, int H, int W, const uint8_t *image, const uint8_t *mask, float *out) {
    if (int rc = ip_check(h, n, H, W, "bf_inpaint_run")) return rc;
    if (!image || !mask || !out) return fail(BF_ERR_INVALID, "bf_inpaint_run: null array");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t bytes = (size_t)n * H * W * 3;
    HIP_TRY(hipMemcpyAsync(h->img.p, image, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->msk.p, mask, bytes, hipMemcpyHostToDevice, s));
    if (int rc = ip_run_resident(h, n, H, W)) return rc;
    HIP_TRY(hipMemcpyAsync(out, h->out.p, bytes * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BF_OK;
}

int bf_inpaint_select_faces(bf_inpaint *h, int H, int W, const uint8_t *img, int n_faces, const float *face_uv, uint8_t *selected) {
    if (int rc = ip_check(h, 1, H, W, "bf_inpaint_select_faces")) return rc;
    if (!img || n_faces < 0 || (n_faces && (!face_uv || !selected))) return fail(BF_ERR_INVALID, "bf_inpaint_select_faces: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->img.p, img, (size_t)H * W * 3, hipMemcpyHostToDevice, h->stream));
    bool bad = false;
    if (int rc = ip_hole_mask(h, H, W, n_faces, face_uv, &bad)) return rc;
    if (bad) return ip_fail_faces("bf_inpaint_select_faces");
    if (n_faces) HIP_TRY(hipMemcpyAsync(selected, h->sel.p, (size_t)n_faces, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BF_OK;
}

int bf_inpaint_hole_mask(bf_inpaint *h, int H, int W, const uint8_t *img, int n_faces, const float *face_uv, uint8_t *mask) {
    if (int rc = ip_check(h, 1, H, W, "bf_inpaint_hole_mask")) return rc;
    if (!img || !mask || n_faces < 0 || (n_faces && !face_uv)) return fail(BF_ERR_INVALID, "bf_inpaint_hole_mask: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->img.p, img, (size_t)H * W * 3, hipMemcpyHostToDevice, h->stream));
    bool bad = false;
    if (int rc = ip_hole_mask(h, H, W, n_faces, face_uv, &bad)) return rc;
    if (bad) return ip_fail_faces("bf_inpaint_hole_mask");
    HIP_TRY(hipMemcpyAsync(mask, h->msk.p, (size_t)H * W * 3, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BF_OK;
}

int bf_inpaint_texture(bf_inpaint *h, int H, int W, const uint8_t *img, int n_faces, const float *face_uv, uint8_t *out, uint8_t *mask) {
    if (int rc = ip_check(h, 1, H, W, "bf_inpaint_texture")) return rc;
    if (!img || !out || n_faces < 0 || (n_faces && !face_uv)) return fail(BF_ERR_INVALID, "bf_inpaint_texture: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const long long count = (long long)H * W * 3;
    HIP_TRY(hipMemcpyAsync(h->img.p, img, (size_t)count, hipMemcpyHostToDevice, s));
    bool bad = false;
    if (int rc = ip_hole_mask(h, H, W, n_faces, face_uv, &bad)) return rc;
    if (bad) return ip_fail_faces("bf_inpaint_texture");
    if (mask) HIP_TRY(hipMemcpyAsync(mask, h->msk.p, (size_t)count, hipMemcpyDeviceToHost, s));
    if (int rc = ip_run_resident(h, 1, H, W)) return rc;
    hipLaunchKernelGGL(bf_ip_quantize_kernel, dim3(ip_blocks(count)), dim3(256), 0, s, count, (const float *)h->out.p, h->q8.p, h->qm.p);
    HIP_TRY(hipGetLastError());
    if (int rc = ip_morph(s, 0, 7, 1, H, W, 3, h->q8.p, h->e8.p)) return rc;          // img2 = erode(img, 7 x 7)
    if (int rc = ip_morph(s, 0, 3, 1, H, W, 3, h->qm.p, h->em.p)) return rc;          // mask = erode(mask, 3 x 3)
    if (int rc = ip_morph(s, 1, 7, 1, H, W, 3, h->em.p, h->dm.p)) return rc;          // mask_d = dilate(mask, 7 x 7)
    hipLaunchKernelGGL(bf_ip_combine_kernel, dim3(ip_blocks(count)), dim3(256), 0, s, count, (const uint8_t *)h->q8.p,
                       (const uint8_t *)h->e8.p, (const uint8_t *)h->em.p, (const uint8_t *)h->dm.p, h->img.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->img.p, (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BF_OK;
}

int bf_morph_u8(int device, int op, int k, int n, int H, int W, int C, const uint8_t *in, uint8_t *out) {
    if ((op != 0 && op != 1) || k < 1 || k > 31 || k % 2 == 0 || n < 1 || H < 1 || W < 1 || C < 1 || C > 4 || !in || !out ||
        (long long)n * H * W * C > (1LL << 31))
        return fail(BF_ERR_INVALID, "bf_morph_u8: bad argument (op 0 / 1, odd k up to 31, 1 .. 4 channels)");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_morph_u8: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * H * W * C;
    DevBuf<uint8_t> a, b;
    HIP_TRY(a.alloc(bytes));
    HIP_TRY(b.alloc(bytes));
    HIP_TRY(hipMemcpy(a.p, in, bytes, hipMemcpyHostToDevice));
    if (int rc = ip_morph(nullptr, op, k, n, H, W, C, a.p, b.p)) return rc;
    HIP_TRY(hipMemcpy(out, b.p, bytes, hipMemcpyDeviceToHost));
    return BF_OK;
}

int bf_inpaint_selftest_conv(int device, int deconv, int n, int H, int W, int cin, int cout, const float *x, const float *xm, const float *w,
                             const float *wm, float *y, float *ym) {
    if ((deconv != 0 && deconv != 1) || n < 1 || n > 64 || H < 1 || W < 1 || H > 1024 || W > 1024 || cin < 4 || cin % 4 || cout < 1 ||
        cout > 1024 || !x || !w || !y || (xm && (deconv || !wm || !ym)) || (!deconv && (H % 2 || W % 2)))
        return fail(BF_ERR_INVALID, "bf_inpaint_selftest_conv: bad argument");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_inpaint_selftest_conv: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    IpConv c = ip_conv(n, H, W, deconv);
    const int coutp = ip_pad4(cout), K = cin * (deconv ? 4 : 16), phases = deconv ? 4 : 1;
    const size_t nx = (size_t)n * H * W * cin, nw = (size_t)phases * K * coutp, ny = (size_t)n * c.Ho * c.Wo * cout;
    DevBuf<float> dx, dxm, dw, dwm, dy, dym, part;
    HIP_TRY(dx.upload(x, nx));
    HIP_TRY(dw.upload(w, nw));
    HIP_TRY(dy.alloc(ny));
    if (xm) {
        HIP_TRY(dxm.upload(xm, nx));
        HIP_TRY(dwm.upload(wm, nw));
        HIP_TRY(dym.alloc(ny));
    }
    HIP_TRY(part.alloc(IP_PART_PER_IMAGE * n));
    c.x = dx.p; c.ldx = cin; c.xm = xm ? dxm.p : nullptr; c.ldxm = cin; c.w = dw.p; c.wm = xm ? dwm.p : nullptr;
    c.cin = cin; c.cout = cout; c.coutp = coutp; c.epi = IP_EPI_RAW;
    c.y0 = dy.p; c.ld0 = cout; c.y1 = xm ? dym.p : nullptr; c.ld1 = cout;
    if (int rc = ip_launch(nullptr, c, part.p, part.n)) return rc;
    HIP_TRY(hipMemcpy(y, dy.p, ny * sizeof(float), hipMemcpyDeviceToHost));
    if (xm) HIP_TRY(hipMemcpy(ym, dym.p, ny * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
