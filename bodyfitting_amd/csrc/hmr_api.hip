// Host side of the HMR forward pass (reference models/hmr.py: ResNet-50 v1.5 + the iterative regressor, in eval()): the network's
// layer list, the resident weights, the activation buffers for max_batch images and the launch sequence.  Kernels: hmr_kernels.hip.
#include "bf_host.h"
#include "hmr_kernels.h"

#define HMR_RES 224
#define HMR_FEAT 2048
#define HMR_NSTATE 157
#define HMR_XC (HMR_FEAT + HMR_NSTATE)
#define HMR_HIDDEN 1024
#define HMR_ITERS 3                        // HMR.forward's n_iter (hmr.py:140)

namespace {
struct HmrLayer { size_t w, b; int cin, cout, k, stride, pad; };     // offsets of the packed [K][Cout] weight and the bias

// The packing order bodyfitting_amd/hmr.py writes: conv1; then per Bottleneck conv1, conv2, conv3 and - first block of a layer -
// downsample.0; then fc1, fc2 and decpose | decshape | deccam as one 1024 -> 157 layer.  Each: weight [K][Cout] with K in
// (ky, kx, ci) order, then the bias [Cout] (BatchNorm folded in).
std::vector<HmrLayer> hmr_layers(size_t *total) {
    std::vector<HmrLayer> L;
    size_t at = 0;
    auto add = [&](int cin, int cout, int k, int stride, int pad) {
        HmrLayer l{at, at + (size_t)cin * k * k * cout, cin, cout, k, stride, pad};
        at = l.b + cout;
        L.push_back(l);
    };
    add(3, 64, 7, 2, 3);
    const int blocks[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512}, strides[4] = {1, 2, 2, 2};
    int inplanes = 64;
    for (int li = 0; li < 4; ++li)
        for (int bi = 0; bi < blocks[li]; ++bi) {
            const int p = planes[li], s = bi == 0 ? strides[li] : 1;
            add(inplanes, p, 1, 1, 0);
            add(p, p, 3, s, 1);                    // the stride is on the 3 x 3 (Bottleneck.conv2, ResNet v1.5)
            add(p, 4 * p, 1, 1, 0);
            if (bi == 0) add(inplanes, 4 * p, 1, s, 0);
            inplanes = 4 * p;
        }
    add(HMR_XC, HMR_HIDDEN, 1, 1, 0);
    add(HMR_HIDDEN, HMR_HIDDEN, 1, 1, 0);
    add(HMR_HIDDEN, HMR_NSTATE, 1, 1, 0);
    *total = at;
    return L;
}

int launch_conv(hipStream_t s, const float *wts, const HmrLayer &l, int n, int H, int W, const float *x, const float *res, int relu,
                float *y, int ldo, int *Ho_out = nullptr, int *Wo_out = nullptr) {
    HmrConv p;
    p.x = x; p.w = wts + l.w; p.bias = wts + l.b; p.res = res; p.y = y;
    p.n = n; p.H = H; p.W = W; p.Cin = l.cin; p.Cout = l.cout; p.kh = p.kw = l.k; p.stride = l.stride; p.pad = l.pad;
    p.Ho = (H + 2 * l.pad - l.k) / l.stride + 1; p.Wo = (W + 2 * l.pad - l.k) / l.stride + 1;
    p.ldo = ldo; p.relu = relu;
    const long long M = (long long)n * p.Ho * p.Wo;
    hipLaunchKernelGGL(bf_hmr_conv_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((l.cout + 63) / 64)), dim3(256), 0, s, p);
    if (Ho_out) *Ho_out = p.Ho;
    if (Wo_out) *Wo_out = p.Wo;
    HIP_TRY(hipGetLastError());
    return BF_OK;
}
}  // namespace

struct bf_hmr {
    int device = 0, max_batch = 0;
    hipStream_t stream = nullptr;
    std::vector<HmrLayer> layers;
    DevBuf<float> w, mean, input, act[4], xc, h1, h2;
    DevBuf<uint8_t> img, resized;
};

static const size_t HMR_ACT = (size_t)112 * 112 * 64;    // floats per image of the largest activation (= 56 x 56 x 256)

// images [n][H][W][3] uint8 -> h->input (normalised NHWC 224 x 224 x 3); resized (host, may be NULL) receives the uint8 image
static int hmr_preprocess(bf_hmr *h, int n, int H, int W, const uint8_t *images, uint8_t *resized) {
    if (n < 1 || n > h->max_batch || H < 1 || W < 1 || !images) return fail(BF_ERR_INVALID, "bf_hmr: bad image batch (1 <= n <= max_batch, H, W >= 1)");
    const size_t bytes = (size_t)n * H * W * 3;
    if (h->img.n < bytes) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->img.release();
        HIP_TRY(h->img.alloc(bytes));
    }
    HIP_TRY(hipMemcpyAsync(h->img.p, images, bytes, hipMemcpyHostToDevice, h->stream));
    const int total = n * HMR_RES * HMR_RES;
    // constants.IMG_NORM_MEAN / IMG_NORM_STD as the float32 tensors transforms.Normalize builds from them
    hipLaunchKernelGGL(bf_hmr_resize_kernel, dim3((total + 255) / 256), dim3(256), 0, h->stream, n, H, W, (double)H / HMR_RES,
                       (double)W / HMR_RES, (const uint8_t *)h->img.p, resized ? h->resized.p : (uint8_t *)nullptr, h->input.p,
                       make_float3(0.485f, 0.456f, 0.406f), make_float3(0.229f, 0.224f, 0.225f));
    HIP_TRY(hipGetLastError());
    if (resized) HIP_TRY(hipMemcpyAsync(resized, h->resized.p, (size_t)total * 3, hipMemcpyDeviceToHost, h->stream));
    return BF_OK;
}

// the backbone on h->input -> h->xc[b][0:2048] (avgpool of layer 4)
static int hmr_backbone(bf_hmr *h, int n) {
    hipStream_t s = h->stream;
    const float *W = h->w.p;
    const std::vector<HmrLayer> &L = h->layers;
    int Hc = 0, Wc = 0;
    float *A[4] = {h->act[0].p, h->act[1].p, h->act[2].p, h->act[3].p};
    if (int rc = launch_conv(s, W, L[0], n, HMR_RES, HMR_RES, h->input.p, nullptr, 1, A[1], L[0].cout, &Hc, &Wc)) return rc;
    const int Hp = (Hc + 2 - 3) / 2 + 1, Wp = (Wc + 2 - 3) / 2 + 1;
    const size_t np = (size_t)n * Hp * Wp * 64;
    hipLaunchKernelGGL(bf_hmr_maxpool_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, n, Hc, Wc, 64, Hp, Wp, (const float *)A[1], A[0]);
    HIP_TRY(hipGetLastError());
    Hc = Hp; Wc = Wp;
    // A[0] holds the block input x; A[1] conv1, A[2] conv2, A[3] the downsampled residual; the block output goes to A[1], which
    // then becomes the next block's x
    size_t li = 1;
    const int blocks[4] = {3, 4, 6, 3};
    for (int g = 0; g < 4; ++g)
        for (int bi = 0; bi < blocks[g]; ++bi) {
            const HmrLayer &c1 = L[li], &c2 = L[li + 1], &c3 = L[li + 2];
            int H2 = 0, W2 = 0;
            if (int rc = launch_conv(s, W, c1, n, Hc, Wc, A[0], nullptr, 1, A[1], c1.cout)) return rc;
            if (int rc = launch_conv(s, W, c2, n, Hc, Wc, A[1], nullptr, 1, A[2], c2.cout, &H2, &W2)) return rc;
            const float *res = A[0];
            if (bi == 0) {
                const HmrLayer &ds = L[li + 3];
                if (int rc = launch_conv(s, W, ds, n, Hc, Wc, A[0], nullptr, 0, A[3], ds.cout)) return rc;
                res = A[3];
            }
            if (int rc = launch_conv(s, W, c3, n, H2, W2, A[2], res, 1, A[1], c3.cout)) return rc;
            std::swap(A[0], A[1]);
            li += bi == 0 ? 4 : 3;
            Hc = H2; Wc = W2;
        }
    if (Hc != 7 || Wc != 7) return fail(BF_ERR_INVALID, "bf_hmr: layer 4 is not 7 x 7");
    hipLaunchKernelGGL(bf_hmr_avgpool_kernel, dim3((n * HMR_FEAT + 255) / 256), dim3(256), 0, s, n, (const float *)A[0], h->xc.p);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// HMR.forward's loop (hmr.py:140-149; dropout is the identity in eval): state += dec(fc2(fc1([xf, state]))), three times
static int hmr_regressor(bf_hmr *h, int n) {
    hipStream_t s = h->stream;
    const size_t nl = h->layers.size();
    const HmrLayer &fc1 = h->layers[nl - 3], &fc2 = h->layers[nl - 2], &dec = h->layers[nl - 1];
    hipLaunchKernelGGL(bf_hmr_init_state_kernel, dim3((n * HMR_NSTATE + 255) / 256), dim3(256), 0, s, n, (const float *)h->mean.p, h->xc.p);
    HIP_TRY(hipGetLastError());
    float *state = h->xc.p + HMR_FEAT;
    for (int it = 0; it < HMR_ITERS; ++it) {
        if (int rc = launch_conv(s, h->w.p, fc1, n, 1, 1, h->xc.p, nullptr, 0, h->h1.p, HMR_HIDDEN)) return rc;
        if (int rc = launch_conv(s, h->w.p, fc2, n, 1, 1, h->h1.p, nullptr, 0, h->h2.p, HMR_HIDDEN)) return rc;
        if (int rc = launch_conv(s, h->w.p, dec, n, 1, 1, h->h2.p, state, 0, state, HMR_XC)) return rc;
    }
    return BF_OK;
}

extern "C" {

int64_t bf_hmr_n_weights(void) {
    size_t total = 0;
    hmr_layers(&total);
    return (int64_t)total;
}

void bf_hmr_destroy(bf_hmr *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    delete h;
}

int bf_hmr_create(int device, const float *weights, int64_t n_weights, const float *mean_params, int max_batch, bf_hmr **out) {
    if (!out || !weights || !mean_params || max_batch < 1 || max_batch > 4096) return fail(BF_ERR_INVALID, "bf_hmr_create: bad argument");
    *out = nullptr;
    size_t total = 0;
    std::vector<HmrLayer> layers = hmr_layers(&total);
    if (n_weights != (int64_t)total)
        return fail(BF_ERR_INVALID, "bf_hmr_create: " + std::to_string(n_weights) + " packed weights, the network has " + std::to_string(total));
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_hmr_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto *h = new bf_hmr();
    h->device = device; h->max_batch = max_batch; h->layers = std::move(layers);
    const size_t mb = (size_t)max_batch;
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              h->w.upload(weights, total) == hipSuccess &&
              h->mean.upload(mean_params, HMR_NSTATE) == hipSuccess &&
              h->input.alloc(mb * HMR_RES * HMR_RES * 3) == hipSuccess && h->resized.alloc(mb * HMR_RES * HMR_RES * 3) == hipSuccess &&
              h->xc.alloc(mb * HMR_XC) == hipSuccess && h->h1.alloc(mb * HMR_HIDDEN) == hipSuccess && h->h2.alloc(mb * HMR_HIDDEN) == hipSuccess;
    for (int i = 0; i < 4 && ok; ++i) ok = h->act[i].alloc(mb * HMR_ACT) == hipSuccess;
    if (!ok) { bf_hmr_destroy(h); return fail(BF_ERR_HIP, "bf_hmr_create: device allocation failed"); }
    *out = h;
    return BF_OK;
}

int bf_hmr_preprocess(bf_hmr *h, int n, int H, int W, const uint8_t *images, uint8_t *resized, float *normalized) {
    if (!h) return fail(BF_ERR_INVALID, "bf_hmr_preprocess: no handle");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = hmr_preprocess(h, n, H, W, images, resized)) return rc;
    if (normalized) HIP_TRY(hipMemcpyAsync(normalized, h->input.p, (size_t)n * HMR_RES * HMR_RES * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BF_OK;
}

int bf_hmr_features(bf_hmr *h, int n, int H, int W, const uint8_t *images, float *xf) {
    if (!h || !xf) return fail(BF_ERR_INVALID, "bf_hmr_features: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = hmr_preprocess(h, n, H, W, images, nullptr)) return rc;
    if (int rc = hmr_backbone(h, n)) return rc;
    HIP_TRY(hipMemcpy2DAsync(xf, HMR_FEAT * sizeof(float), h->xc.p, HMR_XC * sizeof(float), HMR_FEAT * sizeof(float), n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BF_OK;
}

int bf_hmr_predict(bf_hmr *h, int n, int H, int W, const uint8_t *images, float *pose6d, float *betas, float *cam) {
    if (!h || !pose6d || !betas || !cam) return fail(BF_ERR_INVALID, "bf_hmr_predict: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = hmr_preprocess(h, n, H, W, images, nullptr)) return rc;
    if (int rc = hmr_backbone(h, n)) return rc;
    if (int rc = hmr_regressor(h, n)) return rc;
    const size_t row = HMR_XC * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(pose6d, 144 * sizeof(float), h->xc.p + HMR_FEAT, row, 144 * sizeof(float), n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpy2DAsync(betas, 10 * sizeof(float), h->xc.p + HMR_FEAT + 144, row, 10 * sizeof(float), n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpy2DAsync(cam, 3 * sizeof(float), h->xc.p + HMR_FEAT + 154, row, 3 * sizeof(float), n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BF_OK;
}

int bf_hmr_selftest_conv(int device, int n, int H, int W, int cin, int cout, int k, int stride, int pad, const float *x, const float *w,
                         const float *bias, const float *res, int relu, float *y) {
    if (n < 1 || H < 1 || W < 1 || cin < 1 || cout < 1 || k < 1 || stride < 1 || pad < 0 || !x || !w || !bias || !y)
        return fail(BF_ERR_INVALID, "bf_hmr_selftest_conv: bad argument");
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    if (Ho < 1 || Wo < 1) return fail(BF_ERR_INVALID, "bf_hmr_selftest_conv: empty output");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_hmr_selftest_conv: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const size_t nx = (size_t)n * H * W * cin, nw = (size_t)k * k * cin * cout, ny = (size_t)n * Ho * Wo * cout;
    std::vector<float> packed(nw + cout);
    std::memcpy(packed.data(), w, nw * sizeof(float));
    std::memcpy(packed.data() + nw, bias, cout * sizeof(float));
    DevBuf<float> dx, dw, dr, dy;
    HIP_TRY(dx.upload(x, nx));
    HIP_TRY(dw.upload(packed));
    if (res) HIP_TRY(dr.upload(res, ny));
    HIP_TRY(dy.alloc(ny));
    HmrLayer l{0, nw, cin, cout, k, stride, pad};
    if (int rc = launch_conv(nullptr, dw.p, l, n, H, W, dx.p, res ? dr.p : nullptr, relu, dy.p, cout)) return rc;
    HIP_TRY(hipMemcpy(y, dy.p, ny * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
