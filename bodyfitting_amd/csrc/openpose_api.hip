// Host side of the OpenPose body estimator (reference openpose/body.py Body.__call__, openpose/model.py bodypose_model): the layer
// list, the resident weights, the buffers (grown to the largest call) and the launch sequence.  Kernels: openpose_kernels.hip.
#include "openpose_host.h"

#include <cmath>

#define OP_NPAF 38
#define OP_NHEAT 19
#define OP_NOUT 57
#define OP_NPART 18
#define OP_CAT 192                     // the stage input: out1 0:128 | L1 128:166 | 0 0 | L2 168:187 | 0 x 5
#define OP_NSCALE 4


namespace {
const double SCALE_SEARCH[OP_NSCALE] = {0.5, 1.0, 1.5, 2.0};     // body.py:61

// The order bodyfitting_amd/openpose.py pack() writes: the VGG front (conv1_1 .. conv4_4_CPM); conv5_1_CPM L1 | L2 as one 128 -> 256
// layer; conv5_2 .. conv5_5 each L1 then L2; per stage 2 .. 6: Mconv1 L1 | L2 as one 192 -> 256 layer on the padded concat, then
// Mconv2 .. Mconv7 each L1 then L2.
std::vector<OpLayer> op_layers(size_t *total) {
    std::vector<OpLayer> L;
    size_t at = 0;
    auto add = [&](int cin, int cout, int k) { op_add_layer(L, &at, cin, cout, k); };
    const int vgg[12][2] = {{3, 64}, {64, 64}, {64, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 512},
                            {512, 512}, {512, 256}, {256, 128}};
    for (int i = 0; i < 12; ++i) add(vgg[i][0], vgg[i][1], 3);
    add(128, 256, 3);
    for (int br = 0; br < 2; ++br) add(128, 128, 3);
    for (int br = 0; br < 2; ++br) add(128, 128, 3);
    for (int br = 0; br < 2; ++br) add(128, 512, 1);
    add(512, OP_NPAF, 1);
    add(512, OP_NHEAT, 1);
    for (int s = 2; s <= 6; ++s) {
        add(OP_CAT, 256, 7);
        for (int j = 2; j <= 5; ++j)
            for (int br = 0; br < 2; ++br) add(128, 128, 7);
        for (int br = 0; br < 2; ++br) add(128, 128, 1);
        add(128, OP_NPAF, 1);
        add(128, OP_NHEAT, 1);
    }
    *total = at;
    return L;
}

struct ScaleDims { double s; int h, w, Hp, Wp, hq, wq; };
ScaleDims scale_dims(int H, int W, int m) {
    ScaleDims d;
    d.s = SCALE_SEARCH[m] * 368 / H;                              // body.py:67, Python's evaluation order
    d.h = (int)std::rint((double)H * d.s);                         // saturate_cast<int>: round half to even
    d.w = (int)std::rint((double)W * d.s);
    d.Hp = (d.h + 7) / 8 * 8; d.Wp = (d.w + 7) / 8 * 8;
    d.hq = d.Hp / 8; d.wq = d.Wp / 8;
    return d;
}

}  // namespace

struct bf_openpose {
    int device = 0, max_batch = 0, max_h = 0, max_w = 0;
    hipStream_t stream = nullptr;
    std::vector<OpLayer> layers;
    DevBuf<float> w, inp, act[2], cat, br[2], out;
    DevBuf<uint8_t> img;
    DevBuf<double> heat, paf, tmp, bl, scores, jscore;
    DevBuf<int> counts, peaks, jobs, jcnt;
    int map_n = 0, map_h = 0, map_w = 0;                          // the resident maps (0: none)
};

// the buffers of an n x H x W call
static int op_reserve(bf_openpose *op, int n, int H, int W) {
    size_t act = 0, cat = 0, out = 0;
    for (int m = 0; m < OP_NSCALE; ++m) {
        const ScaleDims d = scale_dims(H, W, m);
        const size_t px = (size_t)n * d.Hp * d.Wp, q = (size_t)n * d.hq * d.wq;
        if (d.h < 1 || d.w < 1 || px * 64 > ((size_t)1 << 31)) return fail(BF_ERR_UNSUPPORTED, "bf_openpose: image size outside what the kernels index");
        act = std::max(act, px * 64);
        cat = std::max(cat, q * OP_CAT);
        out = std::max(out, q * OP_NOUT);
    }
    const size_t pix = (size_t)n * H * W;
    hipStream_t s = op->stream;
    HIP_TRY(bf_grow(s, op->img, pix * 3));
    HIP_TRY(bf_grow(s, op->inp, act / 16));
    for (int i = 0; i < 2; ++i) HIP_TRY(bf_grow(s, op->act[i], act));
    HIP_TRY(bf_grow(s, op->cat, cat));
    for (int i = 0; i < 2; ++i) HIP_TRY(bf_grow(s, op->br[i], cat / OP_CAT * 1024));
    HIP_TRY(bf_grow(s, op->out, out));
    HIP_TRY(bf_grow(s, op->heat, pix * OP_NHEAT));
    HIP_TRY(bf_grow(s, op->paf, pix * OP_NPAF));
    HIP_TRY(bf_grow(s, op->tmp, pix * OP_NPART));
    HIP_TRY(bf_grow(s, op->bl, pix * OP_NPART));
    HIP_TRY(bf_grow(s, op->counts, (size_t)n));
    return BF_OK;
}

static int op_check(bf_openpose *op, int n, int H, int W, const void *p, const char *what) {
    if (!op) return fail(BF_ERR_INVALID, std::string(what) + ": no handle");
    if (n < 1 || n > op->max_batch) return fail(BF_ERR_INVALID, std::string(what) + ": batch outside 1 .. max_batch");
    if (H < 13 || W < 13 || H > op->max_h || W > op->max_w)
        return fail(BF_ERR_INVALID, std::string(what) + ": image " + std::to_string(H) + " x " + std::to_string(W) + " outside 13 .. max_h x 13 .. max_w (" +
                                        std::to_string(op->max_h) + " x " + std::to_string(op->max_w) + ")");
    if (!p) return fail(BF_ERR_INVALID, std::string(what) + ": no input");
    return BF_OK;
}

// model.py:111-124 on op->inp (n x Hp x Wp x 4) -> op->out (n x hq x wq x 57: Mconv7_stage6_L1 0:38, Mconv7_stage6_L2 38:57)
static int op_network(bf_openpose *op, int n, int Hp, int Wp) {
    hipStream_t s = op->stream;
    const float *Wt = op->w.p;
    const std::vector<OpLayer> &L = op->layers;
    float *A = op->act[0].p, *B = op->act[1].p;
    int H = Hp, W = Wp;
    // the VGG front: conv1_1 .. conv4_4_CPM, 2 x 2 pools after conv1_2, conv2_2 and conv3_4; conv4_4_CPM writes out1 into the concat
    const int pool_after[3] = {1, 3, 7};
    const float *x = op->inp.p;
    int cin = 4, pi = 0;
    HIP_TRY(hipMemsetAsync(op->cat.p, 0, (size_t)n * (Hp / 8) * (Wp / 8) * OP_CAT * sizeof(float), s));
    for (int i = 0; i < 12; ++i) {
        const bool last = i == 11;
        float *y = last ? op->cat.p : (x == A ? B : A);
        if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[i], x, cin, y, last ? OP_CAT : L[i].cout, 1))) return rc;
        x = y; cin = L[i].cout;
        if (pi < 3 && i == pool_after[pi]) {
            float *z = x == A ? B : A;
            hipLaunchKernelGGL(bf_op_pool_kernel, dim3(op_blocks((long long)n * (H / 2) * (W / 2) * (cin / 4))), dim3(256), 0, s, n, H, W, cin,
                               (const float4 *)x, (float4 *)z);
            HIP_TRY(hipGetLastError());
            x = z; H /= 2; W /= 2; ++pi;
        }
    }
    float *P = op->br[0].p, *Q = op->br[1].p, *cat = op->cat.p;
    size_t li = 12;
    // stage 1: conv5_1 L1 | L2 on out1, then the branches two by two
    if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], cat, OP_CAT, P, 256, 1))) return rc;
    for (int j = 0; j < 2; ++j, li += 2) {
        const OpConv a = conv_of(Wt, L[li], P, 256, Q, 256, 1), b = conv_of(Wt, L[li + 1], P + 128, 256, Q + 128, 256, 1);
        if (int rc = launch_conv(s, n, H, W, a, &b)) return rc;
        std::swap(P, Q);
    }
    {
        const OpConv a = conv_of(Wt, L[li], P, 256, Q, 1024, 1), b = conv_of(Wt, L[li + 1], P + 128, 256, Q + 512, 1024, 1);
        if (int rc = launch_conv(s, n, H, W, a, &b)) return rc;
        li += 2;
        const OpConv c = conv_of(Wt, L[li], Q, 1024, cat + 128, OP_CAT, 0), d = conv_of(Wt, L[li + 1], Q + 512, 1024, cat + 168, OP_CAT, 0);
        if (int rc = launch_conv(s, n, H, W, c, &d)) return rc;
        li += 2;
    }
    for (int st = 2; st <= 6; ++st) {
        if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], cat, OP_CAT, P, 256, 1))) return rc;
        for (int j = 2; j <= 6; ++j, li += 2) {
            const OpConv a = conv_of(Wt, L[li], P, 256, Q, 256, 1), b = conv_of(Wt, L[li + 1], P + 128, 256, Q + 128, 256, 1);
            if (int rc = launch_conv(s, n, H, W, a, &b)) return rc;
            std::swap(P, Q);
        }
        // Mconv7: into the next stage's concat, or - stage 6 - the output; model.py:29-32 lists Mconv7_stage6_L1 twice among the
        // layers without ReLU and never Mconv7_stage6_L2, so the final heatmaps go through a ReLU
        const bool fin = st == 6;
        float *y = fin ? op->out.p : cat;
        const int ldo = fin ? OP_NOUT : OP_CAT;
        const OpConv a = conv_of(Wt, L[li], P, 256, y + (fin ? 0 : 128), ldo, 0);
        const OpConv b = conv_of(Wt, L[li + 1], P + 128, 256, y + (fin ? OP_NPAF : 168), ldo, fin ? 1 : 0);
        if (int rc = launch_conv(s, n, H, W, a, &b)) return rc;
        li += 2;
    }
    return BF_OK;
}

// one scale of body.py:70-102: (network on the resized image, or the injected output) -> heat / paf accumulation.
// in_host / out_host (may be NULL) receive the network input [n][Hp][Wp][4] / output [n][hq][wq][57]
static int op_scale(bf_openpose *op, int n, int H, int W, int m, const float *injected, float *in_host, float *out_host) {
    hipStream_t s = op->stream;
    const ScaleDims d = scale_dims(H, W, m);
    const size_t q = (size_t)n * d.hq * d.wq * OP_NOUT;
    if (injected) {
        HIP_TRY(hipMemcpyAsync(op->out.p, injected, q * sizeof(float), hipMemcpyHostToDevice, s));
    } else {
        const long long px = (long long)n * d.Hp * d.Wp;
        hipLaunchKernelGGL(bf_op_input_kernel, dim3(op_blocks(px)), dim3(256), 0, s, n, H, W, d.h, d.w, d.Hp, d.Wp, 1.0 / d.s,
                           (const uint8_t *)op->img.p, (float4 *)op->inp.p);
        HIP_TRY(hipGetLastError());
        if (in_host) HIP_TRY(hipMemcpyAsync(in_host, op->inp.p, (size_t)px * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (int rc = op_network(op, n, d.Hp, d.Wp)) return rc;
        if (out_host) HIP_TRY(hipMemcpyAsync(out_host, op->out.p, q * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    float *up = op->act[0].p;                                    // n x h x w x 57 <= n x Hp x Wp x 64
    hipLaunchKernelGGL(bf_op_up8_kernel, dim3(op_blocks((long long)n * d.h * d.w * OP_NOUT)), dim3(256), 0, s, n, d.h, d.w, d.hq, d.wq,
                       (const float *)op->out.p, up);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bf_op_maps_kernel, dim3(op_blocks((long long)n * H * W * OP_NOUT)), dim3(256), 0, s, n, H, W, d.h, d.w,
                       1.0 / ((double)H / d.h), 1.0 / ((double)W / d.w), (const float *)up, op->heat.p, op->paf.p);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

static int op_run(bf_openpose *op, int n, int H, int W, const uint8_t *bgr, const float *injected, float *in_host, float *out_host,
                  double *heat, double *paf) {
    HIP_TRY(hipSetDevice(op->device));
    if (int rc = op_reserve(op, n, H, W)) return rc;
    hipStream_t s = op->stream;
    const size_t pix = (size_t)n * H * W;
    op->map_n = 0;
    if (bgr) HIP_TRY(hipMemcpyAsync(op->img.p, bgr, pix * 3, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(op->heat.p, 0, pix * OP_NHEAT * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(op->paf.p, 0, pix * OP_NPAF * sizeof(double), s));
    size_t in_at = 0, out_at = 0;
    for (int m = 0; m < OP_NSCALE; ++m) {
        const ScaleDims d = scale_dims(H, W, m);
        const size_t q = (size_t)n * d.hq * d.wq * OP_NOUT;
        if (int rc = op_scale(op, n, H, W, m, injected ? injected + out_at : nullptr, in_host ? in_host + in_at : nullptr,
                              out_host ? out_host + out_at : nullptr)) return rc;
        in_at += (size_t)n * d.Hp * d.Wp * 4;
        out_at += q;
    }
    if (heat) HIP_TRY(hipMemcpyAsync(heat, op->heat.p, pix * OP_NHEAT * sizeof(double), hipMemcpyDeviceToHost, s));
    if (paf) HIP_TRY(hipMemcpyAsync(paf, op->paf.p, pix * OP_NPAF * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    op->map_n = n; op->map_h = H; op->map_w = W;
    return BF_OK;
}

static size_t op_output_floats(int n, int H, int W) {
    size_t t = 0;
    for (int m = 0; m < OP_NSCALE; ++m) { const ScaleDims d = scale_dims(H, W, m); t += (size_t)n * d.hq * d.wq * OP_NOUT; }
    return t;
}

extern "C" {

int64_t bf_openpose_n_weights(void) {
    size_t total = 0;
    op_layers(&total);
    return (int64_t)total;
}

void bf_openpose_destroy(bf_openpose *op) {
    if (!op) return;
    (void)hipSetDevice(op->device);
    if (op->stream) { (void)hipStreamSynchronize(op->stream); (void)hipStreamDestroy(op->stream); }
    delete op;
}

int bf_openpose_create(int device, const float *weights, int64_t n_weights, int max_batch, int max_h, int max_w, bf_openpose **out) {
    if (!out || !weights || max_batch < 1 || max_batch > 1024 || max_h < 13 || max_w < 13 || max_h > 8192 || max_w > 8192)
        return fail(BF_ERR_INVALID, "bf_openpose_create: bad argument");
    *out = nullptr;
    size_t total = 0;
    std::vector<OpLayer> layers = op_layers(&total);
    if (n_weights != (int64_t)total)
        return fail(BF_ERR_INVALID, "bf_openpose_create: " + std::to_string(n_weights) + " packed weights, the network has " + std::to_string(total));
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_openpose_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto *op = new bf_openpose();
    op->device = device; op->max_batch = max_batch; op->max_h = max_h; op->max_w = max_w; op->layers = std::move(layers);
    const bool ok = hipStreamCreateWithFlags(&op->stream, hipStreamNonBlocking) == hipSuccess &&
                    op->w.upload(weights, total) == hipSuccess;
    if (!ok) { bf_openpose_destroy(op); return fail(BF_ERR_HIP, "bf_openpose_create: device allocation failed"); }
    *out = op;
    return BF_OK;
}

int bf_openpose_maps(bf_openpose *op, int n, int H, int W, const uint8_t *bgr, double *heat, double *paf) {
    if (int rc = op_check(op, n, H, W, bgr, "bf_openpose_maps")) return rc;
    return op_run(op, n, H, W, bgr, nullptr, nullptr, nullptr, heat, paf);
}

int bf_openpose_network(bf_openpose *op, int n, int H, int W, const uint8_t *bgr, float *inputs, float *outputs) {
    if (int rc = op_check(op, n, H, W, bgr, "bf_openpose_network")) return rc;
    if (!outputs) return fail(BF_ERR_INVALID, "bf_openpose_network: no output array");
    return op_run(op, n, H, W, bgr, nullptr, inputs, outputs, nullptr, nullptr);
}

int bf_openpose_inject(bf_openpose *op, int n, int H, int W, const float *outputs, int64_t n_outputs, double *heat, double *paf) {
    if (int rc = op_check(op, n, H, W, outputs, "bf_openpose_inject")) return rc;
    if (n_outputs != (int64_t)op_output_floats(n, H, W))
        return fail(BF_ERR_INVALID, "bf_openpose_inject: " + std::to_string(n_outputs) + " floats, the four scales need " +
                                        std::to_string(op_output_floats(n, H, W)));
    return op_run(op, n, H, W, nullptr, outputs, nullptr, nullptr, heat, paf);
}

int bf_openpose_map_size(bf_openpose *op, int *hw) {
    if (!op || !hw) return fail(BF_ERR_INVALID, "bf_openpose_map_size: bad argument");
    hw[0] = op->map_h; hw[1] = op->map_w;
    return BF_OK;
}

int bf_openpose_peaks(bf_openpose *op, int n, int cap, double *blurred, int *counts, int *peaks, double *scores) {
    if (!op || !counts || !peaks || !scores || cap < 1) return fail(BF_ERR_INVALID, "bf_openpose_peaks: bad argument");
    if (op->map_n < 1 || n < 1 || n > op->map_n) return fail(BF_ERR_INVALID, "bf_openpose_peaks: no resident maps for that many views");
    HIP_TRY(hipSetDevice(op->device));
    hipStream_t s = op->stream;
    const int H = op->map_h, W = op->map_w;
    HIP_TRY(bf_grow(s, op->peaks, (size_t)n * cap * 3));
    HIP_TRY(bf_grow(s, op->scores, (size_t)n * cap));
    const long long total = (long long)n * H * W * OP_NPART;
    hipLaunchKernelGGL(bf_op_gauss_kernel, dim3(op_blocks(total)), dim3(256), 0, s, n, H, W, 0, OP_NHEAT, (const double *)op->heat.p, op->tmp.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bf_op_gauss_kernel, dim3(op_blocks(total)), dim3(256), 0, s, n, H, W, 1, OP_NPART, (const double *)op->tmp.p, op->bl.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(op->counts.p, 0, (size_t)n * sizeof(int), s));
    hipLaunchKernelGGL(bf_op_peaks_kernel, dim3(op_blocks(total)), dim3(256), 0, s, n, H, W, (const double *)op->bl.p, (const double *)op->heat.p,
                       cap, op->counts.p, op->peaks.p, op->scores.p);
    HIP_TRY(hipGetLastError());
    if (blurred) HIP_TRY(hipMemcpyAsync(blurred, op->bl.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(counts, op->counts.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(peaks, op->peaks.p, (size_t)n * cap * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(scores, op->scores.p, (size_t)n * cap * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < n; ++b)
        if (counts[b] > cap) return fail(BF_ERR_UNSUPPORTED, "bf_openpose_peaks: view " + std::to_string(b) + " has " + std::to_string(counts[b]) +
                                                                 " peaks, more than the list holds (" + std::to_string(cap) + ")");
    return BF_OK;
}

int bf_openpose_pairs(bf_openpose *op, int view, int npairs, const int *jobs, double *score, int *above) {
    if (!op || !jobs || !score || !above || npairs < 1) return fail(BF_ERR_INVALID, "bf_openpose_pairs: bad argument");
    if (view < 0 || view >= op->map_n) return fail(BF_ERR_INVALID, "bf_openpose_pairs: no resident maps for that view");
    const int H = op->map_h, W = op->map_w;
    for (int i = 0; i < npairs; ++i) {
        const int *j = jobs + 5 * i;
        if (j[0] < 0 || j[0] >= 19 || j[1] < 0 || j[1] >= W || j[2] < 0 || j[2] >= H || j[3] < 0 || j[3] >= W || j[4] < 0 || j[4] >= H)
            return fail(BF_ERR_INVALID, "bf_openpose_pairs: job " + std::to_string(i) + " outside the maps");
    }
    HIP_TRY(hipSetDevice(op->device));
    hipStream_t s = op->stream;
    HIP_TRY(bf_grow(s, op->jobs, (size_t)npairs * 5));
    HIP_TRY(bf_grow(s, op->jscore, (size_t)npairs));
    HIP_TRY(bf_grow(s, op->jcnt, (size_t)npairs));
    HIP_TRY(hipMemcpyAsync(op->jobs.p, jobs, (size_t)npairs * 5 * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(bf_op_pairs_kernel, dim3((npairs + 63) / 64), dim3(64), 0, s, npairs, H, W,
                       (const double *)(op->paf.p + (size_t)view * H * W * OP_NPAF), (const int *)op->jobs.p, op->jscore.p, op->jcnt.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(score, op->jscore.p, (size_t)npairs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(above, op->jcnt.p, (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BF_OK;
}

int bf_openpose_selftest_conv(int device, int n, int H, int W, int cin, int cout, int k, int relu, const float *x, const float *w,
                              const float *bias, float *y) {
    if (n < 1 || H < 1 || W < 1 || cin < 1 || cout < 1 || cout > 1024 || (k != 1 && k != 3 && k != 7) || !x || !w || !bias || !y)
        return fail(BF_ERR_INVALID, "bf_openpose_selftest_conv: bad argument (k is 1, 3 or 7)");
    if ((long long)n * H * W * std::max(cin + 3, cout) >= (1LL << 31)) return fail(BF_ERR_UNSUPPORTED, "bf_openpose_selftest_conv: too large");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_openpose_selftest_conv: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const int cp = (cin + 3) / 4 * 4, co = (cout + 3) / 4 * 4;
    const size_t px = (size_t)n * H * W;
    std::vector<float> xp(px * cp, 0.f), packed((size_t)k * k * cp * co + co, 0.f);
    for (size_t i = 0; i < px; ++i) std::memcpy(&xp[i * cp], x + i * cin, cin * sizeof(float));
    for (int t = 0; t < k * k; ++t)
        for (int c = 0; c < cin; ++c) std::memcpy(&packed[((size_t)t * cp + c) * co], w + ((size_t)t * cin + c) * cout, cout * sizeof(float));
    std::memcpy(&packed[(size_t)k * k * cp * co], bias, cout * sizeof(float));
    DevBuf<float> dx, dw, dy;
    HIP_TRY(dx.upload(xp));
    HIP_TRY(dw.upload(packed));
    HIP_TRY(dy.alloc(px * cout));
    OpLayer l{0, (size_t)k * k * cp * co, cp, cout, co, k};
    if (int rc = launch_conv(nullptr, n, H, W, conv_of(dw.p, l, dx.p, cp, dy.p, cout, relu))) return rc;
    HIP_TRY(hipMemcpy(y, dy.p, px * cout * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
