// Host side of the OpenPose hand estimator (reference openpose/hand.py Hand.__call__, openpose/model.py handpose_model): the layer
// list, the resident weights, the buffers (grown to the largest call), the per-scale batching of crops and the launch sequence.
// Kernels: openpose_hand_kernels.hip, and the body estimator's convolution and pool kernels (openpose_kernels.hip).
#include "openpose_host.h"
#include "openpose_hand.h"

#include <cmath>

#define OH_CAT 152                    // the stage input: out_prev 0:22 | 0 0 | out1_0 24:152
#define OH_NSCALE 4
#define OH_MIN_SIDE 13                // scipy's reflect on a line of 13 or more needs one reflection (radius 12)


namespace {
const double OH_SCALE_SEARCH[OH_NSCALE] = {0.5, 1.0, 1.5, 2.0};   // hand.py:27
const size_t OH_PICK_SCRATCH = (size_t)1 << 29;                  // bytes of pick scratch per launch (32 B per pixel and part)

// The order bodyfitting_amd/openpose_hand.py pack_hand() writes: conv1_1 .. conv5_3_CPM, conv6_1_CPM, conv6_2_CPM, then per stage
// 2 .. 6 Mconv1 (on the padded 152-channel concat) .. Mconv7.
std::vector<OpLayer> oh_layers(size_t *total) {
    std::vector<OpLayer> L;
    size_t at = 0;
    const int vgg[15][2] = {{3, 64}, {64, 64}, {64, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 512},
                            {512, 512}, {512, 512}, {512, 512}, {512, 512}, {512, 512}, {512, 128}};
    for (int i = 0; i < 15; ++i) op_add_layer(L, &at, vgg[i][0], vgg[i][1], 3);
    op_add_layer(L, &at, 128, 512, 1);
    op_add_layer(L, &at, 512, OH_NMAP, 1);
    for (int s = 2; s <= 6; ++s) {
        op_add_layer(L, &at, OH_CAT, 128, 7);
        for (int j = 2; j <= 5; ++j) op_add_layer(L, &at, 128, 128, 7);
        op_add_layer(L, &at, 128, 128, 1);
        op_add_layer(L, &at, 128, OH_NMAP, 1);
    }
    *total = at;
    return L;
}

// one crop at scale m (hand.py:30-38): scale = m * 368 / bh, the resized size rint(side * scale), padded to a multiple of 8
OhBox oh_box(const int *b, int m, long long px) {
    OhBox o;
    o.view = b[0]; o.x = b[1]; o.y = b[2]; o.bw = b[3]; o.bh = b[4];
    const double s = OH_SCALE_SEARCH[m] * 368 / o.bh;
    o.rh = (int)std::rint((double)o.bh * s);
    o.rw = (int)std::rint((double)o.bw * s);
    o.Hp = (o.rh + 7) / 8 * 8; o.Wp = (o.rw + 7) / 8 * 8;
    o.pad_ = 0;
    o.inv = 1.0 / s;
    o.sy2 = 1.0 / ((double)o.bh / o.rh);
    o.sx2 = 1.0 / ((double)o.bw / o.rw);
    o.px = px;
    return o;
}

// a launch of the network: up to max_hands crops of one scale and one padded size, descriptors at `desc` in the call's table
struct OhChunk { int m, Hp, Wp; size_t desc; std::vector<int> hands; };
}  // namespace

struct bf_openpose_hand {
    int device = 0, max_hands = 0, max_h = 0, max_w = 0;
    hipStream_t stream = nullptr;
    std::vector<OpLayer> layers;
    DevBuf<float> w, inp, act[2], cat, br[2], out;
    DevBuf<uint8_t> img;
    DevBuf<double> heat, tmp, bl, dscr, scores;
    DevBuf<int> iscr, peaks, found;
    DevBuf<OhBox> desc, res_desc;
    std::vector<OhBox> resident;                                   // the crops of the resident maps (scale 0's descriptors)
    long long resident_px = 0;
};

static int oh_fail_box(const char *what, int i, const std::string &why) {
    return fail(BF_ERR_INVALID, std::string(what) + ": box " + std::to_string(i) + " " + why);
}

// boxes[n][5] = (view, x, y, w, h) inside their views (n_views of H x W; n_views = 0: sizes only, for injected outputs)
static int oh_check_boxes(const char *what, int n_views, int H, int W, int n, const int *boxes) {
    if (n < 1 || !boxes) return fail(BF_ERR_INVALID, std::string(what) + ": no boxes");
    for (int i = 0; i < n; ++i) {
        const int *b = boxes + 5 * i;
        if (b[3] < OH_MIN_SIDE || b[4] < OH_MIN_SIDE || b[3] > 8192 || b[4] > 8192)
            return oh_fail_box(what, i, "is " + std::to_string(b[3]) + " x " + std::to_string(b[4]) + ", outside 13 .. 8192 on a side");
        if (n_views > 0 && (b[0] < 0 || b[0] >= n_views || b[1] < 0 || b[2] < 0 || b[1] + b[3] > W || b[2] + b[4] > H))
            return oh_fail_box(what, i, "(view " + std::to_string(b[0]) + ", x " + std::to_string(b[1]) + ", y " + std::to_string(b[2]) +
                                            ", w " + std::to_string(b[3]) + ", h " + std::to_string(b[4]) + ") lies outside its view (" +
                                            std::to_string(n_views) + " views of " + std::to_string(H) + " x " + std::to_string(W) + ")");
    }
    return BF_OK;
}

// model.py:204-217 on h->inp (n x Hp x Wp x 4) -> h->out (n x hq x wq x 22, Mconv7_stage6 without ReLU)
static int oh_network(bf_openpose_hand *h, int n, int Hp, int Wp) {
    hipStream_t s = h->stream;
    const float *Wt = h->w.p;
    const std::vector<OpLayer> &L = h->layers;
    float *A = h->act[0].p, *B = h->act[1].p, *cat = h->cat.p;
    int H = Hp, W = Wp;
    // the VGG front conv1_1 .. conv5_3_CPM, 2 x 2 pools after conv1_2, conv2_2 and conv3_4; conv5_3_CPM writes out1_0 into the concat
    const int pool_after[3] = {1, 3, 7};
    const float *x = h->inp.p;
    int cin = 4, pi = 0;
    HIP_TRY(hipMemsetAsync(cat, 0, (size_t)n * (Hp / 8) * (Wp / 8) * OH_CAT * sizeof(float), s));
    for (int i = 0; i < 15; ++i) {
        const bool last = i == 14;
        float *y = last ? cat + 24 : (x == A ? B : A);
        if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[i], x, cin, y, last ? OH_CAT : L[i].cout, 1))) return rc;
        x = y; cin = L[i].cout;
        if (pi < 3 && i == pool_after[pi]) {
            float *z = x == A ? B : A;
            if (int rc = launch_pool(s, n, H, W, cin, x, z)) return rc;
            x = z; H /= 2; W /= 2; ++pi;
        }
    }
    float *P = h->br[0].p, *Q = h->br[1].p;
    size_t li = 15;
    // stage 1: conv6_1_CPM, then conv6_2_CPM (no ReLU) into the concat's first 22 channels
    if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], cat + 24, OH_CAT, P, 512, 1))) return rc;
    if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], P, 512, cat, OH_CAT, 0))) return rc;
    for (int st = 2; st <= 6; ++st) {
        if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], cat, OH_CAT, P, 128, 1))) return rc;
        for (int j = 2; j <= 6; ++j) {
            if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], P, 128, Q, 128, 1))) return rc;
            std::swap(P, Q);
        }
        // Mconv7 (no ReLU): into the next stage's concat, or - stage 6 - the output
        const bool fin = st == 6;
        if (int rc = launch_conv(s, n, H, W, conv_of(Wt, L[li++], P, 128, fin ? h->out.p : cat, fin ? OH_NMAP : OH_CAT, 0))) return rc;
    }
    return BF_OK;
}

// the call's plan: per scale the crops grouped by padded size (input order within a group), cut into chunks of max_hands
static std::vector<OhChunk> oh_plan(bf_openpose_hand *h, int n, const int *boxes, const std::vector<long long> &px, std::vector<OhBox> *desc) {
    std::vector<OhChunk> plan;
    desc->clear();
    for (int m = 0; m < OH_NSCALE; ++m) {
        std::vector<OhBox> d(n);
        for (int i = 0; i < n; ++i) d[i] = oh_box(boxes + 5 * i, m, px[i]);
        std::vector<bool> done(n, false);
        for (int i = 0; i < n; ++i) {
            if (done[i]) continue;
            std::vector<int> group;
            for (int j = i; j < n; ++j)
                if (!done[j] && d[j].Hp == d[i].Hp && d[j].Wp == d[i].Wp) { group.push_back(j); done[j] = true; }
            for (size_t c = 0; c < group.size(); c += h->max_hands) {
                OhChunk ch;
                ch.m = m; ch.Hp = d[i].Hp; ch.Wp = d[i].Wp; ch.desc = desc->size();
                for (size_t k = c; k < std::min(group.size(), c + (size_t)h->max_hands); ++k) {
                    ch.hands.push_back(group[k]);
                    desc->push_back(d[group[k]]);
                }
                plan.push_back(ch);
            }
        }
    }
    return plan;
}

static int oh_run(bf_openpose_hand *h, int n_views, int H, int W, const uint8_t *bgr, int n, const int *boxes, const float *injected,
                  float *in_host, float *out_host, double *heat) {
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    std::vector<long long> px(n);
    long long total = 0;
    for (int i = 0; i < n; ++i) { px[i] = total; total += (long long)boxes[5 * i + 3] * boxes[5 * i + 4]; }
    std::vector<OhBox> desc;
    const std::vector<OhChunk> plan = oh_plan(h, n, boxes, px, &desc);
    // host offsets of each (scale, crop) in the network input / output layouts: scale-major, crops in input order
    std::vector<size_t> in_at((size_t)OH_NSCALE * n), out_at((size_t)OH_NSCALE * n);
    size_t ia = 0, oa = 0, act = 0, q = 0, up = 0;
    for (int m = 0; m < OH_NSCALE; ++m)
        for (int i = 0; i < n; ++i) {
            const OhBox d = oh_box(boxes + 5 * i, m, px[i]);
            in_at[(size_t)m * n + i] = ia; out_at[(size_t)m * n + i] = oa;
            ia += (size_t)d.Hp * d.Wp * 4; oa += (size_t)d.Hp / 8 * (d.Wp / 8) * OH_NMAP;
        }
    for (const OhChunk &c : plan) {
        const size_t k = c.hands.size(), p = k * c.Hp * c.Wp;
        if (p * 64 > ((size_t)1 << 31)) return fail(BF_ERR_UNSUPPORTED, "bf_openpose_hand: crop size outside what the kernels index");
        act = std::max(act, p * 64);
        q = std::max(q, k * (c.Hp / 8) * (c.Wp / 8));
        for (size_t j = 0; j < k; ++j) up = std::max(up, (size_t)desc[c.desc + j].rh * desc[c.desc + j].rw * OH_NMAP);
    }
    if (bgr) HIP_TRY(bf_grow(s, h->img, (size_t)n_views * H * W * 3));
    HIP_TRY(bf_grow(s, h->inp, act / 16));
    for (int i = 0; i < 2; ++i) HIP_TRY(bf_grow(s, h->act[i], act));
    HIP_TRY(bf_grow(s, h->cat, q * OH_CAT));
    for (int i = 0; i < 2; ++i) HIP_TRY(bf_grow(s, h->br[i], q * 512));
    HIP_TRY(bf_grow(s, h->out, q * OH_NMAP));
    HIP_TRY(bf_grow(s, h->heat, (size_t)total * OH_NMAP));
    HIP_TRY(bf_grow(s, h->desc, desc.size()));
    h->resident.clear(); h->resident_px = 0;
    if (bgr) HIP_TRY(hipMemcpyAsync(h->img.p, bgr, (size_t)n_views * H * W * 3, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->desc.p, desc.data(), desc.size() * sizeof(OhBox), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(h->heat.p, 0, (size_t)total * OH_NMAP * sizeof(double), s));
    for (const OhChunk &c : plan) {
        const int k = (int)c.hands.size(), hq = c.Hp / 8, wq = c.Wp / 8;
        const size_t qn = (size_t)hq * wq * OH_NMAP, pn = (size_t)c.Hp * c.Wp * 4;
        const OhBox *dd = h->desc.p + c.desc;
        if (injected) {
            for (int j = 0; j < k; ++j)
                HIP_TRY(hipMemcpyAsync(h->out.p + j * qn, injected + out_at[(size_t)c.m * n + c.hands[j]], qn * sizeof(float),
                                       hipMemcpyHostToDevice, s));
        } else {
            hipLaunchKernelGGL(bf_oh_input_kernel, dim3(op_blocks((long long)k * c.Hp * c.Wp)), dim3(256), 0, s, k, c.Hp, c.Wp, H, W, dd,
                               (const uint8_t *)h->img.p, (float4 *)h->inp.p);
            HIP_TRY(hipGetLastError());
            if (in_host)
                for (int j = 0; j < k; ++j)
                    HIP_TRY(hipMemcpyAsync(in_host + in_at[(size_t)c.m * n + c.hands[j]], h->inp.p + j * pn, pn * sizeof(float),
                                           hipMemcpyDeviceToHost, s));
            if (int rc = oh_network(h, k, c.Hp, c.Wp)) return rc;
            if (out_host)
                for (int j = 0; j < k; ++j)
                    HIP_TRY(hipMemcpyAsync(out_host + out_at[(size_t)c.m * n + c.hands[j]], h->out.p + j * qn, qn * sizeof(float),
                                           hipMemcpyDeviceToHost, s));
        }
        long long up_n = 0, map_n = 0;
        for (int j = 0; j < k; ++j) {
            const OhBox &d = desc[c.desc + j];
            up_n = std::max(up_n, (long long)d.rh * d.rw * OH_NMAP);
            map_n = std::max(map_n, (long long)d.bh * d.bw * OH_NMAP);
        }
        const long long up_stride = (long long)c.Hp * c.Wp * OH_NMAP;        // >= rh * rw * 22; k of them fit in act[0] (64 per pixel)
        hipLaunchKernelGGL(bf_oh_up8_kernel, dim3(op_blocks(up_n), k), dim3(256), 0, s, hq, wq, up_stride, dd, (const float *)h->out.p,
                           h->act[0].p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bf_oh_maps_kernel, dim3(op_blocks(map_n), k), dim3(256), 0, s, up_stride, dd, (const float *)h->act[0].p,
                           h->heat.p);
        HIP_TRY(hipGetLastError());
    }
    if (heat) HIP_TRY(hipMemcpyAsync(heat, h->heat.p, (size_t)total * OH_NMAP * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) h->resident.push_back(oh_box(boxes + 5 * i, 0, px[i]));
    h->resident_px = total;
    return BF_OK;
}

static int oh_check(bf_openpose_hand *h, int n_views, int H, int W, const void *p, const char *what) {
    if (!h) return fail(BF_ERR_INVALID, std::string(what) + ": no handle");
    if (n_views < 1 || n_views > 4096) return fail(BF_ERR_INVALID, std::string(what) + ": views outside 1 .. 4096");
    if (H < OH_MIN_SIDE || W < OH_MIN_SIDE || H > h->max_h || W > h->max_w)
        return fail(BF_ERR_INVALID, std::string(what) + ": views of " + std::to_string(H) + " x " + std::to_string(W) + " outside 13 .. max_h x 13 .. max_w (" +
                                        std::to_string(h->max_h) + " x " + std::to_string(h->max_w) + ")");
    if (!p) return fail(BF_ERR_INVALID, std::string(what) + ": no views");
    return BF_OK;
}

static size_t oh_output_floats(int n, const int *boxes) {
    size_t t = 0;
    for (int m = 0; m < OH_NSCALE; ++m)
        for (int i = 0; i < n; ++i) { const OhBox d = oh_box(boxes + 5 * i, m, 0); t += (size_t)d.Hp / 8 * (d.Wp / 8) * OH_NMAP; }
    return t;
}

extern "C" {

int64_t bf_openpose_hand_n_weights(void) {
    size_t total = 0;
    oh_layers(&total);
    return (int64_t)total;
}

void bf_openpose_hand_destroy(bf_openpose_hand *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    delete h;
}

int bf_openpose_hand_create(int device, const float *weights, int64_t n_weights, int max_hands, int max_h, int max_w, bf_openpose_hand **out) {
    if (!out || !weights || max_hands < 1 || max_hands > 1024 || max_h < OH_MIN_SIDE || max_w < OH_MIN_SIDE || max_h > 8192 || max_w > 8192)
        return fail(BF_ERR_INVALID, "bf_openpose_hand_create: bad argument");
    *out = nullptr;
    size_t total = 0;
    std::vector<OpLayer> layers = oh_layers(&total);
    if (n_weights != (int64_t)total)
        return fail(BF_ERR_INVALID, "bf_openpose_hand_create: " + std::to_string(n_weights) + " packed weights, the network has " + std::to_string(total));
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_openpose_hand_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto *h = new bf_openpose_hand();
    h->device = device; h->max_hands = max_hands; h->max_h = max_h; h->max_w = max_w; h->layers = std::move(layers);
    const bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
                    h->w.upload(weights, total) == hipSuccess;
    if (!ok) { bf_openpose_hand_destroy(h); return fail(BF_ERR_HIP, "bf_openpose_hand_create: device allocation failed"); }
    *out = h;
    return BF_OK;
}

int bf_openpose_hand_maps(bf_openpose_hand *h, int n_views, int H, int W, const uint8_t *bgr, int n_hands, const int *boxes, double *heat) {
    if (int rc = oh_check(h, n_views, H, W, bgr, "bf_openpose_hand_maps")) return rc;
    if (int rc = oh_check_boxes("bf_openpose_hand_maps", n_views, H, W, n_hands, boxes)) return rc;
    return oh_run(h, n_views, H, W, bgr, n_hands, boxes, nullptr, nullptr, nullptr, heat);
}

int bf_openpose_hand_network(bf_openpose_hand *h, int n_views, int H, int W, const uint8_t *bgr, int n_hands, const int *boxes, float *inputs,
                             float *outputs) {
    if (int rc = oh_check(h, n_views, H, W, bgr, "bf_openpose_hand_network")) return rc;
    if (int rc = oh_check_boxes("bf_openpose_hand_network", n_views, H, W, n_hands, boxes)) return rc;
    if (!outputs) return fail(BF_ERR_INVALID, "bf_openpose_hand_network: no output array");
    return oh_run(h, n_views, H, W, bgr, n_hands, boxes, nullptr, inputs, outputs, nullptr);
}

int bf_openpose_hand_inject(bf_openpose_hand *h, int n_hands, const int *boxes, const float *outputs, int64_t n_outputs, double *heat) {
    if (!h || !outputs) return fail(BF_ERR_INVALID, "bf_openpose_hand_inject: bad argument");
    if (int rc = oh_check_boxes("bf_openpose_hand_inject", 0, 0, 0, n_hands, boxes)) return rc;
    if (n_outputs != (int64_t)oh_output_floats(n_hands, boxes))
        return fail(BF_ERR_INVALID, "bf_openpose_hand_inject: " + std::to_string(n_outputs) + " floats, the four scales need " +
                                        std::to_string(oh_output_floats(n_hands, boxes)));
    return oh_run(h, 0, 0, 0, nullptr, n_hands, boxes, outputs, nullptr, nullptr, heat);
}

int bf_openpose_hand_peaks(bf_openpose_hand *h, int n, double *blurred, int *peaks, double *scores, int *found) {
    if (!h || !peaks || !scores || !found) return fail(BF_ERR_INVALID, "bf_openpose_hand_peaks: bad argument");
    if (h->resident.empty() || n != (int)h->resident.size())
        return fail(BF_ERR_INVALID, "bf_openpose_hand_peaks: " + std::to_string(n) + " crops asked, " + std::to_string(h->resident.size()) + " resident");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const long long total = h->resident_px;
    long long most = 0;
    for (const OhBox &d : h->resident) most = std::max(most, (long long)d.bh * d.bw);
    HIP_TRY(bf_grow(s, h->res_desc, (size_t)n));
    HIP_TRY(bf_grow(s, h->tmp, (size_t)total * OH_NPART));
    HIP_TRY(bf_grow(s, h->bl, (size_t)total * OH_NPART));
    HIP_TRY(bf_grow(s, h->peaks, (size_t)n * OH_NPART * 2));
    HIP_TRY(bf_grow(s, h->scores, (size_t)n * OH_NPART));
    HIP_TRY(bf_grow(s, h->found, (size_t)n * OH_NPART));
    HIP_TRY(hipMemcpyAsync(h->res_desc.p, h->resident.data(), (size_t)n * sizeof(OhBox), hipMemcpyHostToDevice, s));
    const dim3 grid(op_blocks(most * OH_NPART), n);
    hipLaunchKernelGGL(bf_oh_gauss_kernel, grid, dim3(256), 0, s, 0, OH_NMAP, (const OhBox *)h->res_desc.p, (const double *)h->heat.p, h->tmp.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bf_oh_gauss_kernel, grid, dim3(256), 0, s, 1, OH_NPART, (const OhBox *)h->res_desc.p, (const double *)h->tmp.p, h->bl.p);
    HIP_TRY(hipGetLastError());
    // the pick in chunks of crops whose scratch fits the budget
    for (int i = 0; i < n;) {
        int j = i;
        long long cpx = 0;
        while (j < n) {
            const long long p = (long long)h->resident[j].bh * h->resident[j].bw;
            if (j > i && (size_t)(cpx + p) * OH_NPART * 32 > OH_PICK_SCRATCH) break;
            cpx += p; ++j;
        }
        HIP_TRY(bf_grow(s, h->iscr, (size_t)cpx * OH_NPART * 4));
        HIP_TRY(bf_grow(s, h->dscr, (size_t)cpx * OH_NPART * 2));
        hipLaunchKernelGGL(bf_oh_pick_kernel, dim3(OH_NPART, j - i), dim3(256), 0, s, (const OhBox *)(h->res_desc.p + i), h->resident[i].px,
                           (const double *)h->bl.p, (const double *)h->heat.p, h->iscr.p, h->dscr.p, h->peaks.p + (size_t)i * OH_NPART * 2,
                           h->scores.p + (size_t)i * OH_NPART, h->found.p + (size_t)i * OH_NPART);
        HIP_TRY(hipGetLastError());
        i = j;
    }
    if (blurred) HIP_TRY(hipMemcpyAsync(blurred, h->bl.p, (size_t)total * OH_NPART * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(peaks, h->peaks.p, (size_t)n * OH_NPART * 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(scores, h->scores.p, (size_t)n * OH_NPART * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(found, h->found.p, (size_t)n * OH_NPART * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BF_OK;
}

int bf_openpose_hand_selftest_label(int device, int n, int H, int W, const uint8_t *binary, int *labels, int *counts) {
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (long long)H * W > (1LL << 22) || !binary || !labels || !counts)
        return fail(BF_ERR_INVALID, "bf_openpose_hand_selftest_label: bad argument");
    if (device < 0 || device >= bf_device_count()) return fail(BF_ERR_NO_DEVICE, "bf_openpose_hand_selftest_label: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const size_t N = (size_t)H * W;
    DevBuf<uint8_t> db;
    DevBuf<int> scr, dl, dc;
    HIP_TRY(db.upload(binary, N * n));
    HIP_TRY(scr.alloc(N * 4 * n));
    HIP_TRY(dl.alloc(N * n));
    HIP_TRY(dc.alloc((size_t)n));
    hipLaunchKernelGGL(bf_oh_label_kernel, dim3(n), dim3(256), 0, nullptr, H, W, (const uint8_t *)db.p, scr.p, dl.p, dc.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(labels, dl.p, N * n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, dc.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
