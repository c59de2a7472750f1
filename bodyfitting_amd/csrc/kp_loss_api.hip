// Host side of bf_gmm_create / bf_gmm_destroy / bf_keypoint_loss / bf_keypoint_loss_dev (include/bodyfit.h): the reference's
// multiview_keypoint_loss and MaxMixturePrior as one stateless call - what a user's own torch loop (smplify.py:177-213) evaluates
// behind the body model.  One launch of bf_keypoint_loss_kernel (kp_loss_kernels.hip), issued by ONE body on a BfRouteCall
// (dev_route.h); the two entry points check their arguments, count their route and hand it their call: host arrays, the block cache's
// buffers and a drain, or device pointers on the caller's stream with a bf_workspace.
#include "bf_host.h"
#include "dev_route.h"
#include "kp_loss_kernels.h"


struct bf_gmm {
    int device = 0, n_comp = 0, dim = 0;
    DevBuf<float> means, prec, logw;
};

namespace {
// the sizes against the kernel's LDS tables (BF_KPL_MAX_*, bf_internal.h) and against each other
int bf_kp_loss_check(const bf_gmm *g, const bf_keypoint_loss_in *in, const float *dposes, const float *dbetas) {
    const char *who = "bf_keypoint_loss: ";
    if (in->n <= 0 || in->n_views < 0 || in->n_rows < 0) return fail(BF_ERR_INVALID, std::string(who) + "n must be positive, n_views and n_rows non-negative");
    if (in->n_rows > BF_KPL_MAX_ROWS) return fail(BF_ERR_UNSUPPORTED, std::string(who) + "more than " + std::to_string(BF_KPL_MAX_ROWS) + " joint rows");
    if (in->n_rows > 0 && !in->joints) return fail(BF_ERR_INVALID, std::string(who) + "joints is NULL");
    if (in->n_views > 0 && in->n_rows > 0 && (!in->w2c || !in->K || !in->keypoints || !in->divisor))
        return fail(BF_ERR_INVALID, std::string(who) + "w2c, K, keypoints and divisor are required when there are views");
    if (in->n_views > 0 && in->n_rows > 0)
        for (int i = 0; i < in->n; ++i)
            if (in->divisor[i] <= 0) return fail(BF_ERR_INVALID, std::string(who) + "divisor must be positive");
    if (in->poses) {
        if (in->pose_dim > BF_KPL_MAX_DIM) return fail(BF_ERR_UNSUPPORTED, std::string(who) + "pose_dim above " + std::to_string(BF_KPL_MAX_DIM));
        if (in->pose_dim <= 55) return fail(BF_ERR_INVALID, std::string(who) + "pose_dim must be above 55 (the angle prior reads dof 55)");
        if (g && in->pose_dim > g->dim) return fail(BF_ERR_INVALID, std::string(who) + "pose_dim above the GMM's dimension");
    } else if (dposes) return fail(BF_ERR_INVALID, std::string(who) + "dposes asked for without poses");
    if (in->betas) {
        if (in->n_betas <= 0) return fail(BF_ERR_INVALID, std::string(who) + "n_betas must be positive");
        if (in->n_betas > BF_KPL_MAX_BETAS) return fail(BF_ERR_UNSUPPORTED, std::string(who) + "more than " + std::to_string(BF_KPL_MAX_BETAS) + " betas");
    } else if (dbetas) return fail(BF_ERR_INVALID, std::string(who) + "dbetas asked for without betas");
    return BF_OK;
}

// The one launch, on either route (sizes checked, an output wanted).  divisor[n] is a host array on both: the host route uploads it with
// the others, the device route sends it through the workspace, and only when it differs from what the workspace sent last.
int bf_kp_loss_run(BfRouteCall &c, int device, const bf_gmm *gmm, const bf_keypoint_loss_in *in, const bf_hyper &h, const float *dterms,
                   float *terms, float *djoints, float *dposes, float *dbetas) {
    BF_TRY(c.begin(device));
    const size_t N = (size_t)in->n, V = (size_t)in->n_views, R = (size_t)in->n_rows;
    const bool views = V > 0 && R > 0;
    KpLossIO Q{};
    Q.n_views = views ? in->n_views : 0;
    Q.n_rows = in->n_rows;
    if (R > 0) BF_TRY(c.in(in->joints, N * R * 3, Q.joints));
    if (views) {
        BF_TRY(c.in(in->w2c, N * V * 16, Q.w2c));
        BF_TRY(c.in(in->K, N * V * 9, Q.K));
        BF_TRY(c.in(in->keypoints, N * V * R * 3, Q.keypoints));
        if (c.ws) BF_TRY(bf_ws_divisor(c.ws, c.stream, in->divisor, N, &Q.divisor));
        else BF_TRY(c.in(in->divisor, N, Q.divisor));
        BF_TRY(c.in(in->present, N * V, Q.present));
    }
    if (in->poses) {
        Q.pose_dim = in->pose_dim;
        BF_TRY(c.in(in->poses, N * in->pose_dim, Q.poses));
        if (gmm) { Q.gmm_comp = gmm->n_comp; Q.gmm_dim = gmm->dim; Q.g_means = gmm->means.p; Q.g_prec = gmm->prec.p; Q.g_logw = gmm->logw.p; }
    }
    if (in->betas) {
        Q.n_betas = in->n_betas;
        BF_TRY(c.in(in->betas, N * in->n_betas, Q.betas));
    }
    BF_TRY(c.in(dterms, N * 4, Q.dterms));
    BF_TRY(c.out(terms, N * 4, Q.terms));
    if (R > 0) BF_TRY(c.out(djoints, N * R * 3, Q.djoints));
    BF_TRY(c.out(dposes, N * in->pose_dim, Q.dposes));
    BF_TRY(c.out(dbetas, N * in->n_betas, Q.dbetas));
    hipLaunchKernelGGL(bf_keypoint_loss_kernel, dim3((unsigned)N), dim3(BF_KPL_THREADS), 0, c.stream, Q, bf_to_dev(h));
    return c.finish();
}
}  // namespace

extern "C" int bf_gmm_create(int device, int n_components, int dim, const float *means, const float *precisions, const float *nll_weights,
                             bf_gmm **out) {
    if (!out) return fail(BF_ERR_INVALID, "bf_gmm_create: bad argument");
    *out = nullptr;
    if (!means || !precisions || !nll_weights || n_components <= 0 || dim <= 0) return fail(BF_ERR_INVALID, "bf_gmm_create: bad argument");
    if (n_components > BF_KPL_MAX_COMP) return fail(BF_ERR_UNSUPPORTED, "bf_gmm_create: more than " + std::to_string(BF_KPL_MAX_COMP) + " components");
    if (dim > BF_KPL_MAX_DIM) return fail(BF_ERR_UNSUPPORTED, "bf_gmm_create: dimension above " + std::to_string(BF_KPL_MAX_DIM));
    std::vector<float> logw(n_components);
    for (int m = 0; m < n_components; ++m) {
        if (!(nll_weights[m] > 0.f) || !std::isfinite(nll_weights[m])) return fail(BF_ERR_INVALID, "bf_gmm_create: nll_weights must be positive and finite");
        logw[m] = (float)std::log((double)nll_weights[m]);                  // torch.log(self.nll_weights), prior.py:189
    }
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<bf_gmm> g(new bf_gmm);
    g->device = device; g->n_comp = n_components; g->dim = dim;
    const size_t M = (size_t)n_components, D = (size_t)dim;
    HIP_TRY(g->means.upload(means, M * D));
    HIP_TRY(g->prec.upload(precisions, M * D * D));
    HIP_TRY(g->logw.upload(logw));
    *out = g.release();
    return BF_OK;
}

extern "C" void bf_gmm_destroy(bf_gmm *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    delete g;
}

extern "C" int bf_keypoint_loss(int device, const bf_gmm *gmm, const bf_keypoint_loss_in *in, const bf_hyper *hyper, const float *dterms,
                                float *terms, float *djoints, float *dposes, float *dbetas) {
    if (!in) return fail(BF_ERR_INVALID, "bf_keypoint_loss: bad argument");
    if (gmm && gmm->device != device) return fail(BF_ERR_INVALID, "bf_keypoint_loss: the GMM lives on another device");
    BF_TRY(bf_kp_loss_check(gmm, in, dposes, dbetas));
    ++bf_route_stats().host;
    if (!terms && !djoints && !dposes && !dbetas) return BF_OK;
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    if (!(h.imsize > 0.f)) return fail(BF_ERR_INVALID, "bf_keypoint_loss: imsize must be positive");
    BfRouteCall c(nullptr, nullptr);
    return bf_kp_loss_run(c, device, gmm, in, h, dterms, terms, djoints, dposes, dbetas);
}

// The device route: every array of `in` but `divisor` is a device pointer and is read where it lies; the results are written where the
// caller wants them; divisor[n], validated on the host as above, is the one thing sent (bf_kp_loss_run).
extern "C" int bf_keypoint_loss_dev(bf_workspace *ws, void *stream, const bf_gmm *gmm, const bf_keypoint_loss_in *in, const bf_hyper *hyper,
                                    const float *dterms, float *terms, float *djoints, float *dposes, float *dbetas) {
    if (!ws || !in) return fail(BF_ERR_INVALID, "bf_keypoint_loss_dev: bad argument");
    if (gmm && gmm->device != ws->device) return fail(BF_ERR_INVALID, "bf_keypoint_loss_dev: the GMM lives on another device than the workspace");
    BF_TRY(bf_kp_loss_check(gmm, in, dposes, dbetas));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    if (!(h.imsize > 0.f)) return fail(BF_ERR_INVALID, "bf_keypoint_loss_dev: imsize must be positive");
    ++bf_route_stats().dev;
    if (!terms && !djoints && !dposes && !dbetas) return BF_OK;
    BfRouteCall c(ws, (hipStream_t)stream);
    return bf_kp_loss_run(c, ws->device, gmm, in, h, dterms, terms, djoints, dposes, dbetas);
}
