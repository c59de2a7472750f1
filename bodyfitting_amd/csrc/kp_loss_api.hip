// Host side of bf_gmm_create / bf_gmm_destroy / bf_keypoint_loss (include/bodyfit.h): the reference's multiview_keypoint_loss and
// MaxMixturePrior as one stateless call on host arrays - what a user's own torch loop (smplify.py:177-213) evaluates behind the
// body model.  One launch of bf_keypoint_loss_kernel (kp_loss_kernels.hip); the call's buffers come from the device's block cache.
#include "bf_host.h"
#include "dev_route.h"
#include "kp_loss_kernels.h"


struct bf_gmm {
    int device = 0, n_comp = 0, dim = 0;
    DevBuf<float> means, prec, logw;
};

namespace {
struct DrainOnExit { ~DrainOnExit() { (void)hipDeviceSynchronize(); } };

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
    HIP_TRY(g->means.upload(std::vector<float>(means, means + M * D)));
    HIP_TRY(g->prec.upload(std::vector<float>(precisions, precisions + M * D * D)));
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
    HIP_TRY(hipSetDevice(device));
    const size_t N = (size_t)in->n, V = (size_t)in->n_views, R = (size_t)in->n_rows;
    const bool views = V > 0 && R > 0;
    DevBuf<float> d_joints, d_w2c, d_K, d_kp, d_poses, d_betas, d_dterms, d_terms, d_dj, d_dp, d_db;
    DevBuf<unsigned char> d_present;
    DevBuf<int> d_div;
    DrainOnExit drain;               // (destroyed before the buffers: no kernel still uses a block when it goes back to the cache)
    KpLossIO Q{};
    Q.n_views = views ? in->n_views : 0;
    Q.n_rows = in->n_rows;
    if (R > 0) { HIP_TRY(d_joints.upload_pooled(in->joints, N * R * 3)); Q.joints = d_joints.p; }
    if (views) {
        HIP_TRY(d_w2c.upload_pooled(in->w2c, N * V * 16));
        HIP_TRY(d_K.upload_pooled(in->K, N * V * 9));
        HIP_TRY(d_kp.upload_pooled(in->keypoints, N * V * R * 3));
        HIP_TRY(d_div.upload_pooled(in->divisor, N));
        Q.w2c = d_w2c.p; Q.K = d_K.p; Q.keypoints = d_kp.p; Q.divisor = d_div.p;
        if (in->present) { HIP_TRY(d_present.upload_pooled(in->present, N * V)); Q.present = d_present.p; }
    }
    if (in->poses) {
        Q.pose_dim = in->pose_dim;
        HIP_TRY(d_poses.upload_pooled(in->poses, N * in->pose_dim));
        Q.poses = d_poses.p;
        if (gmm) { Q.gmm_comp = gmm->n_comp; Q.gmm_dim = gmm->dim; Q.g_means = gmm->means.p; Q.g_prec = gmm->prec.p; Q.g_logw = gmm->logw.p; }
    }
    if (in->betas) {
        Q.n_betas = in->n_betas;
        HIP_TRY(d_betas.upload_pooled(in->betas, N * in->n_betas));
        Q.betas = d_betas.p;
    }
    if (dterms) { HIP_TRY(d_dterms.upload_pooled(dterms, N * 4)); Q.dterms = d_dterms.p; }
    if (terms) { HIP_TRY(d_terms.alloc_pooled(N * 4)); Q.terms = d_terms.p; }
    if (djoints && R > 0) { HIP_TRY(d_dj.alloc_pooled(N * R * 3)); Q.djoints = d_dj.p; }
    if (dposes) { HIP_TRY(d_dp.alloc_pooled(N * in->pose_dim)); Q.dposes = d_dp.p; }
    if (dbetas) { HIP_TRY(d_db.alloc_pooled(N * in->n_betas)); Q.dbetas = d_db.p; }
    hipLaunchKernelGGL(bf_keypoint_loss_kernel, dim3((unsigned)N), dim3(BF_KPL_THREADS), 0, 0, Q, bf_to_dev(h));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (terms) HIP_TRY(hipMemcpy(terms, d_terms.p, N * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (Q.djoints) HIP_TRY(hipMemcpy(djoints, d_dj.p, N * R * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (dposes) HIP_TRY(hipMemcpy(dposes, d_dp.p, N * in->pose_dim * sizeof(float), hipMemcpyDeviceToHost));
    if (dbetas) HIP_TRY(hipMemcpy(dbetas, d_db.p, N * in->n_betas * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

// The device route (dev_route.h): the same launch on the caller's stream.  Every array of `in` but `divisor` is a device pointer and is
// read where it lies; the results are written where the caller wants them; divisor[n], validated on the host as above, is the one
// thing sent, through the workspace, and only when it differs from what the workspace sent last.
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
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(ws->device));
    const hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)in->n;
    const bool views = in->n_views > 0 && in->n_rows > 0;
    BfWsCall call(ws, s);
    BF_TRY(call.begin());
    KpLossIO Q{};
    Q.n_views = views ? in->n_views : 0;
    Q.n_rows = in->n_rows;
    if (in->n_rows > 0) Q.joints = in->joints;
    if (views) {
        Q.w2c = in->w2c; Q.K = in->K; Q.keypoints = in->keypoints; Q.present = in->present;
        BF_TRY(bf_ws_divisor(ws, s, in->divisor, N, &Q.divisor));
    }
    if (in->poses) {
        Q.pose_dim = in->pose_dim;
        Q.poses = in->poses;
        if (gmm) { Q.gmm_comp = gmm->n_comp; Q.gmm_dim = gmm->dim; Q.g_means = gmm->means.p; Q.g_prec = gmm->prec.p; Q.g_logw = gmm->logw.p; }
    }
    if (in->betas) { Q.n_betas = in->n_betas; Q.betas = in->betas; }
    Q.dterms = dterms;
    Q.terms = terms;
    if (in->n_rows > 0) Q.djoints = djoints;
    Q.dposes = dposes;
    Q.dbetas = dbetas;
    hipLaunchKernelGGL(bf_keypoint_loss_kernel, dim3((unsigned)N), dim3(BF_KPL_THREADS), 0, s, Q, bf_to_dev(h));
    HIP_TRY(hipGetLastError());
    return BF_OK;
}
