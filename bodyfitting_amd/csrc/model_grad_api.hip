// Host side of bf_smpl_vjp, bf_smplx_forward and bf_smplx_vjp (include/bodyfit.h): the reverse torch.autograd runs through
// models.smpl.SMPL.forward (smplx's lbs() and models/smpl.py:69-83), smplx.create(model_type='smplx', ...)'s forward as the reference
// calls it (smplify.py:177-190) and its reverse - all on the dense schedule's mesh passes, through one ModelPass:
//   forward  bf_pose_state_kernel (non-packed thetas, no similarity, constant scale 1) + the mesh pass; for the reverse it saves the
//            pose-blended vertices and, on an SMPL-X model, the landmarks' vertices / weights of every frame
//   reverse  1. bf_model_vjp_fold_kernel: the joint cotangents onto the vertices (selector, J_regressor_extra, landmarks) and the
//               posed chain joints
//            2. bf_mesh_bwd_multi_launch + bf_ext_reduce_kernel, unchanged (no mask fold, no doorbell): dfeat | skinning sums per
//               joint | dbeta | dt ds per frame
//            3. bf_smpl_vjp_chain_kernel (table-driven, one lane per joint): the kinematic chain and Rodrigues reversed -> dtheta, dbeta
// SMPL-X puts bf_smplx_pose_assemble_kernel (blocks -> full_pose) in front, bf_smplx_dyn_row_kernel behind its forward and
// bf_smplx_pose_reverse_kernel (dtheta + dfull_pose -> the parameter blocks) behind its reverse.
// With expression coefficients (bf_smplx_forward_expr / bf_smplx_vjp_expr on a model bf_model_set_expression gave directions to) the
// kernels of expr_kernels.hip go around those passes, which stay as they are: bf_expr_chain_kernel between the pose state and the mesh
// pass, bf_expr_vertex_kernel between the mesh and the joints pass, bf_expr_reverse_kernel + bf_ext_reduce_kernel in front of the chain
// reverse, which takes Jx psi into its rest joints and closes dexpression.  Without coefficients the launch sequence is the one above.
// Stateless: nothing stays on the device between calls but the model's lazily built posedirsT.
#include "bf_host.h"
#include "dev_route.h"
#include "mesh_kernels.h"
#include "model_grad_kernels.h"
#include "expr_kernels.h"
#include "scan_kernels.h"


// the model is of the entry point's kind and fits the kernels' LDS tables (BF_GRAD_MAX_*, bf_internal.h)
static int bf_grad_check(const bf_model *m, int kind, const char *who) {
    if (m->kind != kind) return fail(BF_ERR_UNSUPPORTED, std::string(who) + (kind ? ": SMPL-X-kind models only" : ": SMPL-kind models only"));
    // (np: the pose assembly's table, which an SMPL model never meets)
    if (m->nj > BF_GRAD_MAX_JOINTS || m->n_all > BF_GRAD_MAX_ALL || m->n_selector > BF_GRAD_MAX_SEL || m->n_lmk > BF_GRAD_MAX_LMK ||
        m->n_joint_map > BF_GRAD_MAX_MAP || (kind && m->np > BF_GRAD_MAX_NP) || m->n_all != m->nj + m->n_selector + m->n_extra + m->n_lmk)
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + (kind ? ": model larger than the kernels' tables" : ": model larger than the reverse kernels' tables"));
    return BF_OK;
}

namespace {
struct DrainOnExit { bool on = true; ~DrainOnExit() { if (on) (void)hipDeviceSynchronize(); } };

// One call's forward and reverse through a body model, and the buffers both run on.  A fitting loop calls these entry points once
// per step: the buffers come from the device's block cache, not from hipMalloc / hipFree.  Whatever else the kernels of a call
// touch is declared BEFORE its ModelPass, so that `drain` has run when those blocks go back to the cache.
// That is the host route: the null stream, pooled buffers, the device drained on the way out.  The device route (the *_dev entry points)
// gives the pass its caller's stream and workspace: the same launches with the same arguments go to that stream, the buffers are the
// workspace's slots, nothing is drained, and an output the caller wants (`to`) is written where the caller wants it.
struct ModelPass {
    bf_model *const m;
    const int n;
    const hipStream_t stream;
    bf_workspace *const ws;
    struct { float *vraw = nullptr, *joints = nullptr, *jraw = nullptr, *dbeta = nullptr, *dexpr = nullptr; } to;      // the caller's blocks (device route)
    DevBuf<float> state, vraw, vposed, xpart, joints, jraw, lmk_w, dv, dchain, part, ext, dtheta, dbeta;
    DevBuf<float> dJx, epart, emesh, dexpr;         // with expression coefficients only (expr_kernels.hip)
    const float *expr = nullptr;                    // the coefficients [n][n_expr] on the device: set by a forward that was given them
    DevBuf<int> lmk_vid;
    MeshScratch scratch;
    // (destroyed before the buffers: whatever path leaves the call, no kernel still uses a block when it goes back to the cache)
    DrainOnExit drain;
    ModelPass(bf_model *model, int frames, hipStream_t s = nullptr, bf_workspace *w = nullptr) : m(model), n(frames), stream(s), ws(w) { drain.on = !w; }

    // `count` elements for b: the caller's block when there is one, else a slot of the workspace, else a block of the cache
    template <class T>
    int need(DevBuf<T> &b, size_t count, T *target = nullptr) {
        if (target) { b.slice(target, count); return BF_OK; }
        if (!ws) { HIP_TRY(b.alloc_pooled(count)); return BF_OK; }
        void *p = nullptr;
        BF_TRY(bf_ws_take(ws, std::max<size_t>(count, 1) * sizeof(T), &p));
        b.slice((T *)p, count);
        return BF_OK;
    }
    // the mesh pass, and the workspace scratch's growth counted with the workspace's other allocations
    int launch_mesh(const MeshPass &mesh) {
        const MeshScratch *s = mesh.scr;
        const float *a = s->pose_off.p, *b = s->featT.p;
        const int rc = bf_launch_mesh(m, mesh);
        if (ws) bf_route_stats().allocs += (s->pose_off.p != a) + (s->featT.p != b);
        return rc;
    }

    // Model space: no similarity, constant scale 1 - as bf_smpl_forward builds its state, so that the mesh reverse's dvout is dL/dv in
    // model space.  for_reverse: vposed is saved instead of the mapped joints.  An SMPL-X model's joints pass leaves all its joints
    // (jraw) and, for the reverse, every frame's landmark vertices and weights (the contour row of ITS yaw).
    // expression (device, [n][n_expr]; null: none - then the launches are the ones of a model without directions): the chain delta
    // shifts the state's Gt / At in front of the mesh pass, the vertex delta runs between the mesh and the joints pass.
    int forward(const float *beta, const float *th_root, const float *th_rest, bool for_reverse, const float *expression = nullptr) {
        const size_t N = (size_t)n, nv3 = (size_t)m->nv * 3;
        const bool x = m->kind == 1;
        expr = expression;
        BF_TRY(need(state, N * bf_state_stride(m->nj, m->npf, m->nb)));
        BF_TRY(need(vraw, N * nv3, to.vraw));
        if (for_reverse) BF_TRY(need(vposed, N * nv3));
        if (x) {
            BF_TRY(need(xpart, N * m->mesh.n_tiles * std::max(m->n_extra, 1) * 3));
            BF_TRY(need(jraw, N * m->n_all * 3, to.jraw));
            if (!for_reverse) BF_TRY(need(joints, N * m->n_joint_map * 3, to.joints));
            if (for_reverse) BF_TRY(need(lmk_vid, N * m->n_lmk * 3));
            if (for_reverse) BF_TRY(need(lmk_w, N * m->n_lmk * 3));
        }
        hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, stream, m->fit, beta, th_root, th_rest, (const float *)nullptr, state.p,
                           (const float *)nullptr, (const float *)nullptr, 1.0f);
        HIP_TRY(hipGetLastError());
        MeshPass mesh;
        mesh.scr = ws ? &ws->scratch : &scratch; mesh.n = n; mesh.state = state.p; mesh.stream = stream;
        mesh.vraw = vraw.p; mesh.xpart = xpart.p; mesh.vposed = vposed.p;
        if (!expr) {
            mesh.joints = joints.p; mesh.jraw = jraw.p; mesh.lmk_vid = lmk_vid.p; mesh.lmk_w = lmk_w.p;
            return launch_mesh(mesh);
        }
        const int ne = m->n_expr;
        BF_TRY(need(dJx, N * m->nj * 3));
        hipLaunchKernelGGL(bf_expr_chain_kernel, dim3(n), dim3(64), 0, stream, m->fit, state.p, expr, ne, (const float *)m->Jx.p, dJx.p);
        HIP_TRY(hipGetLastError());
        BF_TRY(launch_mesh(mesh));                             // (no joints asked for: the mesh pass alone)
        hipLaunchKernelGGL(bf_expr_vertex_kernel, dim3((m->nv + 255) / 256, n), dim3(256), 0, stream, m->mesh, (const float *)state.p, expr, ne,
                           (const float *)m->exprT.p, vraw.p, vposed.p);
        HIP_TRY(hipGetLastError());
        if (m->n_extra > 0) {                                     // the extra-regressor joints' per-tile sums, from the updated vertices
            hipLaunchKernelGGL(bf_expr_xpart_kernel, dim3(m->mesh.n_tiles, n), dim3(128), 0, stream, m->mesh, (const float *)vraw.p, xpart.p);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(bf_joints_kernel, dim3(n), dim3(256), 0, stream, m->mesh, (const float *)state.p, (const float *)vraw.p,
                           (const float *)xpart.p, joints.p, (float *)nullptr, jraw.p, lmk_vid.p, lmk_w.p, BfHandOver{});
        HIP_TRY(hipGetLastError());
        return BF_OK;
    }

    // After forward(..., true): the cotangents on the device (any may be null = zero; ddirect covers the first n_direct joints) ->
    // dtheta[n][3 NJ], dbeta[n][NB], left on the device.  The caller holds the model's posedirsT (bf_ensure_posedirsT_locked).
    int reverse(const float *dvertices, const float *djoints, const float *ddirect, int n_direct, bool want_dexpr = false) {
        const int nj = m->nj, nb = m->nb, nv = m->nv;
        const size_t N = (size_t)n, nv3 = (size_t)nv * 3;
        const int EXT = m->npf + nj * 12 + nb + 4;
        // (one frame: room for the split single-frame instance of the mesh reverse, two partial rows per tile)
        const int part_rows = (n == 1 ? 2 : 1) * m->mesh.n_tiles;
        BF_TRY(need(dv, N * nv3));
        BF_TRY(need(dchain, N * nj * 3));
        BF_TRY(need(part, N * part_rows * EXT));
        BF_TRY(need(ext, N * EXT));
        BF_TRY(need(dtheta, N * nj * 3));
        BF_TRY(need(dbeta, N * nb, to.dbeta));
        // 1. joint cotangents -> dL/dvertices of the mesh reverse, dL/d(posed chain joints)
        hipLaunchKernelGGL(bf_model_vjp_fold_kernel, dim3((nv + 255) / 256, n), dim3(256), 0, stream, m->mesh, dvertices, djoints, ddirect, n_direct,
                           (const int *)lmk_vid.p, (const float *)lmk_w.p, dv.p, dchain.p);
        HIP_TRY(hipGetLastError());
        // 2. the dense schedule's reverse mesh pass (no silhouette fold) and its reduction (no doorbell)
        int rows = m->mesh.n_tiles;
        const int e = bf_mesh_bwd_multi_launch(&m->mesh, m->posedirsT.p, state.p, n, dv.p, vposed.p, vraw.p, part.p, stream,
                                               nullptr, 0, 0, 4, part_rows, &rows, nullptr);
        if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_bwd_multi_kernel: ") + hipGetErrorString((hipError_t)e));
        hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((EXT + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, stream,
                           (const float *)part.p, rows, EXT, ext.p, EXT, (int *)nullptr, 0);
        HIP_TRY(hipGetLastError());
        // (with expression coefficients whose gradient is wanted) E_v^T (sum_j w_vj GR_j^T dv_v) per 256-vertex tile, the tiles in tile order
        const int ne = expr ? m->n_expr : 0, etiles = (nv + 255) / 256;
        const bool dex = expr && want_dexpr;
        if (dex) {
            BF_TRY(need(epart, N * etiles * ne));
            BF_TRY(need(emesh, N * ne));
            BF_TRY(need(dexpr, N * ne, to.dexpr));
            hipLaunchKernelGGL(bf_expr_reverse_kernel, dim3(etiles, n), dim3(256), 0, stream, m->mesh, (const float *)state.p, (const float *)dv.p, ne,
                               (const float *)m->exprT.p, epart.p);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((ne + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, stream,
                               (const float *)epart.p, etiles, ne, emesh.p, ne, (int *)nullptr, 0);
            HIP_TRY(hipGetLastError());
        }
        // 3. chain + Rodrigues reversed (the rest joints with Jx psi; dexpression = the vertex part + Jx^T dL/d(rest joints))
        hipLaunchKernelGGL(bf_smpl_vjp_chain_kernel, dim3(n), dim3(64), 0, stream, m->fit, (const float *)state.p, (const float *)ext.p, EXT,
                           (const float *)dchain.p, dtheta.p, dbeta.p, (const float *)(expr ? dJx.p : nullptr),
                           (const float *)(expr ? m->Jx.p : nullptr), ne, (const float *)(dex ? emesh.p : nullptr), dex ? dexpr.p : (float *)nullptr);
        HIP_TRY(hipGetLastError());
        return BF_OK;
    }
};

// rows[n][stride] on the device -> per block (dst, off, cnt), dst[n][cnt] = rows[.][off .. off + cnt) on the host (null dst: not wanted)
struct Block { float *dst; int off, cnt; };
int fetch_blocks(const float *rows_dev, size_t N, int stride, std::initializer_list<Block> blocks) {
    std::vector<float> g(N * stride);
    HIP_TRY(hipMemcpy(g.data(), rows_dev, g.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (const Block &b : blocks)
        if (b.dst)
            for (size_t f = 0; f < N; ++f) std::memcpy(b.dst + f * b.cnt, g.data() + f * stride + b.off, b.cnt * sizeof(float));
    return BF_OK;
}

int ensure_posedirsT(bf_model *m) {
    std::lock_guard<std::mutex> g(m->lazy);
    return bf_ensure_posedirsT_locked(m, nullptr);
}

// SMPL-X: the parameter blocks on the device and the thetas assembled from them
struct Inputs {
    DevBuf<float> beta, orient, body, jaw, leye, reye, lh, rh, full, th_root, th_rest;
    // (device route) the caller's blocks as they lie
    void view(const bf_model *m, size_t N, const bf_smplx_params *in) {
        const int n_pca = m->fit.n_pca;
        const auto at = [](DevBuf<float> &b, const float *p, size_t count) { if (p) b.slice(const_cast<float *>(p), count); };
        at(beta, in->betas, N * m->nb); at(orient, in->global_orient, N * 3); at(body, in->body_pose, N * m->fit.nbp);
        at(jaw, in->jaw_pose, N * 3); at(leye, in->leye_pose, N * 3); at(reye, in->reye_pose, N * 3);
        at(lh, in->left_hand_pose, N * n_pca); at(rh, in->right_hand_pose, N * n_pca);
    }
    int upload_and_assemble(const bf_model *m, size_t N, const bf_smplx_params *in, ModelPass &pass) {
        const int n_pca = m->fit.n_pca;
        HIP_TRY(beta.upload_pooled(in->betas, N * m->nb));
        HIP_TRY(orient.upload_pooled(in->global_orient, N * 3));
        HIP_TRY(body.upload_pooled(in->body_pose, N * m->fit.nbp));
        if (in->jaw_pose) HIP_TRY(jaw.upload_pooled(in->jaw_pose, N * 3));
        if (in->leye_pose) HIP_TRY(leye.upload_pooled(in->leye_pose, N * 3));
        if (in->reye_pose) HIP_TRY(reye.upload_pooled(in->reye_pose, N * 3));
        if (in->left_hand_pose) HIP_TRY(lh.upload_pooled(in->left_hand_pose, N * n_pca));
        if (in->right_hand_pose) HIP_TRY(rh.upload_pooled(in->right_hand_pose, N * n_pca));
        return assemble(m, N, pass, nullptr);
    }
    // full_to: the caller's full_pose block (device route), or null
    int assemble(const bf_model *m, size_t N, ModelPass &pass, float *full_to) {
        const int nj = m->nj;
        BF_TRY(pass.need(full, N * 3 * nj, full_to));
        BF_TRY(pass.need(th_root, N * 3));
        BF_TRY(pass.need(th_rest, N * 3 * (nj - 1)));
        hipLaunchKernelGGL(bf_smplx_pose_assemble_kernel, dim3((unsigned)N), dim3(64), 0, pass.stream, m->fit, (const float *)orient.p, (const float *)body.p,
                           (const float *)jaw.p, (const float *)leye.p, (const float *)reye.p, (const float *)lh.p, (const float *)rh.p,
                           full.p, th_root.p, th_rest.p);
        HIP_TRY(hipGetLastError());
        return BF_OK;
    }
};
}  // namespace

extern "C" int bf_smpl_vjp(bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                           const float *dvertices, const float *djoints, const float *djoints_ori,
                           float *dbetas, float *dglobal_orient, float *dbody_pose) {
    if (!m || n <= 0 || !betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, "bf_smpl_vjp: bad argument");
    BF_TRY(bf_grad_check(m, 0, "bf_smpl_vjp"));
    ++bf_route_stats().host;
    if (!dbetas && !dglobal_orient && !dbody_pose) return BF_OK;
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(ensure_posedirsT(m));
    const int nj = m->nj, nb = m->nb, n_ori = nj + m->n_selector;
    const size_t N = (size_t)n;
    DevBuf<float> d_beta, d_or, d_bp, d_dvert, d_dj, d_djo;
    ModelPass pass(m, n);
    HIP_TRY(d_beta.upload_pooled(betas, N * nb));
    HIP_TRY(d_or.upload_pooled(global_orient, N * 3));
    HIP_TRY(d_bp.upload_pooled(body_pose, N * 3 * (nj - 1)));
    if (dvertices) HIP_TRY(d_dvert.upload_pooled(dvertices, N * m->nv * 3));
    if (djoints) HIP_TRY(d_dj.upload_pooled(djoints, N * m->n_joint_map * 3));
    if (djoints_ori) HIP_TRY(d_djo.upload_pooled(djoints_ori, N * n_ori * 3));
    BF_TRY(pass.forward(d_beta.p, d_or.p, d_bp.p, true));
    BF_TRY(pass.reverse(d_dvert.p, d_dj.p, d_djo.p, n_ori));
    HIP_TRY(hipDeviceSynchronize());
    if (dbetas) HIP_TRY(hipMemcpy(dbetas, pass.dbeta.p, N * nb * sizeof(float), hipMemcpyDeviceToHost));
    if (!dglobal_orient && !dbody_pose) return BF_OK;
    return fetch_blocks(pass.dtheta.p, N, 3 * nj, {{dglobal_orient, 0, 3}, {dbody_pose, 3, 3 * (nj - 1)}});
}

// a call's expression argument against the model: coefficients need directions
static int bf_expr_check(const bf_model *m, const float *expression, const char *who) {
    if (expression && m->n_expr == 0)
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": the model has no expression directions - call bf_model_set_expression first");
    return BF_OK;
}

extern "C" int bf_model_n_expression(const bf_model *m) { return m ? m->n_expr : 0; }

extern "C" int bf_model_set_expression(bf_model *m, int n_expr, const float *exprdirs) {
    if (!m || !exprdirs) return fail(BF_ERR_INVALID, "bf_model_set_expression: bad argument");
    BF_TRY(bf_grad_check(m, 1, "bf_model_set_expression"));
    if (n_expr < 1 || n_expr > BF_EXPR_MAX)
        return fail(BF_ERR_UNSUPPORTED, "bf_model_set_expression: 1.." + std::to_string(BF_EXPR_MAX) + " expression coefficients supported");
    std::lock_guard<std::mutex> g(m->lazy);
    if (m->n_expr != 0) return fail(BF_ERR_INVALID, "bf_model_set_expression: the model has its expression directions already");
    HIP_TRY(hipSetDevice(m->device));
    const int nv = m->nv, nj = m->nj, ne = n_expr;
    // E transposed: [l][k][v]
    std::vector<float> eT((size_t)ne * 3 * nv);
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < ne; ++l) eT[((size_t)l * 3 + k) * nv + v] = exprdirs[((size_t)v * 3 + k) * ne + l];
    // Jx = J_regressor E: float64 accumulation over a joint's non-zero weights in vertex order, rounded once (as contract_regressor forms Jd)
    std::vector<float> jx((size_t)nj * 3 * ne);
    std::vector<double> acc((size_t)3 * ne);
    for (int j = 0; j < nj; ++j) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int q = m->jreg_start[j]; q < m->jreg_start[j + 1]; ++q) {
            const double w = m->jreg_w[q];
            const float *e = exprdirs + (size_t)m->jreg_v[q] * 3 * ne;
            for (int i = 0; i < 3 * ne; ++i) acc[i] += w * e[i];
        }
        for (int i = 0; i < 3 * ne; ++i) jx[(size_t)j * 3 * ne + i] = (float)acc[i];
    }
    HIP_TRY(m->exprT.upload(eT));
    HIP_TRY(m->Jx.upload(jx));
    m->n_expr = ne;
    return BF_OK;
}

extern "C" int bf_smplx_forward(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_outputs *out) {
    return bf_smplx_forward_expr(m, n, in, nullptr, out);
}

extern "C" int bf_smplx_forward_expr(bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_outputs *out) {
    const char *who = expression ? "bf_smplx_forward_expr" : "bf_smplx_forward";
    if (!m || n <= 0 || !in || !out || !in->betas || !in->global_orient || !in->body_pose)
        return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 1, who));
    BF_TRY(bf_expr_check(m, expression, who));
    ++bf_route_stats().host;
    HIP_TRY(hipSetDevice(m->device));
    const size_t N = (size_t)n;
    Inputs x;
    DevBuf<int> d_row;
    DevBuf<float> d_expr;
    ModelPass pass(m, n);
    BF_TRY(x.upload_and_assemble(m, N, in, pass));
    if (expression) HIP_TRY(d_expr.upload_pooled(expression, N * m->n_expr));
    HIP_TRY(d_row.alloc_pooled(N));
    BF_TRY(pass.forward(x.beta.p, x.th_root.p, x.th_rest.p, false, d_expr.p));
    hipLaunchKernelGGL(bf_smplx_dyn_row_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, m->mesh, (const float *)pass.state.p, n, d_row.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (out->vertices) HIP_TRY(hipMemcpy(out->vertices, pass.vraw.p, N * m->nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->joints) HIP_TRY(hipMemcpy(out->joints, pass.joints.p, N * m->n_joint_map * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->joints_all) HIP_TRY(hipMemcpy(out->joints_all, pass.jraw.p, N * m->n_all * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->full_pose) HIP_TRY(hipMemcpy(out->full_pose, x.full.p, N * 3 * m->nj * sizeof(float), hipMemcpyDeviceToHost));
    if (out->dyn_row) HIP_TRY(hipMemcpy(out->dyn_row, d_row.p, N * sizeof(int), hipMemcpyDeviceToHost));
    return BF_OK;
}

extern "C" int bf_smplx_vjp(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_cotangents *cot, const bf_smplx_grads *grads) {
    return bf_smplx_vjp_expr(m, n, in, nullptr, cot, grads, nullptr);
}

extern "C" int bf_smplx_vjp_expr(bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_cotangents *cot,
                                 const bf_smplx_grads *grads, float *dexpression) {
    const char *who = expression ? "bf_smplx_vjp_expr" : "bf_smplx_vjp";
    if (!m || n <= 0 || !in || !cot || !grads || !in->betas || !in->global_orient || !in->body_pose || (dexpression && !expression))
        return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 1, who));
    BF_TRY(bf_expr_check(m, expression, who));
    ++bf_route_stats().host;
    if (!grads->dbetas && !grads->dglobal_orient && !grads->dbody_pose && !grads->djaw_pose && !grads->dleye_pose && !grads->dreye_pose &&
        !grads->dleft_hand_pose && !grads->dright_hand_pose && !dexpression)
        return BF_OK;
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(ensure_posedirsT(m));
    const int nj = m->nj, nb = m->nb, n_pca = m->fit.n_pca, nbp = m->fit.nbp, OUT = 3 * nj + 2 * n_pca;
    const size_t N = (size_t)n;
    Inputs x;
    DevBuf<float> d_dvert, d_dj, d_dja, d_dfull, d_out, d_expr;
    ModelPass pass(m, n);
    BF_TRY(x.upload_and_assemble(m, N, in, pass));
    if (expression) HIP_TRY(d_expr.upload_pooled(expression, N * m->n_expr));
    if (cot->dvertices) HIP_TRY(d_dvert.upload_pooled(cot->dvertices, N * m->nv * 3));
    if (cot->djoints) HIP_TRY(d_dj.upload_pooled(cot->djoints, N * m->n_joint_map * 3));
    if (cot->djoints_all) HIP_TRY(d_dja.upload_pooled(cot->djoints_all, N * m->n_all * 3));
    if (cot->dfull_pose) HIP_TRY(d_dfull.upload_pooled(cot->dfull_pose, N * 3 * nj));
    HIP_TRY(d_out.alloc_pooled(N * OUT));
    BF_TRY(pass.forward(x.beta.p, x.th_root.p, x.th_rest.p, true, d_expr.p));
    BF_TRY(pass.reverse(d_dvert.p, d_dj.p, d_dja.p, m->n_all, dexpression != nullptr));
    // the pose assembly reversed
    hipLaunchKernelGGL(bf_smplx_pose_reverse_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)pass.dtheta.p, (const float *)d_dfull.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (grads->dbetas) HIP_TRY(hipMemcpy(grads->dbetas, pass.dbeta.p, N * nb * sizeof(float), hipMemcpyDeviceToHost));
    if (dexpression) HIP_TRY(hipMemcpy(dexpression, pass.dexpr.p, N * m->n_expr * sizeof(float), hipMemcpyDeviceToHost));
    // full pose order: root | body | jaw | left eye | right eye | hands (through their PCA coefficients, behind the thetas)
    return fetch_blocks(d_out.p, N, OUT, {{grads->dglobal_orient, 0, 3}, {grads->dbody_pose, 3, nbp}, {grads->djaw_pose, 3 + nbp, 3},
                                          {grads->dleye_pose, 6 + nbp, 3}, {grads->dreye_pose, 9 + nbp, 3},
                                          {grads->dleft_hand_pose, 3 * nj, n_pca}, {grads->dright_hand_pose, 3 * nj + n_pca, n_pca}});
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The device route: the entry points above on device pointers, on the caller's stream, with the caller's workspace.  Each issues its
// host twin's kernels in its twin's order with its twin's grids and arguments; what differs is where the buffers come from and that
// nothing waits.  Outputs a pass can write in place are given the caller's pointer (ModelPass::to); the gradient rows that have to be
// cut into the caller's blocks go through bf_block_scatter_kernel.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
int scatter_blocks(const float *rows, int n, int stride, std::initializer_list<Block> blocks, hipStream_t stream) {
    BfScatter S{};
    for (const Block &b : blocks)
        if (b.dst && b.cnt > 0) { S.dst[S.n_blocks] = b.dst; S.off[S.n_blocks] = b.off; S.cnt[S.n_blocks] = b.cnt; ++S.n_blocks; }
    if (S.n_blocks == 0) return BF_OK;
    const size_t total = (size_t)n * stride;
    hipLaunchKernelGGL(bf_block_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, rows, n, stride, S);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

// the arguments every *_dev entry point of a model shares
int dev_route_check(const bf_model *m, const bf_workspace *ws, int n, const char *who) {
    if (!m || !ws || n <= 0) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    if (ws->device != m->device) return fail(BF_ERR_INVALID, std::string(who) + ": the workspace lives on another device than the model");
    return BF_OK;
}

int ensure_posedirsT_on(bf_model *m, hipStream_t stream) {
    std::lock_guard<std::mutex> g(m->lazy);
    return bf_ensure_posedirsT_locked(m, stream);       // (built once, and complete on the device when this returns: later calls come on any stream)
}
}  // namespace

extern "C" int bf_smpl_forward_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const float *betas, const float *global_orient,
                                   const float *body_pose, float *vertices, float *joints, float *joints_ori) {
    const char *who = "bf_smpl_forward_dev";
    BF_TRY(dev_route_check(m, ws, n, who));
    if (!betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    if (m->kind != 0) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": SMPL-kind models only");
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(m->device));
    const hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)n;
    BfWsCall call(ws, s);
    BF_TRY(call.begin());
    // bf_smpl_forward's buffers and launches (api.hip)
    ModelPass pass(m, n, s, ws);
    DevBuf<float> jori;
    BF_TRY(pass.need(pass.state, N * bf_state_stride(m->nj, m->npf, m->nb)));
    BF_TRY(pass.need(pass.vraw, N * m->nv * 3, vertices));
    BF_TRY(pass.need(pass.xpart, N * m->mesh.n_tiles * m->n_extra * 3));
    BF_TRY(pass.need(pass.joints, N * m->n_joint_map * 3, joints));
    BF_TRY(pass.need(jori, N * (m->nj + m->n_selector) * 3, joints_ori));
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, s, m->fit, betas, global_orient, body_pose, (const float *)nullptr,
                       pass.state.p, (const float *)nullptr, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    MeshPass mesh;
    mesh.scr = &ws->scratch; mesh.n = n; mesh.state = pass.state.p; mesh.stream = s;
    mesh.vraw = pass.vraw.p; mesh.xpart = pass.xpart.p; mesh.joints = pass.joints.p; mesh.joints_ori = jori.p;
    return pass.launch_mesh(mesh);
}

extern "C" int bf_smpl_vjp_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const float *betas, const float *global_orient,
                               const float *body_pose, const float *dvertices, const float *djoints, const float *djoints_ori,
                               float *dbetas, float *dglobal_orient, float *dbody_pose) {
    const char *who = "bf_smpl_vjp_dev";
    BF_TRY(dev_route_check(m, ws, n, who));
    if (!betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 0, who));
    ++bf_route_stats().dev;
    if (!dbetas && !dglobal_orient && !dbody_pose) return BF_OK;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(m->device));
    const hipStream_t s = (hipStream_t)stream;
    BF_TRY(ensure_posedirsT_on(m, s));
    const int nj = m->nj, n_ori = nj + m->n_selector;
    BfWsCall call(ws, s);
    BF_TRY(call.begin());
    ModelPass pass(m, n, s, ws);
    pass.to.dbeta = dbetas;
    BF_TRY(pass.forward(betas, global_orient, body_pose, true));
    BF_TRY(pass.reverse(dvertices, djoints, djoints_ori, n_ori));
    return scatter_blocks(pass.dtheta.p, n, 3 * nj, {{dglobal_orient, 0, 3}, {dbody_pose, 3, 3 * (nj - 1)}}, s);
}

extern "C" int bf_smplx_forward_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const bf_smplx_params *in, const float *expression,
                                    const bf_smplx_outputs *out) {
    const char *who = "bf_smplx_forward_dev";
    BF_TRY(dev_route_check(m, ws, n, who));
    if (!in || !out || !in->betas || !in->global_orient || !in->body_pose) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 1, who));
    BF_TRY(bf_expr_check(m, expression, who));
    ++bf_route_stats().dev;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(m->device));
    const hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)n;
    BfWsCall call(ws, s);
    BF_TRY(call.begin());
    Inputs x;
    DevBuf<int> d_row;
    ModelPass pass(m, n, s, ws);
    pass.to.vraw = out->vertices; pass.to.joints = out->joints; pass.to.jraw = out->joints_all;
    x.view(m, N, in);
    BF_TRY(x.assemble(m, N, pass, out->full_pose));
    BF_TRY(pass.need(d_row, N, (int *)out->dyn_row));
    BF_TRY(pass.forward(x.beta.p, x.th_root.p, x.th_rest.p, false, expression));
    hipLaunchKernelGGL(bf_smplx_dyn_row_kernel, dim3((n + 63) / 64), dim3(64), 0, s, m->mesh, (const float *)pass.state.p, n, d_row.p);
    HIP_TRY(hipGetLastError());
    return BF_OK;
}

extern "C" int bf_smplx_vjp_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const bf_smplx_params *in, const float *expression,
                                const bf_smplx_cotangents *cot, const bf_smplx_grads *grads, float *dexpression) {
    const char *who = "bf_smplx_vjp_dev";
    BF_TRY(dev_route_check(m, ws, n, who));
    if (!in || !cot || !grads || !in->betas || !in->global_orient || !in->body_pose || (dexpression && !expression))
        return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 1, who));
    BF_TRY(bf_expr_check(m, expression, who));
    ++bf_route_stats().dev;
    if (!grads->dbetas && !grads->dglobal_orient && !grads->dbody_pose && !grads->djaw_pose && !grads->dleye_pose && !grads->dreye_pose &&
        !grads->dleft_hand_pose && !grads->dright_hand_pose && !dexpression)
        return BF_OK;
    BfDeviceGuard keep;
    HIP_TRY(hipSetDevice(m->device));
    const hipStream_t s = (hipStream_t)stream;
    BF_TRY(ensure_posedirsT_on(m, s));
    const int nj = m->nj, n_pca = m->fit.n_pca, nbp = m->fit.nbp, OUT = 3 * nj + 2 * n_pca;
    const size_t N = (size_t)n;
    BfWsCall call(ws, s);
    BF_TRY(call.begin());
    Inputs x;
    DevBuf<float> d_out;
    ModelPass pass(m, n, s, ws);
    pass.to.dbeta = grads->dbetas; pass.to.dexpr = dexpression;
    x.view(m, N, in);
    BF_TRY(x.assemble(m, N, pass, nullptr));
    BF_TRY(pass.need(d_out, N * OUT));
    BF_TRY(pass.forward(x.beta.p, x.th_root.p, x.th_rest.p, true, expression));
    BF_TRY(pass.reverse(cot->dvertices, cot->djoints, cot->djoints_all, m->n_all, dexpression != nullptr));
    hipLaunchKernelGGL(bf_smplx_pose_reverse_kernel, dim3(n), dim3(64), 0, s, m->fit, (const float *)pass.dtheta.p, cot->dfull_pose, d_out.p);
    HIP_TRY(hipGetLastError());
    return scatter_blocks(d_out.p, n, OUT, {{grads->dglobal_orient, 0, 3}, {grads->dbody_pose, 3, nbp}, {grads->djaw_pose, 3 + nbp, 3},
                                            {grads->dleye_pose, 6 + nbp, 3}, {grads->dreye_pose, 9 + nbp, 3},
                                            {grads->dleft_hand_pose, 3 * nj, n_pca}, {grads->dright_hand_pose, 3 * nj + n_pca, n_pca}}, s);
}
