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
struct DrainOnExit { ~DrainOnExit() { (void)hipDeviceSynchronize(); } };

// One call's forward and reverse through a body model, and the buffers both run on.  A fitting loop calls these entry points once
// per step: the buffers come from the device's block cache, not from hipMalloc / hipFree.  Whatever else the kernels of a call
// touch is declared BEFORE its ModelPass, so that `drain` has run when those blocks go back to the cache.
struct ModelPass {
    bf_model *const m;
    const int n;
    DevBuf<float> state, vraw, vposed, xpart, joints, jraw, lmk_w, dv, dchain, part, ext, dtheta, dbeta;
    DevBuf<float> dJx, epart, emesh, dexpr;         // with expression coefficients only (expr_kernels.hip)
    const float *expr = nullptr;                    // the coefficients [n][n_expr] on the device: set by a forward that was given them
    DevBuf<int> lmk_vid;
    MeshScratch scratch;
    // (destroyed before the buffers: whatever path leaves the call, no kernel still uses a block when it goes back to the cache)
    DrainOnExit drain;
    ModelPass(bf_model *model, int frames) : m(model), n(frames) {}

    // Model space: no similarity, constant scale 1 - as bf_smpl_forward builds its state, so that the mesh reverse's dvout is dL/dv in
    // model space.  for_reverse: vposed is saved instead of the mapped joints.  An SMPL-X model's joints pass leaves all its joints
    // (jraw) and, for the reverse, every frame's landmark vertices and weights (the contour row of ITS yaw).
    // expression (device, [n][n_expr]; null: none - then the launches are the ones of a model without directions): the chain delta
    // shifts the state's Gt / At in front of the mesh pass, the vertex delta runs between the mesh and the joints pass.
    int forward(const float *beta, const float *th_root, const float *th_rest, bool for_reverse, const float *expression = nullptr) {
        const size_t N = (size_t)n, nv3 = (size_t)m->nv * 3;
        const bool x = m->kind == 1;
        expr = expression;
        HIP_TRY(state.alloc_pooled(N * bf_state_stride(m->nj, m->npf, m->nb)));
        HIP_TRY(vraw.alloc_pooled(N * nv3));
        if (for_reverse) HIP_TRY(vposed.alloc_pooled(N * nv3));
        if (x) {
            HIP_TRY(xpart.alloc_pooled(N * m->mesh.n_tiles * std::max(m->n_extra, 1) * 3));
            HIP_TRY(jraw.alloc_pooled(N * m->n_all * 3));
            if (!for_reverse) HIP_TRY(joints.alloc_pooled(N * m->n_joint_map * 3));
            if (for_reverse) HIP_TRY(lmk_vid.alloc_pooled(N * m->n_lmk * 3));
            if (for_reverse) HIP_TRY(lmk_w.alloc_pooled(N * m->n_lmk * 3));
        }
        hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, 0, m->fit, beta, th_root, th_rest, (const float *)nullptr, state.p,
                           (const float *)nullptr, (const float *)nullptr, 1.0f);
        HIP_TRY(hipGetLastError());
        MeshPass mesh;
        mesh.scr = &scratch; mesh.n = n; mesh.state = state.p;
        mesh.vraw = vraw.p; mesh.xpart = xpart.p; mesh.vposed = vposed.p;
        if (!expr) {
            mesh.joints = joints.p; mesh.jraw = jraw.p; mesh.lmk_vid = lmk_vid.p; mesh.lmk_w = lmk_w.p;
            return bf_launch_mesh(m, mesh);
        }
        const int ne = m->n_expr;
        HIP_TRY(dJx.alloc_pooled(N * m->nj * 3));
        hipLaunchKernelGGL(bf_expr_chain_kernel, dim3(n), dim3(64), 0, 0, m->fit, state.p, expr, ne, (const float *)m->Jx.p, dJx.p);
        HIP_TRY(hipGetLastError());
        BF_TRY(bf_launch_mesh(m, mesh));                          // (no joints asked for: the mesh pass alone)
        hipLaunchKernelGGL(bf_expr_vertex_kernel, dim3((m->nv + 255) / 256, n), dim3(256), 0, 0, m->mesh, (const float *)state.p, expr, ne,
                           (const float *)m->exprT.p, vraw.p, vposed.p);
        HIP_TRY(hipGetLastError());
        if (m->n_extra > 0) {                                     // the extra-regressor joints' per-tile sums, from the updated vertices
            hipLaunchKernelGGL(bf_expr_xpart_kernel, dim3(m->mesh.n_tiles, n), dim3(128), 0, 0, m->mesh, (const float *)vraw.p, xpart.p);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(bf_joints_kernel, dim3(n), dim3(256), 0, 0, m->mesh, (const float *)state.p, (const float *)vraw.p,
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
        HIP_TRY(dv.alloc_pooled(N * nv3));
        HIP_TRY(dchain.alloc_pooled(N * nj * 3));
        HIP_TRY(part.alloc_pooled(N * part_rows * EXT));
        HIP_TRY(ext.alloc_pooled(N * EXT));
        HIP_TRY(dtheta.alloc_pooled(N * nj * 3));
        HIP_TRY(dbeta.alloc_pooled(N * nb));
        // 1. joint cotangents -> dL/dvertices of the mesh reverse, dL/d(posed chain joints)
        hipLaunchKernelGGL(bf_model_vjp_fold_kernel, dim3((nv + 255) / 256, n), dim3(256), 0, 0, m->mesh, dvertices, djoints, ddirect, n_direct,
                           (const int *)lmk_vid.p, (const float *)lmk_w.p, dv.p, dchain.p);
        HIP_TRY(hipGetLastError());
        // 2. the dense schedule's reverse mesh pass (no silhouette fold) and its reduction (no doorbell)
        int rows = m->mesh.n_tiles;
        const int e = bf_mesh_bwd_multi_launch(&m->mesh, m->posedirsT.p, state.p, n, dv.p, vposed.p, vraw.p, part.p, 0,
                                               nullptr, 0, 0, 4, part_rows, &rows, nullptr);
        if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_bwd_multi_kernel: ") + hipGetErrorString((hipError_t)e));
        hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((EXT + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, 0,
                           (const float *)part.p, rows, EXT, ext.p, EXT, (int *)nullptr, 0);
        HIP_TRY(hipGetLastError());
        // (with expression coefficients whose gradient is wanted) E_v^T (sum_j w_vj GR_j^T dv_v) per 256-vertex tile, the tiles in tile order
        const int ne = expr ? m->n_expr : 0, etiles = (nv + 255) / 256;
        const bool dex = expr && want_dexpr;
        if (dex) {
            HIP_TRY(epart.alloc_pooled(N * etiles * ne));
            HIP_TRY(emesh.alloc_pooled(N * ne));
            HIP_TRY(dexpr.alloc_pooled(N * ne));
            hipLaunchKernelGGL(bf_expr_reverse_kernel, dim3(etiles, n), dim3(256), 0, 0, m->mesh, (const float *)state.p, (const float *)dv.p, ne,
                               (const float *)m->exprT.p, epart.p);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((ne + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, 0,
                               (const float *)epart.p, etiles, ne, emesh.p, ne, (int *)nullptr, 0);
            HIP_TRY(hipGetLastError());
        }
        // 3. chain + Rodrigues reversed (the rest joints with Jx psi; dexpression = the vertex part + Jx^T dL/d(rest joints))
        hipLaunchKernelGGL(bf_smpl_vjp_chain_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)state.p, (const float *)ext.p, EXT,
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
    int upload_and_assemble(const bf_model *m, size_t N, const bf_smplx_params *in) {
        const int nj = m->nj, n_pca = m->fit.n_pca;
        HIP_TRY(beta.upload_pooled(in->betas, N * m->nb));
        HIP_TRY(orient.upload_pooled(in->global_orient, N * 3));
        HIP_TRY(body.upload_pooled(in->body_pose, N * m->fit.nbp));
        if (in->jaw_pose) HIP_TRY(jaw.upload_pooled(in->jaw_pose, N * 3));
        if (in->leye_pose) HIP_TRY(leye.upload_pooled(in->leye_pose, N * 3));
        if (in->reye_pose) HIP_TRY(reye.upload_pooled(in->reye_pose, N * 3));
        if (in->left_hand_pose) HIP_TRY(lh.upload_pooled(in->left_hand_pose, N * n_pca));
        if (in->right_hand_pose) HIP_TRY(rh.upload_pooled(in->right_hand_pose, N * n_pca));
        HIP_TRY(full.alloc_pooled(N * 3 * nj));
        HIP_TRY(th_root.alloc_pooled(N * 3));
        HIP_TRY(th_rest.alloc_pooled(N * 3 * (nj - 1)));
        hipLaunchKernelGGL(bf_smplx_pose_assemble_kernel, dim3((unsigned)N), dim3(64), 0, 0, m->fit, (const float *)orient.p, (const float *)body.p,
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
    HIP_TRY(hipSetDevice(m->device));
    const size_t N = (size_t)n;
    Inputs x;
    DevBuf<int> d_row;
    DevBuf<float> d_expr;
    ModelPass pass(m, n);
    BF_TRY(x.upload_and_assemble(m, N, in));
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
    BF_TRY(x.upload_and_assemble(m, N, in));
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
