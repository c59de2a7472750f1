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
// Stateless: nothing stays on the device between calls but the model's lazily built posedirsT.
#include "bf_host.h"
#include "mesh_kernels.h"
#include "model_grad_kernels.h"
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
    DevBuf<int> lmk_vid;
    MeshScratch scratch;
    // (destroyed before the buffers: whatever path leaves the call, no kernel still uses a block when it goes back to the cache)
    DrainOnExit drain;
    ModelPass(bf_model *model, int frames) : m(model), n(frames) {}

    // Model space: no similarity, constant scale 1 - as bf_smpl_forward builds its state, so that the mesh reverse's dvout is dL/dv in
    // model space.  for_reverse: vposed is saved instead of the mapped joints.  An SMPL-X model's joints pass leaves all its joints
    // (jraw) and, for the reverse, every frame's landmark vertices and weights (the contour row of ITS yaw).
    int forward(const float *beta, const float *th_root, const float *th_rest, bool for_reverse) {
        const size_t N = (size_t)n, nv3 = (size_t)m->nv * 3;
        const bool x = m->kind == 1;
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
        mesh.joints = joints.p; mesh.jraw = jraw.p; mesh.lmk_vid = lmk_vid.p; mesh.lmk_w = lmk_w.p;
        return bf_launch_mesh(m, mesh);
    }

    // After forward(..., true): the cotangents on the device (any may be null = zero; ddirect covers the first n_direct joints) ->
    // dtheta[n][3 NJ], dbeta[n][NB], left on the device.  The caller holds the model's posedirsT (bf_ensure_posedirsT_locked).
    int reverse(const float *dvertices, const float *djoints, const float *ddirect, int n_direct) {
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
        // 3. chain + Rodrigues reversed
        hipLaunchKernelGGL(bf_smpl_vjp_chain_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)state.p, (const float *)ext.p, EXT,
                           (const float *)dchain.p, dtheta.p, dbeta.p);
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

extern "C" int bf_smplx_forward(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_outputs *out) {
    if (!m || n <= 0 || !in || !out || !in->betas || !in->global_orient || !in->body_pose)
        return fail(BF_ERR_INVALID, "bf_smplx_forward: bad argument");
    BF_TRY(bf_grad_check(m, 1, "bf_smplx_forward"));
    HIP_TRY(hipSetDevice(m->device));
    const size_t N = (size_t)n;
    Inputs x;
    DevBuf<int> d_row;
    ModelPass pass(m, n);
    BF_TRY(x.upload_and_assemble(m, N, in));
    HIP_TRY(d_row.alloc_pooled(N));
    BF_TRY(pass.forward(x.beta.p, x.th_root.p, x.th_rest.p, false));
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
    if (!m || n <= 0 || !in || !cot || !grads || !in->betas || !in->global_orient || !in->body_pose)
        return fail(BF_ERR_INVALID, "bf_smplx_vjp: bad argument");
    BF_TRY(bf_grad_check(m, 1, "bf_smplx_vjp"));
    if (!grads->dbetas && !grads->dglobal_orient && !grads->dbody_pose && !grads->djaw_pose && !grads->dleye_pose && !grads->dreye_pose &&
        !grads->dleft_hand_pose && !grads->dright_hand_pose)
        return BF_OK;
    HIP_TRY(hipSetDevice(m->device));
    BF_TRY(ensure_posedirsT(m));
    const int nj = m->nj, nb = m->nb, n_pca = m->fit.n_pca, nbp = m->fit.nbp, OUT = 3 * nj + 2 * n_pca;
    const size_t N = (size_t)n;
    Inputs x;
    DevBuf<float> d_dvert, d_dj, d_dja, d_dfull, d_out;
    ModelPass pass(m, n);
    BF_TRY(x.upload_and_assemble(m, N, in));
    if (cot->dvertices) HIP_TRY(d_dvert.upload_pooled(cot->dvertices, N * m->nv * 3));
    if (cot->djoints) HIP_TRY(d_dj.upload_pooled(cot->djoints, N * m->n_joint_map * 3));
    if (cot->djoints_all) HIP_TRY(d_dja.upload_pooled(cot->djoints_all, N * m->n_all * 3));
    if (cot->dfull_pose) HIP_TRY(d_dfull.upload_pooled(cot->dfull_pose, N * 3 * nj));
    HIP_TRY(d_out.alloc_pooled(N * OUT));
    BF_TRY(pass.forward(x.beta.p, x.th_root.p, x.th_rest.p, true));
    BF_TRY(pass.reverse(d_dvert.p, d_dj.p, d_dja.p, m->n_all));
    // the pose assembly reversed
    hipLaunchKernelGGL(bf_smplx_pose_reverse_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)pass.dtheta.p, (const float *)d_dfull.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (grads->dbetas) HIP_TRY(hipMemcpy(grads->dbetas, pass.dbeta.p, N * nb * sizeof(float), hipMemcpyDeviceToHost));
    // full pose order: root | body | jaw | left eye | right eye | hands (through their PCA coefficients, behind the thetas)
    return fetch_blocks(d_out.p, N, OUT, {{grads->dglobal_orient, 0, 3}, {grads->dbody_pose, 3, nbp}, {grads->djaw_pose, 3 + nbp, 3},
                                          {grads->dleye_pose, 6 + nbp, 3}, {grads->dreye_pose, 9 + nbp, 3},
                                          {grads->dleft_hand_pose, 3 * nj, n_pca}, {grads->dright_hand_pose, 3 * nj + n_pca, n_pca}});
}
