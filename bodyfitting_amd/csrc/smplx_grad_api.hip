// Host side of bf_smplx_forward / bf_smplx_vjp (include/bodyfit.h): smplx.create(model_type='smplx', ...)'s forward as the reference
// calls it (smplify.py:177-190) and the reverse torch.autograd runs through it, on the dense schedule's mesh passes.
//   forward: bf_smplx_pose_assemble_kernel (blocks -> full_pose) -> bf_pose_state_kernel's non-packed path -> the mesh pass and
//            bf_joints_kernel exactly as bf_model_forward launches them (+ the 144 joints) -> bf_smplx_dyn_row_kernel
//   reverse: 1. the forward recomputed, saving the pose-blended vertices and the landmarks' vertices / weights of every frame
//            2. bf_smplx_vjp_fold_kernel: the joint cotangents onto the vertices (selector, landmarks) and the posed chain joints
//            3. bf_mesh_bwd_multi_launch + bf_ext_reduce_kernel, unchanged (no mask fold, no doorbell)
//            4. bf_smpl_vjp_chain_kernel, unchanged (table-driven, one lane per joint: 55 of its 64) -> dtheta, dbeta
//            5. bf_smplx_pose_reverse_kernel: dtheta (+ dfull_pose) -> the parameter blocks
// Stateless: nothing stays on the device between calls but the model's lazily built posedirsT.
#include "bf_host.h"

extern "C" __global__ void bf_pose_state_kernel(FitTab, const float *, const float *, const float *, const float *, float *, const float *, const float *, float);
extern "C" int bf_mesh_bwd_multi_launch(const MeshTab *, const float *, const float *, int, const float *, const float *, const float *, float *, hipStream_t,
                                        const float *, int, int, int, int, int *, const MaskFold *);
extern "C" __global__ void bf_ext_reduce_kernel(const float *, int, int, float *, int, int *, int);
extern "C" __global__ void bf_smpl_vjp_chain_kernel(FitTab, const float *, const float *, int, const float *, float *, float *);
extern "C" __global__ void bf_smplx_pose_assemble_kernel(FitTab, const float *, const float *, const float *, const float *, const float *, const float *,
                                                         const float *, float *, float *, float *);
extern "C" __global__ void bf_smplx_dyn_row_kernel(MeshTab, const float *, int, int *);
extern "C" __global__ void bf_smplx_vjp_fold_kernel(MeshTab, const float *, const float *, const float *, const int *, const float *, float *, float *);
extern "C" __global__ void bf_smplx_pose_reverse_kernel(FitTab, const float *, const float *, float *);

// (the limits of the kernels' LDS tables, smplx_grad_kernels.hip / smpl_grad_kernels.hip)
static constexpr int kMaxAll = 192, kMaxMap = 256, kMaxSel = 64, kMaxLmk = 96, kMaxNp = 128, kMaxJoints = 64;

static int check_model(const bf_model *m, const char *who) {
    if (m->kind != 1) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": SMPL-X-kind models only");
    if (m->nj > kMaxJoints || m->n_all > kMaxAll || m->n_selector > kMaxSel || m->n_lmk > kMaxLmk || m->n_joint_map > kMaxMap ||
        m->np > kMaxNp || m->n_all != m->nj + m->n_selector + m->n_extra + m->n_lmk)
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": model larger than the kernels' tables");
    return BF_OK;
}

namespace {
// the parameter blocks on the device and the thetas assembled from them
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
struct DrainOnExit { ~DrainOnExit() { (void)hipDeviceSynchronize(); } };
}  // namespace

extern "C" int bf_smplx_forward(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_outputs *out) {
    if (!m || n <= 0 || !in || !out || !in->betas || !in->global_orient || !in->body_pose)
        return fail(BF_ERR_INVALID, "bf_smplx_forward: bad argument");
    BF_TRY(check_model(m, "bf_smplx_forward"));
    HIP_TRY(hipSetDevice(m->device));
    const int nj = m->nj, nb = m->nb, nv = m->nv;
    const size_t N = (size_t)n;
    Inputs x;
    DevBuf<float> d_state, d_vraw, d_j, d_jall, d_xp;
    DevBuf<int> d_row;
    MeshScratch scratch;
    // (destroyed before the buffers: whatever path leaves this function, no kernel still uses a block when it goes back to the cache)
    DrainOnExit drain;
    BF_TRY(x.upload_and_assemble(m, N, in));
    HIP_TRY(d_state.alloc_pooled(N * bf_state_stride(nj, m->npf, nb)));
    HIP_TRY(d_vraw.alloc_pooled(N * nv * 3));
    HIP_TRY(d_j.alloc_pooled(N * m->n_joint_map * 3));
    HIP_TRY(d_jall.alloc_pooled(N * m->n_all * 3));
    HIP_TRY(d_xp.alloc_pooled(N * m->mesh.n_tiles * std::max(m->n_extra, 1) * 3));
    HIP_TRY(d_row.alloc_pooled(N));
    // model space: no similarity, constant scale 1
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, 0, m->fit, (const float *)x.beta.p, (const float *)x.th_root.p,
                       (const float *)x.th_rest.p, (const float *)nullptr, d_state.p, (const float *)nullptr, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    BF_TRY(bf_launch_mesh(m, &scratch, n, d_state.p, d_vraw.p, nullptr, d_xp.p, d_j.p, nullptr, 0, nullptr, nullptr, d_jall.p));
    hipLaunchKernelGGL(bf_smplx_dyn_row_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, m->mesh, (const float *)d_state.p, n, d_row.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (out->vertices) HIP_TRY(hipMemcpy(out->vertices, d_vraw.p, N * nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->joints) HIP_TRY(hipMemcpy(out->joints, d_j.p, N * m->n_joint_map * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->joints_all) HIP_TRY(hipMemcpy(out->joints_all, d_jall.p, N * m->n_all * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->full_pose) HIP_TRY(hipMemcpy(out->full_pose, x.full.p, N * 3 * nj * sizeof(float), hipMemcpyDeviceToHost));
    if (out->dyn_row) HIP_TRY(hipMemcpy(out->dyn_row, d_row.p, N * sizeof(int), hipMemcpyDeviceToHost));
    return BF_OK;
}

extern "C" int bf_smplx_vjp(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_cotangents *cot, const bf_smplx_grads *grads) {
    if (!m || n <= 0 || !in || !cot || !grads || !in->betas || !in->global_orient || !in->body_pose)
        return fail(BF_ERR_INVALID, "bf_smplx_vjp: bad argument");
    BF_TRY(check_model(m, "bf_smplx_vjp"));
    const int nj = m->nj, nb = m->nb, nv = m->nv, npf = m->npf, n_pca = m->fit.n_pca, nbp = m->fit.nbp, nlm = m->n_lmk;
    if (!grads->dbetas && !grads->dglobal_orient && !grads->dbody_pose && !grads->djaw_pose && !grads->dleye_pose && !grads->dreye_pose &&
        !grads->dleft_hand_pose && !grads->dright_hand_pose)
        return BF_OK;
    HIP_TRY(hipSetDevice(m->device));
    {
        std::lock_guard<std::mutex> g(m->lazy);
        BF_TRY(bf_ensure_posedirsT_locked(m, nullptr));
    }
    const size_t N = (size_t)n, nv3 = (size_t)nv * 3;
    const size_t stride = bf_state_stride(nj, npf, nb);
    const int EXT = npf + nj * 12 + nb + 4, OUT = 3 * nj + 2 * n_pca;
    // (one frame: room for the split single-frame instance of the mesh reverse, two partial rows per tile)
    const int part_rows = (n == 1 ? 2 : 1) * m->mesh.n_tiles;
    // (a fitting loop calls this once per step: the buffers come from the device's block cache, not from hipMalloc / hipFree)
    Inputs x;
    DevBuf<float> d_state, d_vraw, d_vposed, d_xp, d_jall, d_lw, d_dvert, d_dj, d_dja, d_dfull, d_dv, d_dchain, d_part, d_ext, d_dth, d_db, d_out;
    DevBuf<int> d_lv;
    MeshScratch scratch;
    DrainOnExit drain;
    BF_TRY(x.upload_and_assemble(m, N, in));
    if (cot->dvertices) HIP_TRY(d_dvert.upload_pooled(cot->dvertices, N * nv3));
    if (cot->djoints) HIP_TRY(d_dj.upload_pooled(cot->djoints, N * m->n_joint_map * 3));
    if (cot->djoints_all) HIP_TRY(d_dja.upload_pooled(cot->djoints_all, N * m->n_all * 3));
    if (cot->dfull_pose) HIP_TRY(d_dfull.upload_pooled(cot->dfull_pose, N * 3 * nj));
    HIP_TRY(d_state.alloc_pooled(N * stride));
    HIP_TRY(d_vraw.alloc_pooled(N * nv3));
    HIP_TRY(d_vposed.alloc_pooled(N * nv3));
    HIP_TRY(d_xp.alloc_pooled(N * m->mesh.n_tiles * std::max(m->n_extra, 1) * 3));
    HIP_TRY(d_jall.alloc_pooled(N * m->n_all * 3));
    HIP_TRY(d_lv.alloc_pooled(N * nlm * 3));
    HIP_TRY(d_lw.alloc_pooled(N * nlm * 3));
    HIP_TRY(d_dv.alloc_pooled(N * nv3));
    HIP_TRY(d_dchain.alloc_pooled(N * nj * 3));
    HIP_TRY(d_part.alloc_pooled(N * part_rows * EXT));
    HIP_TRY(d_ext.alloc_pooled(N * EXT));
    HIP_TRY(d_dth.alloc_pooled(N * nj * 3));
    HIP_TRY(d_db.alloc_pooled(N * nb));
    HIP_TRY(d_out.alloc_pooled(N * OUT));
    // 1. forward recompute: the mesh reverse's dvout is then dL/dv in model space; the joints pass leaves every frame's landmark
    //    vertices and weights (the contour row of ITS yaw)
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, 0, m->fit, (const float *)x.beta.p, (const float *)x.th_root.p,
                       (const float *)x.th_rest.p, (const float *)nullptr, d_state.p, (const float *)nullptr, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    BF_TRY(bf_launch_mesh(m, &scratch, n, d_state.p, d_vraw.p, nullptr, d_xp.p, nullptr, nullptr, 0, nullptr, d_vposed.p, d_jall.p, d_lv.p, d_lw.p));
    // 2. joint cotangents -> dL/dvertices of the mesh reverse, dL/d(posed chain joints)
    hipLaunchKernelGGL(bf_smplx_vjp_fold_kernel, dim3((nv + 255) / 256, n), dim3(256), 0, 0, m->mesh, (const float *)d_dvert.p,
                       (const float *)d_dj.p, (const float *)d_dja.p, (const int *)d_lv.p, (const float *)d_lw.p, d_dv.p, d_dchain.p);
    HIP_TRY(hipGetLastError());
    // 3. the dense schedule's reverse mesh pass (no silhouette fold) and its reduction (no doorbell)
    int rows = m->mesh.n_tiles;
    const int e = bf_mesh_bwd_multi_launch(&m->mesh, m->posedirsT.p, d_state.p, n, d_dv.p, d_vposed.p, d_vraw.p, d_part.p, 0,
                                           nullptr, 0, 0, 4, part_rows, &rows, nullptr);
    if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_bwd_multi_kernel: ") + hipGetErrorString((hipError_t)e));
    hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((EXT + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, 0,
                       (const float *)d_part.p, rows, EXT, d_ext.p, EXT, (int *)nullptr, 0);
    HIP_TRY(hipGetLastError());
    // 4. chain + Rodrigues reversed, 5. pose assembly reversed
    hipLaunchKernelGGL(bf_smpl_vjp_chain_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)d_state.p, (const float *)d_ext.p, EXT,
                       (const float *)d_dchain.p, d_dth.p, d_db.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bf_smplx_pose_reverse_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)d_dth.p, (const float *)d_dfull.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (grads->dbetas) HIP_TRY(hipMemcpy(grads->dbetas, d_db.p, N * nb * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> g(N * OUT);
    HIP_TRY(hipMemcpy(g.data(), d_out.p, g.size() * sizeof(float), hipMemcpyDeviceToHost));
    // full pose order: root | body | jaw | left eye | right eye | hands (through their PCA coefficients, behind the thetas)
    const struct { float *dst; int off, cnt; } blocks[] = {
        {grads->dglobal_orient, 0, 3}, {grads->dbody_pose, 3, nbp}, {grads->djaw_pose, 3 + nbp, 3}, {grads->dleye_pose, 6 + nbp, 3},
        {grads->dreye_pose, 9 + nbp, 3}, {grads->dleft_hand_pose, 3 * nj, n_pca}, {grads->dright_hand_pose, 3 * nj + n_pca, n_pca}};
    for (const auto &b : blocks)
        if (b.dst)
            for (size_t f = 0; f < N; ++f) std::memcpy(b.dst + f * b.cnt, g.data() + f * OUT + b.off, b.cnt * sizeof(float));
    return BF_OK;
}
