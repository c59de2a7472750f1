// Host side of bf_smpl_vjp (include/bodyfit.h): the reverse of models.smpl.SMPL.forward that torch.autograd runs through
// smplx's lbs() and models/smpl.py:69-83, on the dense schedule's reverse mesh pass.
//   1. forward recompute: bf_pose_state_kernel (no similarity, constant scale 1) + the mesh pass, saving the pose-blended vertices
//   2. bf_smpl_vjp_fold_kernel: the joint cotangents onto the vertices (selector, J_regressor_extra) and the posed chain joints
//   3. bf_mesh_bwd_multi_launch + bf_ext_reduce_kernel, unchanged: dfeat | skinning sums per joint | dbeta | dt ds per frame
//   4. bf_smpl_vjp_chain_kernel: the kinematic chain and Rodrigues reversed -> dtheta, dbeta
// Stateless: nothing stays on the device between calls but the model's lazily built posedirsT.
#include "bf_host.h"

extern "C" __global__ void bf_pose_state_kernel(FitTab, const float *, const float *, const float *, const float *, float *, const float *, const float *, float);
extern "C" int bf_mesh_bwd_multi_launch(const MeshTab *, const float *, const float *, int, const float *, const float *, const float *, float *, hipStream_t,
                                        const float *, int, int, int, int, int *, const MaskFold *);
extern "C" __global__ void bf_ext_reduce_kernel(const float *, int, int, float *, int, int *, int);
extern "C" __global__ void bf_smpl_vjp_fold_kernel(MeshTab, const float *, const float *, const float *, float *, float *);
extern "C" __global__ void bf_smpl_vjp_chain_kernel(FitTab, const float *, const float *, int, const float *, float *, float *);

// (the limits of the two kernels' LDS tables, smpl_grad_kernels.hip)
static constexpr int kMaxAll = 128, kMaxMap = 256, kMaxJoints = 64;

extern "C" int bf_smpl_vjp(bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                           const float *dvertices, const float *djoints, const float *djoints_ori,
                           float *dbetas, float *dglobal_orient, float *dbody_pose) {
    if (!m || n <= 0 || !betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, "bf_smpl_vjp: bad argument");
    if (m->kind != 0) return fail(BF_ERR_UNSUPPORTED, "bf_smpl_vjp: SMPL-kind models only");
    const int nj = m->nj, nb = m->nb, nv = m->nv, npf = m->npf;
    if (nj > kMaxJoints || nj + m->n_selector + m->n_extra > kMaxAll || m->n_selector > kMaxAll || m->n_joint_map > kMaxMap)
        return fail(BF_ERR_UNSUPPORTED, "bf_smpl_vjp: model larger than the reverse kernels' tables");
    if (!dbetas && !dglobal_orient && !dbody_pose) return BF_OK;
    HIP_TRY(hipSetDevice(m->device));
    {
        std::lock_guard<std::mutex> g(m->lazy);
        int rc = bf_ensure_posedirsT_locked(m, nullptr);
        if (rc) return rc;
    }
    const size_t N = (size_t)n, nv3 = (size_t)nv * 3;
    const size_t stride = bf_state_stride(nj, npf, nb);
    const int EXT = npf + nj * 12 + nb + 4;
    // (one frame: room for the split single-frame instance of the mesh reverse, two partial rows per tile)
    const int part_rows = (n == 1 ? 2 : 1) * m->mesh.n_tiles;
    // (a fitting loop calls this once per step: the buffers come from the device's block cache, not from hipMalloc / hipFree)
    DevBuf<float> d_beta, d_or, d_bp, d_state, d_vraw, d_vposed, d_dvert, d_dj, d_djo, d_dv, d_dchain, d_part, d_ext, d_dth, d_db;
    MeshScratch scratch;
    // (destroyed before the buffers: whatever path leaves this function, no kernel still uses a block when it goes back to the cache)
    struct DrainOnExit { ~DrainOnExit() { (void)hipDeviceSynchronize(); } } drain;
    HIP_TRY(d_beta.upload_pooled(betas, N * nb));
    HIP_TRY(d_or.upload_pooled(global_orient, N * 3));
    HIP_TRY(d_bp.upload_pooled(body_pose, N * 3 * (nj - 1)));
    if (dvertices) HIP_TRY(d_dvert.upload_pooled(dvertices, N * nv3));
    if (djoints) HIP_TRY(d_dj.upload_pooled(djoints, N * m->n_joint_map * 3));
    if (djoints_ori) HIP_TRY(d_djo.upload_pooled(djoints_ori, N * (nj + m->n_selector) * 3));
    HIP_TRY(d_state.alloc_pooled(N * stride));
    HIP_TRY(d_vraw.alloc_pooled(N * nv3));
    HIP_TRY(d_vposed.alloc_pooled(N * nv3));
    HIP_TRY(d_dv.alloc_pooled(N * nv3));
    HIP_TRY(d_dchain.alloc_pooled(N * nj * 3));
    HIP_TRY(d_part.alloc_pooled(N * part_rows * EXT));
    HIP_TRY(d_ext.alloc_pooled(N * EXT));
    HIP_TRY(d_dth.alloc_pooled(N * nj * 3));
    HIP_TRY(d_db.alloc_pooled(N * nb));
    // 1. forward recompute, as bf_smpl_forward builds its state: the mesh reverse's dvout is then dL/dv in model space
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, 0, m->fit, (const float *)d_beta.p,
                       (const float *)d_or.p, (const float *)d_bp.p, (const float *)nullptr, d_state.p,
                       (const float *)nullptr, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    int rc = bf_launch_mesh(m, &scratch, n, d_state.p, d_vraw.p, nullptr, nullptr, nullptr, nullptr, 0, nullptr, d_vposed.p);
    if (rc) return rc;
    // 2. joint cotangents -> dL/dvertices of the mesh reverse, dL/d(posed chain joints)
    hipLaunchKernelGGL(bf_smpl_vjp_fold_kernel, dim3((nv + 255) / 256, n), dim3(256), 0, 0, m->mesh, (const float *)d_dvert.p,
                       (const float *)d_dj.p, (const float *)d_djo.p, d_dv.p, d_dchain.p);
    HIP_TRY(hipGetLastError());
    // 3. the dense schedule's reverse mesh pass (no silhouette fold) and its reduction (no doorbell)
    int rows = m->mesh.n_tiles;
    const int e = bf_mesh_bwd_multi_launch(&m->mesh, m->posedirsT.p, d_state.p, n, d_dv.p, d_vposed.p, d_vraw.p, d_part.p, 0,
                                           nullptr, 0, 0, 4, part_rows, &rows, nullptr);
    if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_bwd_multi_kernel: ") + hipGetErrorString((hipError_t)e));
    hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((EXT + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, 0,
                       (const float *)d_part.p, rows, EXT, d_ext.p, EXT, (int *)nullptr, 0);
    HIP_TRY(hipGetLastError());
    // 4. chain + Rodrigues reversed
    hipLaunchKernelGGL(bf_smpl_vjp_chain_kernel, dim3(n), dim3(64), 0, 0, m->fit, (const float *)d_state.p, (const float *)d_ext.p, EXT,
                       (const float *)d_dchain.p, d_dth.p, d_db.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (dbetas) HIP_TRY(hipMemcpy(dbetas, d_db.p, N * nb * sizeof(float), hipMemcpyDeviceToHost));
    if (dglobal_orient || dbody_pose) {
        std::vector<float> th(N * nj * 3);
        HIP_TRY(hipMemcpy(th.data(), d_dth.p, th.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t f = 0; f < N; ++f) {
            const float *t = th.data() + f * nj * 3;
            if (dglobal_orient) std::memcpy(dglobal_orient + f * 3, t, 3 * sizeof(float));
            if (dbody_pose) std::memcpy(dbody_pose + f * 3 * (nj - 1), t + 3, 3 * (nj - 1) * sizeof(float));
        }
    }
    return BF_OK;
}
