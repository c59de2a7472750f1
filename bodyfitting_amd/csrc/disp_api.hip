// Host side of the SMPL+D stage (smplify.py:228-247): the per-vertex displacement loop against the attached scans.
#include "bf_host.h"
#include "disp_kernels.h"
#include "scan_kernels.h"

extern "C" {
int bf_fit_displacement(bf_batch *b, int n_iters, const bf_hyper *hyper) {
    if (!b || n_iters <= 0) return fail(BF_ERR_INVALID, "bf_fit_displacement: bad argument");
    bf_model *m = b->m;
    if (b->scans_lost)
        return fail(BF_ERR_INVALID, "bf_fit_displacement: a scan this batch held was destroyed (bf_scan_destroy) - call bf_batch_set_scans again");
    if (b->scans.empty()) return fail(BF_ERR_INVALID, "bf_fit_displacement: no scans attached (bf_batch_set_scans)");
    if (!b->have_result) return fail(BF_ERR_INVALID, "bf_fit_displacement: run bf_fit first (the stage starts from its vertices)");
    if (m->faces_host.empty()) return fail(BF_ERR_INVALID, "bf_fit_displacement: the model was created without faces");
    HIP_TRY(hipSetDevice(m->device));
    bf_hyper h;
    if (hyper) h = *hyper; else bf_hyper_default(&h);
    const int F = b->F, nv = m->nv, nf = (int)m->faces_host.size() / 3;
    BF_TRY(bf_guard_arena(b));
    std::unique_lock<std::mutex> lazy(m->lazy);
    if (!m->topo.built()) HIP_TRY(m->topo.build(m->faces_host, nv));
    lazy.unlock();
    const size_t nv3 = (size_t)F * nv * 3;
    if (!b->disp.p) {
        bool ok = b->disp.alloc(nv3) == hipSuccess && b->disp_m.alloc(nv3) == hipSuccess && b->disp_v.alloc(nv3) == hipSuccess &&
                  b->disp_base.alloc(nv3) == hipSuccess && b->disp_P.alloc(nv3) == hipSuccess && b->disp_dv.alloc(nv3) == hipSuccess &&
                  b->disp_fn.alloc((size_t)F * nf * 4) == hipSuccess && b->disp_vn.alloc((size_t)F * nv * 4) == hipSuccess &&
                  b->disp_dPf.alloc((size_t)F * nf * 9) == hipSuccess;
        if (!ok) return fail(BF_ERR_HIP, "bf_fit_displacement: device allocation failed");
    }
    // zeros for disp and its moments; the base is the mesh of the last forward, detached (smplify.py:229-231)
    HIP_TRY(hipMemsetAsync(b->disp.p, 0, nv3 * sizeof(float), b->stream));
    HIP_TRY(hipMemsetAsync(b->disp_m.p, 0, nv3 * sizeof(float), b->stream));
    HIP_TRY(hipMemsetAsync(b->disp_v.p, 0, nv3 * sizeof(float), b->stream));
    HIP_TRY(hipMemcpyAsync(b->disp_base.p, b->vout.p, nv3 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
    const dim3 gv((nv + 255) / 256, F), gf((nf + 255) / 256, F);
    const int *faces = m->topo.faces.p, *adj_start = m->topo.adj_start.p, *adj = m->topo.adj.p;
    const int nblk = (nv + 255) / 256;
    const double b1 = h.adam_beta1, b2 = h.adam_beta2;
    for (int it = 1; it <= n_iters; ++it) {
        hipLaunchKernelGGL(bf_disp_face_kernel, gf, dim3(256), 0, b->stream, faces, nf, nv,
                           (const float *)b->disp_base.p, (const float *)b->disp.p, b->disp_fn.p);
        hipLaunchKernelGGL(bf_disp_vertex_kernel, gv, dim3(256), 0, b->stream, adj_start, adj, nf, nv,
                           (const float *)b->disp_base.p, (const float *)b->disp.p, (const float *)b->disp_fn.p, b->disp_P.p, b->disp_vn.p);
        bf_nearest_launch(dim3((nv + 3) / 4, F), b->stream, (const ScanDev *)b->scan_dev.p, (const float *)b->disp_P.p, nv,
                          b->cface.p, b->cpts.p, (float *)nullptr, b->cface_valid ? 1 : 0);
        b->cface_valid = true;
        hipLaunchKernelGGL(bf_disp_vgrad_kernel, gv, dim3(256), 0, b->stream, faces, adj_start, adj, nf, nv,
                           (const float *)b->disp_vn.p, (const float *const *)b->scan_fn.p,
                           (const int *)b->cface.p, (const float *)b->cscale.p, b->disp_dv.p, (const float *)b->disp_P.p,
                           (const float *)b->cpts.p, b->pc_partial.p);      // (+ the block sums of |P - C|^2: was bf_pc_partial_kernel)
        hipLaunchKernelGGL(bf_disp_fgrad_kernel, gf, dim3(256), 0, b->stream, faces, nf, nv, (const float *)b->disp_P.p,
                           (const float *)b->disp_fn.p, (const float *)b->disp_dv.p, b->disp_dPf.p);
        const float step_size = (float)((double)h.lr_displacement / (1.0 - std::pow(b1, it)));
        const float bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, it));
        hipLaunchKernelGGL(bf_disp_adam_kernel, gv, dim3(256), 0, b->stream, adj_start, adj, nf, nv,
                           (const float *)b->disp_P.p, (const float *)b->cpts.p, (const float *)b->pc_partial.p, nblk,
                           (const float *)b->disp_dPf.p, b->disp.p, b->disp_m.p, b->disp_v.p, step_size, bc2_sqrt, h.adam_beta1,
                           h.adam_beta2, h.adam_eps);
        HIP_TRY(hipGetLastError());
    }
    b->have_disp = true;
    return BF_OK;
}

int bf_batch_get_displacement(bf_batch *b, float *displacement) {
    if (!b || !displacement) return fail(BF_ERR_INVALID, "bf_batch_get_displacement: null argument");
    if (!b->have_disp) return fail(BF_ERR_INVALID, "bf_batch_get_displacement: no bf_fit_displacement yet");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(displacement, b->disp.p, b->disp.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

/* test hook: first Adam moment of the displacement (after one step it is 0.1 x the gradient) */
int bf_batch_debug_disp_moment(bf_batch *b, float *m_out) {
    if (!b || !m_out || !b->have_disp) return fail(BF_ERR_INVALID, "bf_batch_debug_disp_moment: bad argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(m_out, b->disp_m.p, b->disp_m.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

/* test hook: second Adam moment of the displacement */
int bf_batch_debug_disp_moment2(bf_batch *b, float *v_out) {
    if (!b || !v_out || !b->have_disp) return fail(BF_ERR_INVALID, "bf_batch_debug_disp_moment2: bad argument");
    HIP_TRY(hipSetDevice(b->m->device));
    BF_TRY(bf_sync_all(b));
    HIP_TRY(hipMemcpy(v_out, b->disp_v.p, b->disp_v.n * sizeof(float), hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
