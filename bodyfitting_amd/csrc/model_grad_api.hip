// Host side of bf_smpl_forward, bf_smpl_vjp, bf_smplx_forward and bf_smplx_vjp (include/bodyfit.h): models.smpl.SMPL.forward, the reverse
// torch.autograd runs through it (smplx's lbs() and models/smpl.py:69-83), smplx.create(model_type='smplx', ...)'s forward as the reference
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
// A shape space (bf_model_set_shape_space: betas beyond the tenth, up to 100 expression coefficients) rides the same way: the model's
// passes see the ten core betas, and a frame's extension coefficients [betas[10:], expression] take expression's place.
// bf_shape_ext_pack_kernel cuts the caller's rows into those two blocks, bf_shape_ext_join_kernel puts the two gradients back into rows
// for deliver_blocks; up to BF_EXPR_MAX directions run on expr_kernels.hip's kernels, more (bf_model::ext_wide) on shape_ext_kernels.hip's.
// Stateless: nothing stays on the device between calls but the model's lazily built posedirsT.
// Every operation is ONE body on a BfRouteCall (dev_route.h); its host entry point and its *_dev twin check their arguments, count
// their route and hand the body their call.  The launches, their order, grids and arguments are the same on both routes; what differs
// is where the arrays live (host arrays and the block cache's buffers, or device pointers and workspace slots), the stream (the NULL
// stream, or the caller's) and the end: the host route drains the device and copies, the device route waits for nothing and cuts the
// gradient rows into the caller's blocks with bf_block_scatter_kernel.
#include "bf_host.h"
#include "dev_route.h"
#include "mesh_kernels.h"
#include "model_grad_kernels.h"
#include "expr_kernels.h"
#include "shape_ext_kernels.h"
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
// One call's forward and reverse through a body model on a BfRouteCall, which owns every buffer both run on: a fitting loop calls
// these entry points once per step, so the host route's buffers come from the device's block cache, not from hipMalloc / hipFree, and
// the device route's from the caller's workspace.  An output the caller wants (`to`: a host array on the host route, a device array on
// the device route) is written where the caller wants it, or copied there when the call finishes.
struct ModelPass {
    bf_model *const m;
    const int n;
    BfRouteCall &c;
    struct { float *vraw = nullptr, *joints = nullptr, *jraw = nullptr, *dbeta = nullptr, *dexpr = nullptr; } to;      // the caller's arrays
    float *state = nullptr, *vraw = nullptr, *vposed = nullptr, *xpart = nullptr, *joints = nullptr, *jraw = nullptr, *lmk_w = nullptr;
    float *dv = nullptr, *dchain = nullptr, *part = nullptr, *ext = nullptr, *dtheta = nullptr, *dbeta = nullptr;
    float *dJx = nullptr, *epart = nullptr, *emesh = nullptr, *dexpr = nullptr;         // with expression coefficients only (expr_kernels.hip)
    const float *expr = nullptr;                    // the extension coefficients [n][n_ext] on the device: set by a forward that was given them
    int *lmk_vid = nullptr;
    ModelPass(bf_model *model, int frames, BfRouteCall &call) : m(model), n(frames), c(call) {}

    // `count` elements for p, which the kernels write whoever wants them: the caller's array `target` gets them when there is one
    template <class T>
    int need(T *&p, size_t count, T *target = nullptr) { return c.out(target, count, p, true); }
    // the mesh pass, and the workspace scratch's growth counted with the workspace's other allocations
    int launch_mesh(const MeshPass &mesh) {
        const MeshScratch *s = mesh.scr;
        const float *a = s->pose_off.p, *b = s->featT.p;
        const int rc = bf_launch_mesh(m, mesh);
        if (c.ws) bf_route_stats().allocs += (s->pose_off.p != a) + (s->featT.p != b);
        return rc;
    }

    // Model space: no similarity, constant scale 1 - as smpl_forward builds its state, so that the mesh reverse's dvout is dL/dv in
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
        hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, c.stream, m->fit, beta, th_root, th_rest, (const float *)nullptr, state,
                           (const float *)nullptr, (const float *)nullptr, 1.0f);
        HIP_TRY(hipGetLastError());
        MeshPass mesh;
        mesh.scr = c.mesh_scratch(); mesh.n = n; mesh.state = state; mesh.stream = c.stream;
        mesh.vraw = vraw; mesh.xpart = xpart; mesh.vposed = vposed;
        if (!expr) {
            mesh.joints = joints; mesh.jraw = jraw; mesh.lmk_vid = lmk_vid; mesh.lmk_w = lmk_w;
            return launch_mesh(mesh);
        }
        const int ne = m->n_ext, fblocks = (n + BF_EXT_FB - 1) / BF_EXT_FB;
        BF_TRY(need(dJx, N * m->nj * 3));
        if (m->ext_wide)
            hipLaunchKernelGGL(bf_shape_ext_chain_kernel, dim3(n), dim3(256), 0, c.stream, m->fit, state, expr, ne, (const float *)m->JxT.p, dJx);
        else
            hipLaunchKernelGGL(bf_expr_chain_kernel, dim3(n), dim3(64), 0, c.stream, m->fit, state, expr, ne, (const float *)m->Jx.p, dJx);
        HIP_TRY(hipGetLastError());
        BF_TRY(launch_mesh(mesh));                             // (no joints asked for: the mesh pass alone)
        if (m->ext_wide)
            hipLaunchKernelGGL(bf_shape_ext_vertex_kernel, dim3((m->nv + 255) / 256, fblocks), dim3(256), 0, c.stream, m->mesh, (const float *)state,
                               expr, ne, n, (const float *)m->exprT.p, vraw, vposed);
        else
            hipLaunchKernelGGL(bf_expr_vertex_kernel, dim3((m->nv + 255) / 256, n), dim3(256), 0, c.stream, m->mesh, (const float *)state, expr, ne,
                               (const float *)m->exprT.p, vraw, vposed);
        HIP_TRY(hipGetLastError());
        if (m->n_extra > 0) {                                     // the extra-regressor joints' per-tile sums, from the updated vertices
            hipLaunchKernelGGL(bf_expr_xpart_kernel, dim3(m->mesh.n_tiles, n), dim3(128), 0, c.stream, m->mesh, (const float *)vraw, xpart);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(bf_joints_kernel, dim3(n), dim3(256), 0, c.stream, m->mesh, (const float *)state, (const float *)vraw,
                           (const float *)xpart, joints, (float *)nullptr, jraw, lmk_vid, lmk_w, BfHandOver{});
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
        hipLaunchKernelGGL(bf_model_vjp_fold_kernel, dim3((nv + 255) / 256, n), dim3(256), 0, c.stream, m->mesh, dvertices, djoints, ddirect, n_direct,
                           (const int *)lmk_vid, (const float *)lmk_w, dv, dchain);
        HIP_TRY(hipGetLastError());
        // 2. the dense schedule's reverse mesh pass (no silhouette fold) and its reduction (no doorbell)
        int rows = m->mesh.n_tiles;
        const int e = bf_mesh_bwd_multi_launch(&m->mesh, m->posedirsT.p, state, n, dv, vposed, vraw, part, c.stream,
                                               nullptr, 0, 0, 4, part_rows, &rows, nullptr);
        if (e) return fail(BF_ERR_HIP, std::string("bf_mesh_bwd_multi_kernel: ") + hipGetErrorString((hipError_t)e));
        hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((EXT + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, c.stream,
                           (const float *)part, rows, EXT, ext, EXT, (int *)nullptr, 0);
        HIP_TRY(hipGetLastError());
        // (with expression coefficients whose gradient is wanted) E_v^T (sum_j w_vj GR_j^T dv_v) per 256-vertex tile, the tiles in tile order
        const int ne = expr ? m->n_ext : 0, etiles = (nv + 255) / 256;
        const bool dex = expr && want_dexpr;
        if (dex) {
            BF_TRY(need(epart, N * etiles * ne));
            BF_TRY(need(emesh, N * ne));
            BF_TRY(need(dexpr, N * ne, to.dexpr));
            if (m->ext_wide)
                hipLaunchKernelGGL(bf_shape_ext_reverse_kernel, dim3(etiles, (n + BF_EXT_FB - 1) / BF_EXT_FB), dim3(256), 0, c.stream, m->mesh,
                                   (const float *)state, (const float *)dv, ne, n, (const float *)m->extVK.p, epart);
            else
                hipLaunchKernelGGL(bf_expr_reverse_kernel, dim3(etiles, n), dim3(256), 0, c.stream, m->mesh, (const float *)state, (const float *)dv, ne,
                                   (const float *)m->exprT.p, epart);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bf_ext_reduce_kernel, dim3((ne + BF_RED_COLS - 1) / BF_RED_COLS, n), dim3(8 * BF_RED_COLS), 0, c.stream,
                               (const float *)epart, etiles, ne, emesh, ne, (int *)nullptr, 0);
            HIP_TRY(hipGetLastError());
        }
        // 3. chain + Rodrigues reversed (the rest joints with Jx psi; dexpression = the vertex part + Jx^T dL/d(rest joints))
        hipLaunchKernelGGL(bf_smpl_vjp_chain_kernel, dim3(n), dim3(64), 0, c.stream, m->fit, (const float *)state, (const float *)ext, EXT,
                           (const float *)dchain, dtheta, dbeta, (const float *)(expr ? dJx : nullptr),
                           (const float *)(expr ? m->Jx.p : nullptr), ne, (const float *)(dex ? emesh : nullptr), dex ? dexpr : (float *)nullptr);
        HIP_TRY(hipGetLastError());
        return BF_OK;
    }
};

// rows[n][stride] on the device -> per block (dst, off, cnt), dst[n][cnt] = rows[.][off .. off + cnt) (null dst: not wanted), and the
// call finished: the host route drains, fetches the rows once and cuts them on the host; the device route cuts them with one launch
struct Block { float *dst; int off, cnt; };
// the betas a call takes: the shape space's when one is attached, else the model's own
int bf_nb_total(const bf_model *m) { return m->nb_total ? m->nb_total : m->nb; }
// last = false: more kernels follow - nothing is finished; the host route's copy waits for the NULL stream's work as every hipMemcpy does
int deliver_blocks(BfRouteCall &c, const float *rows, size_t N, int stride, std::initializer_list<Block> blocks, bool last = true) {
    BfScatter S{};
    for (const Block &b : blocks)
        if (b.dst && b.cnt > 0) { S.dst[S.n_blocks] = b.dst; S.off[S.n_blocks] = b.off; S.cnt[S.n_blocks] = b.cnt; ++S.n_blocks; }
    if (c.ws && S.n_blocks > 0)
        hipLaunchKernelGGL(bf_block_scatter_kernel, dim3((unsigned)((N * stride + 255) / 256)), dim3(256), 0, c.stream, rows, (int)N, stride, S);
    if (last) BF_TRY(c.finish());
    if (c.ws || S.n_blocks == 0) return BF_OK;
    std::vector<float> g(N * stride);
    HIP_TRY(hipMemcpy(g.data(), rows, g.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < S.n_blocks; ++k)
        for (size_t f = 0; f < N; ++f) std::memcpy(S.dst[k] + f * S.cnt[k], g.data() + f * stride + S.off[k], S.cnt[k] * sizeof(float));
    return BF_OK;
}

// (built once, and complete on the device when this returns: later calls come on any stream)
int ensure_posedirsT(bf_model *m, hipStream_t stream) {
    std::lock_guard<std::mutex> g(m->lazy);
    return bf_ensure_posedirsT_locked(m, stream);
}

// SMPL-X: the parameter blocks where the kernels read them and the thetas assembled from them
struct Inputs {
    const float *beta = nullptr, *orient = nullptr, *body = nullptr, *jaw = nullptr, *leye = nullptr, *reye = nullptr, *lh = nullptr, *rh = nullptr;
    const float *ext = nullptr;             // the extension coefficients [n][n_ext], or null: none - the launches of a call without expression
    float *full = nullptr, *th_root = nullptr, *th_rest = nullptr;
    // full_to: the caller's full_pose array, or null.  expression: the caller's [n][n_expr], or null
    int bind(BfRouteCall &c, const bf_model *m, size_t N, const bf_smplx_params *in, const float *expression, float *full_to) {
        const int n_pca = m->fit.n_pca, nj = m->nj, nbt = bf_nb_total(m);
        BF_TRY(c.in(in->betas, N * nbt, beta));
        BF_TRY(c.in(in->global_orient, N * 3, orient));
        BF_TRY(c.in(in->body_pose, N * m->fit.nbp, body));
        BF_TRY(c.in(in->jaw_pose, N * 3, jaw));
        BF_TRY(c.in(in->leye_pose, N * 3, leye));
        BF_TRY(c.in(in->reye_pose, N * 3, reye));
        BF_TRY(c.in(in->left_hand_pose, N * n_pca, lh));
        BF_TRY(c.in(in->right_hand_pose, N * n_pca, rh));
        BF_TRY(c.out(full_to, N * 3 * nj, full, true));
        BF_TRY(c.scratch(N * 3, th_root));
        BF_TRY(c.scratch(N * 3 * (nj - 1), th_rest));
        hipLaunchKernelGGL(bf_smplx_pose_assemble_kernel, dim3((unsigned)N), dim3(64), 0, c.stream, m->fit, orient, body, jaw, leye, reye, lh, rh,
                           full, th_root, th_rest);
        HIP_TRY(hipGetLastError());
        BF_TRY(c.in(expression, N * m->n_expr, ext));
        if (nbt > m->nb) {                  // a shape space: the caller's rows cut into the core block and [betas[nb:], expression]
            float *core = nullptr, *e = nullptr;
            BF_TRY(c.scratch(N * m->nb, core));
            BF_TRY(c.scratch(N * m->n_ext, e));
            hipLaunchKernelGGL(bf_shape_ext_pack_kernel, dim3((unsigned)N), dim3(64), 0, c.stream, beta, ext, nbt, m->n_expr, m->nb, core, e);
            HIP_TRY(hipGetLastError());
            beta = core; ext = e;
        }
        return BF_OK;
    }
};

// the bodies of bf_smpl_forward, bf_smpl_vjp, bf_smplx_forward_expr and bf_smplx_vjp_expr and of their *_dev twins (arguments checked)
// models.smpl.SMPL.forward: the joints pass writes the mapped joints and joints_ori whoever wants them
int smpl_forward(BfRouteCall &c, bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                 float *vertices, float *joints, float *joints_ori) {
    BF_TRY(c.begin(m->device));
    const size_t N = (size_t)n;
    const float *d_beta = nullptr, *d_or = nullptr, *d_bp = nullptr;
    BF_TRY(c.in(betas, N * m->nb, d_beta));
    BF_TRY(c.in(global_orient, N * 3, d_or));
    BF_TRY(c.in(body_pose, N * 3 * (m->nj - 1), d_bp));
    ModelPass pass(m, n, c);
    float *jori = nullptr;
    BF_TRY(pass.need(pass.state, N * bf_state_stride(m->nj, m->npf, m->nb)));
    BF_TRY(pass.need(pass.vraw, N * m->nv * 3, vertices));
    BF_TRY(pass.need(pass.xpart, N * m->mesh.n_tiles * m->n_extra * 3));
    BF_TRY(pass.need(pass.joints, N * m->n_joint_map * 3, joints));
    BF_TRY(pass.need(jori, N * (m->nj + m->n_selector) * 3, joints_ori));
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, c.stream, m->fit, d_beta, d_or, d_bp, (const float *)nullptr, pass.state,
                       (const float *)nullptr, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    MeshPass mesh;
    mesh.scr = c.mesh_scratch(); mesh.n = n; mesh.state = pass.state; mesh.stream = c.stream;
    mesh.vraw = pass.vraw; mesh.xpart = pass.xpart; mesh.joints = pass.joints; mesh.joints_ori = jori;
    BF_TRY(pass.launch_mesh(mesh));
    return c.finish();
}

int smpl_vjp(BfRouteCall &c, bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
             const float *dvertices, const float *djoints, const float *djoints_ori, float *dbetas, float *dglobal_orient, float *dbody_pose) {
    BF_TRY(c.begin(m->device));
    BF_TRY(ensure_posedirsT(m, c.stream));
    const int nj = m->nj, nb = m->nb, n_ori = nj + m->n_selector;
    const size_t N = (size_t)n;
    const float *d_beta = nullptr, *d_or = nullptr, *d_bp = nullptr, *d_dvert = nullptr, *d_dj = nullptr, *d_djo = nullptr;
    BF_TRY(c.in(betas, N * nb, d_beta));
    BF_TRY(c.in(global_orient, N * 3, d_or));
    BF_TRY(c.in(body_pose, N * 3 * (nj - 1), d_bp));
    BF_TRY(c.in(dvertices, N * m->nv * 3, d_dvert));
    BF_TRY(c.in(djoints, N * m->n_joint_map * 3, d_dj));
    BF_TRY(c.in(djoints_ori, N * n_ori * 3, d_djo));
    ModelPass pass(m, n, c);
    pass.to.dbeta = dbetas;
    BF_TRY(pass.forward(d_beta, d_or, d_bp, true));
    BF_TRY(pass.reverse(d_dvert, d_dj, d_djo, n_ori));
    return deliver_blocks(c, pass.dtheta, N, 3 * nj, {{dglobal_orient, 0, 3}, {dbody_pose, 3, 3 * (nj - 1)}});
}

int smplx_forward(BfRouteCall &c, bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_outputs *out) {
    BF_TRY(c.begin(m->device));
    const size_t N = (size_t)n;
    Inputs x;
    int *d_row = nullptr;
    BF_TRY(x.bind(c, m, N, in, expression, out->full_pose));
    BF_TRY(c.out((int *)out->dyn_row, N, d_row, true));
    ModelPass pass(m, n, c);
    pass.to.vraw = out->vertices; pass.to.joints = out->joints; pass.to.jraw = out->joints_all;
    BF_TRY(pass.forward(x.beta, x.th_root, x.th_rest, false, x.ext));
    hipLaunchKernelGGL(bf_smplx_dyn_row_kernel, dim3((n + 63) / 64), dim3(64), 0, c.stream, m->mesh, (const float *)pass.state, n, d_row);
    return c.finish();
}

int smplx_vjp(BfRouteCall &c, bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_cotangents *cot,
              const bf_smplx_grads *grads, float *dexpression) {
    BF_TRY(c.begin(m->device));
    BF_TRY(ensure_posedirsT(m, c.stream));
    const int nj = m->nj, n_pca = m->fit.n_pca, nbp = m->fit.nbp, OUT = 3 * nj + 2 * n_pca;
    const size_t N = (size_t)n;
    Inputs x;
    const float *d_dvert = nullptr, *d_dj = nullptr, *d_dja = nullptr, *d_dfull = nullptr;
    float *d_out = nullptr;
    BF_TRY(x.bind(c, m, N, in, expression, nullptr));
    BF_TRY(c.in(cot->dvertices, N * m->nv * 3, d_dvert));
    BF_TRY(c.in(cot->djoints, N * m->n_joint_map * 3, d_dj));
    BF_TRY(c.in(cot->djoints_all, N * m->n_all * 3, d_dja));
    BF_TRY(c.in(cot->dfull_pose, N * 3 * nj, d_dfull));
    BF_TRY(c.scratch(N * OUT, d_out));
    ModelPass pass(m, n, c);
    // (a shape space: dbetas[n][NB] = the core gradient | the head of the extension's, dexpression its tail - joined into rows below)
    const int nbt = bf_nb_total(m);
    const bool space = nbt > m->nb;
    if (!space) { pass.to.dbeta = grads->dbetas; pass.to.dexpr = dexpression; }
    BF_TRY(pass.forward(x.beta, x.th_root, x.th_rest, true, x.ext));
    BF_TRY(pass.reverse(d_dvert, d_dj, d_dja, m->n_all, space ? grads->dbetas || dexpression : dexpression != nullptr));
    if (space && (grads->dbetas || dexpression)) {
        float *rows = nullptr;
        BF_TRY(c.scratch(N * (nbt + m->n_expr), rows));
        hipLaunchKernelGGL(bf_shape_ext_join_kernel, dim3(n), dim3(64), 0, c.stream, (const float *)pass.dbeta, (const float *)pass.dexpr, m->nb,
                           m->n_ext, rows);
        HIP_TRY(hipGetLastError());
        BF_TRY(deliver_blocks(c, rows, N, nbt + m->n_expr, {{grads->dbetas, 0, nbt}, {dexpression, nbt, m->n_expr}}, false));
    }
    // the pose assembly reversed
    hipLaunchKernelGGL(bf_smplx_pose_reverse_kernel, dim3(n), dim3(64), 0, c.stream, m->fit, (const float *)pass.dtheta, d_dfull, d_out);
    HIP_TRY(hipGetLastError());
    // full pose order: root | body | jaw | left eye | right eye | hands (through their PCA coefficients, behind the thetas)
    return deliver_blocks(c, d_out, N, OUT, {{grads->dglobal_orient, 0, 3}, {grads->dbody_pose, 3, nbp}, {grads->djaw_pose, 3 + nbp, 3},
                                             {grads->dleye_pose, 6 + nbp, 3}, {grads->dreye_pose, 9 + nbp, 3},
                                             {grads->dleft_hand_pose, 3 * nj, n_pca}, {grads->dright_hand_pose, 3 * nj + n_pca, n_pca}});
}

// a call's expression argument against the model: coefficients need directions
int bf_expr_check(const bf_model *m, const float *expression, const char *who) {
    if (expression && m->n_expr == 0)
        return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": the model has no expression directions - call bf_model_set_expression first");
    return BF_OK;
}

// the arguments every *_dev entry point of a model shares
int dev_route_check(const bf_model *m, const bf_workspace *ws, int n, const char *who) {
    if (!m || !ws || n <= 0) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    if (ws->device != m->device) return fail(BF_ERR_INVALID, std::string(who) + ": the workspace lives on another device than the model");
    return BF_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// The entry points: the arguments checked (a refused call has queued nothing), the route counted, the body run on that route's call
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int bf_smpl_vjp(bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                           const float *dvertices, const float *djoints, const float *djoints_ori,
                           float *dbetas, float *dglobal_orient, float *dbody_pose) {
    if (!m || n <= 0 || !betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, "bf_smpl_vjp: bad argument");
    BF_TRY(bf_grad_check(m, 0, "bf_smpl_vjp"));
    ++bf_route_stats().host;
    if (!dbetas && !dglobal_orient && !dbody_pose) return BF_OK;
    BfRouteCall c(nullptr, nullptr);
    return smpl_vjp(c, m, n, betas, global_orient, body_pose, dvertices, djoints, djoints_ori, dbetas, dglobal_orient, dbody_pose);
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
    BfRouteCall c(ws, (hipStream_t)stream);
    return smpl_vjp(c, m, n, betas, global_orient, body_pose, dvertices, djoints, djoints_ori, dbetas, dglobal_orient, dbody_pose);
}

extern "C" int bf_smpl_forward(bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                               float *vertices, float *joints, float *joints_ori) {
    if (!m || n <= 0 || !betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, "bf_smpl_forward: bad argument");
    ++bf_route_stats().host;
    BfRouteCall c(nullptr, nullptr);
    return smpl_forward(c, m, n, betas, global_orient, body_pose, vertices, joints, joints_ori);
}

extern "C" int bf_smpl_forward_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const float *betas, const float *global_orient,
                                   const float *body_pose, float *vertices, float *joints, float *joints_ori) {
    const char *who = "bf_smpl_forward_dev";
    BF_TRY(dev_route_check(m, ws, n, who));
    if (!betas || !global_orient || !body_pose) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    if (m->kind != 0) return fail(BF_ERR_UNSUPPORTED, std::string(who) + ": SMPL-kind models only");
    ++bf_route_stats().dev;
    BfRouteCall c(ws, (hipStream_t)stream);
    return smpl_forward(c, m, n, betas, global_orient, body_pose, vertices, joints, joints_ori);
}

extern "C" int bf_model_n_expression(const bf_model *m) { return m ? m->n_expr : 0; }

// dirs[NV][3][L] onto the model as its extension directions: the transposed copy, Jx, and for the wide kernels the second layout and
// Jx transposed.  The caller holds m->lazy and has checked the counts; the model counts no directions unless every upload succeeded.
static int bf_attach_directions(bf_model *m, int nb_total, int n_expr, int L, const float *dirs) {
    HIP_TRY(hipSetDevice(m->device));
    const int nv = m->nv, nj = m->nj, ne = L;
    const char *sw = getenv("BF_SHAPE_EXT_WIDE");
    const bool wide = L > BF_EXPR_MAX || (sw && sw[0] == '1' && sw[1] == 0);
    // E transposed: [l][k][v]
    std::vector<float> eT((size_t)ne * 3 * nv);
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < ne; ++l) eT[((size_t)l * 3 + k) * nv + v] = dirs[((size_t)v * 3 + k) * ne + l];
    // Jx = J_regressor E: float64 accumulation over a joint's non-zero weights in vertex order, rounded once (as contract_regressor forms Jd)
    std::vector<float> jx((size_t)nj * 3 * ne);
    std::vector<double> acc((size_t)3 * ne);
    for (int j = 0; j < nj; ++j) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int q = m->jreg_start[j]; q < m->jreg_start[j + 1]; ++q) {
            const double w = m->jreg_w[q];
            const float *e = dirs + (size_t)m->jreg_v[q] * 3 * ne;
            for (int i = 0; i < 3 * ne; ++i) acc[i] += w * e[i];
        }
        for (int i = 0; i < 3 * ne; ++i) jx[(size_t)j * 3 * ne + i] = (float)acc[i];
    }
    HIP_TRY(m->exprT.upload(eT));
    HIP_TRY(m->Jx.upload(jx));
    if (wide) {
        std::vector<float> jxT((size_t)ne * nj * 3);
        for (int r = 0; r < nj * 3; ++r)
            for (int l = 0; l < ne; ++l) jxT[(size_t)l * nj * 3 + r] = jx[(size_t)r * ne + l];
        HIP_TRY(m->JxT.upload(jxT));
        HIP_TRY(m->extVK.upload(std::vector<float>(dirs, dirs + (size_t)nv * 3 * ne)));
    }
    m->n_expr = n_expr;
    m->nb_total = nb_total;
    m->ext_wide = wide;
    m->n_ext = L;
    return BF_OK;
}

extern "C" int bf_model_set_expression(bf_model *m, int n_expr, const float *exprdirs) {
    if (!m || !exprdirs) return fail(BF_ERR_INVALID, "bf_model_set_expression: bad argument");
    BF_TRY(bf_grad_check(m, 1, "bf_model_set_expression"));
    if (n_expr < 1 || n_expr > BF_EXPR_MAX)
        return fail(BF_ERR_UNSUPPORTED, "bf_model_set_expression: 1.." + std::to_string(BF_EXPR_MAX) + " expression coefficients supported");
    std::lock_guard<std::mutex> g(m->lazy);
    if (m->n_ext != 0) return fail(BF_ERR_INVALID, "bf_model_set_expression: the model has its expression directions already");
    return bf_attach_directions(m, 0, n_expr, n_expr, exprdirs);
}

extern "C" int bf_model_n_betas(const bf_model *m) { return m ? bf_nb_total(m) : 0; }
extern "C" int bf_model_shape_ext_wide(const bf_model *m) { return m && m->ext_wide ? 1 : 0; }

extern "C" int bf_model_set_shape_space(bf_model *m, int n_betas, int n_expr, const float *dirs) {
    if (!m || !dirs) return fail(BF_ERR_INVALID, "bf_model_set_shape_space: bad argument");
    BF_TRY(bf_grad_check(m, 1, "bf_model_set_shape_space"));
    const int L = n_betas - m->nb + n_expr;
    if (n_betas < 10 || n_betas > 300 || n_betas < m->nb || n_expr < 0 || n_expr > 100 || L < 1 || L > BF_SHAPE_EXT_MAX)
        return fail(BF_ERR_UNSUPPORTED, "bf_model_set_shape_space: 10..300 betas and 0..100 expression coefficients supported, at least one "
                                        "direction beyond the model's " + std::to_string(m->nb) + " betas");
    std::lock_guard<std::mutex> g(m->lazy);
    if (m->n_ext != 0) return fail(BF_ERR_INVALID, "bf_model_set_shape_space: the model has its shape space or expression directions already");
    return bf_attach_directions(m, n_betas, n_expr, L, dirs);
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
    BfRouteCall c(nullptr, nullptr);
    return smplx_forward(c, m, n, in, expression, out);
}

extern "C" int bf_smplx_forward_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const bf_smplx_params *in, const float *expression,
                                    const bf_smplx_outputs *out) {
    const char *who = "bf_smplx_forward_dev";
    BF_TRY(dev_route_check(m, ws, n, who));
    if (!in || !out || !in->betas || !in->global_orient || !in->body_pose) return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 1, who));
    BF_TRY(bf_expr_check(m, expression, who));
    ++bf_route_stats().dev;
    BfRouteCall c(ws, (hipStream_t)stream);
    return smplx_forward(c, m, n, in, expression, out);
}

extern "C" int bf_smplx_vjp(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_cotangents *cot, const bf_smplx_grads *grads) {
    return bf_smplx_vjp_expr(m, n, in, nullptr, cot, grads, nullptr);
}

// no gradient is asked for
static bool none_wanted(const bf_smplx_grads *g, const float *dexpression) {
    return !g->dbetas && !g->dglobal_orient && !g->dbody_pose && !g->djaw_pose && !g->dleye_pose && !g->dreye_pose && !g->dleft_hand_pose &&
           !g->dright_hand_pose && !dexpression;
}

extern "C" int bf_smplx_vjp_expr(bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_cotangents *cot,
                                 const bf_smplx_grads *grads, float *dexpression) {
    const char *who = expression ? "bf_smplx_vjp_expr" : "bf_smplx_vjp";
    if (!m || n <= 0 || !in || !cot || !grads || !in->betas || !in->global_orient || !in->body_pose || (dexpression && !expression))
        return fail(BF_ERR_INVALID, std::string(who) + ": bad argument");
    BF_TRY(bf_grad_check(m, 1, who));
    BF_TRY(bf_expr_check(m, expression, who));
    ++bf_route_stats().host;
    if (none_wanted(grads, dexpression)) return BF_OK;
    BfRouteCall c(nullptr, nullptr);
    return smplx_vjp(c, m, n, in, expression, cot, grads, dexpression);
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
    if (none_wanted(grads, dexpression)) return BF_OK;
    BfRouteCall c(ws, (hipStream_t)stream);
    return smplx_vjp(c, m, n, in, expression, cot, grads, dexpression);
}
