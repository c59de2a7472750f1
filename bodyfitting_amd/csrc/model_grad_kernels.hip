// The body models' forward ends and reverse pass for gfx950: the kernels bf_smpl_vjp, bf_smplx_forward and bf_smplx_vjp
// (model_grad_api.hip) add around the pose-state kernel, the dense schedule's mesh passes and bf_ext_reduce_kernel.  The reverse is
// that of models.smpl.SMPL.forward (smplx lbs() + the wrapper of models/smpl.py:69-83) and of smplx.create(model_type='smplx').forward.
//
//   bf_model_vjp_fold_kernel       dL/d(mapped joints), dL/d(smplx joints), dL/dvertices -> dL/dvertices of the mesh reverse + dL/d(posed chain joints)
//   bf_smpl_vjp_chain_kernel       the reduced mesh-reverse row + dL/d(posed chain joints) -> dL/dtheta, dL/dbeta
//   bf_smplx_pose_assemble_kernel  the eight parameter blocks -> full_pose (hands = PCA . components, + pose_mean, jaw as an input)
//   bf_smplx_dyn_row_kernel        the contour-table row the neck chain's yaw selects (an output of the forward)
//   bf_smplx_pose_reverse_kernel   dL/dtheta (+ dL/dfull_pose) -> the pass-through thetas and the hand PCA coefficients' gradients
//
// The math is the reverse half of oracle/analytic.py: loss_grad, with the skinning sums taken from bf_ext_reduce_kernel's row.
// No float atomics: every sum has a fixed order, so a call's bits do not depend on timing.
// The LDS tables are sized by BF_GRAD_MAX_* (bf_internal.h), which the host checks a model against.
#include "bf_internal.h"
#include "pose_state_body.h"
#include "model_grad_kernels.h"

#define BF_VJP_FOLD_THREADS 256

// grid (ceil(NV / 256), n), 256 threads.  All joints in smplx order: chain | selector vertices | J_regressor_extra rows | landmarks
// (nlm of them: the model's with lmk_vid given, none without - SMPL).  Per frame f:
//   dall[j] = sum over i ascending with joint_map[i] == j of djoints[i]  (+ ddirect[j] for j < n_direct)
//   dchain[f][j] = dall[j] for the NJ chain joints (workgroup x = 0 writes it)
//   dv[f][v] = dvertices[f][v] + sum over s ascending with selector_ids[s] == v of dall[NJ + s]
//              + sum over e ascending of J_regressor_extra[e][v] dall[NJ + n_selector + e]
//              + sum over the landmark entries q = 3 l + c ascending with lmk_vid[f][q] == v of lmk_w[f][q] dall[first landmark + l]
// ddirect[n][n_direct][3]: the cotangent of the joints the model returns itself - SMPL's joints_ori (NJ + n_selector of them),
// SMPL-X's joints_all (all).
// lmk_vid / lmk_w: the corner vertices and barycentric weights the forward recompute used for this frame (bf_joints_body); the
// row choice behind them is an integer look-up and carries no gradient.  Several landmarks share vertices, hence a gather.
// Without landmarks their staging, its barrier and the last term are skipped, not taken as zero: -0 + 0 is +0, and SMPL's dv
// keeps the sign it has without that term.
// Any of dvertices / djoints / ddirect may be null (= zero).
extern "C" __global__ void __launch_bounds__(BF_VJP_FOLD_THREADS)
bf_model_vjp_fold_kernel(MeshTab M, const float *__restrict__ dvertices, const float *__restrict__ djoints, const float *__restrict__ ddirect,
                         int n_direct, const int *__restrict__ lmk_vid, const float *__restrict__ lmk_w, float *__restrict__ dv,
                         float *__restrict__ dchain) {
    __shared__ float s_dall[BF_GRAD_MAX_ALL * 3];
    __shared__ int s_map[BF_GRAD_MAX_MAP];
    __shared__ int s_sel[BF_GRAD_MAX_SEL];
    __shared__ int s_lv[BF_GRAD_MAX_LMK * 3];
    __shared__ float s_lc[BF_GRAD_MAX_LMK * 3 * 3];       // per entry: weight x the landmark's cotangent
    const int nj = M.nj, nv = M.nv, nsel = M.n_selector, ne = M.n_extra, nmap = M.n_joint_map;
    const int nlm = lmk_vid ? M.n_lmk_static + M.n_lmk_dyn : 0;
    const int n_ori = nj + nsel, lm0 = n_ori + ne, n_all = lm0 + nlm;
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < nmap; i += BF_VJP_FOLD_THREADS) s_map[i] = M.joint_map[i];
    for (int i = tid; i < nsel; i += BF_VJP_FOLD_THREADS) s_sel[i] = M.selector_ids[i];
    for (int i = tid; i < nlm * 3; i += BF_VJP_FOLD_THREADS) s_lv[i] = lmk_vid[(size_t)f * nlm * 3 + i];
    __syncthreads();
    for (int i = tid; i < n_all * 3; i += BF_VJP_FOLD_THREADS) {
        const int j = i / 3, k = i - j * 3;
        float acc = 0.f;
        if (djoints) {
            const float *dj = djoints + (size_t)f * nmap * 3 + k;
            for (int q = 0; q < nmap; ++q)
                if (s_map[q] == j) acc += dj[q * 3];
        }
        if (ddirect && j < n_direct) acc += ddirect[((size_t)f * n_direct + j) * 3 + k];
        s_dall[i] = acc;
        if (j < nj && blockIdx.x == 0) dchain[((size_t)f * nj + j) * 3 + k] = acc;
    }
    __syncthreads();
    if (nlm) {                                                   // (block-uniform)
        for (int i = tid; i < nlm * 9; i += BF_VJP_FOLD_THREADS) {
            const int q = i / 3, k = i - q * 3, l = q / 3;
            s_lc[i] = lmk_w[(size_t)f * nlm * 3 + q] * s_dall[(lm0 + l) * 3 + k];
        }
        __syncthreads();
    }
    const int v = blockIdx.x * BF_VJP_FOLD_THREADS + tid;
    if (v >= nv) return;
    float sel[3] = {0.f, 0.f, 0.f}, ext[3] = {0.f, 0.f, 0.f}, lmk[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < nsel; ++s)
        if (s_sel[s] == v) {
            sel[0] += s_dall[(nj + s) * 3]; sel[1] += s_dall[(nj + s) * 3 + 1]; sel[2] += s_dall[(nj + s) * 3 + 2];
        }
    for (int e = 0; e < ne; ++e) {
        const float w = M.j_extra[(size_t)e * nv + v];          // (row e over the vertices: coalesced)
        const float *d = s_dall + (n_ori + e) * 3;
        ext[0] += w * d[0]; ext[1] += w * d[1]; ext[2] += w * d[2];
    }
    for (int q = 0; q < nlm * 3; ++q)                            // (every lane reads the same LDS word: a broadcast)
        if (s_lv[q] == v) { lmk[0] += s_lc[q * 3]; lmk[1] += s_lc[q * 3 + 1]; lmk[2] += s_lc[q * 3 + 2]; }
    const size_t o = ((size_t)f * nv + v) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = dvertices ? dvertices[o + k] : 0.f;
        const float body = (g + sel[k]) + ext[k];
        dv[o + k] = nlm ? body + lmk[k] : body;
    }
}

namespace {
// smplx batch_rodrigues reversed (oracle/analytic.py: rodrigues_bwd): theta[3], dL/dR[9] -> dL/dtheta[3].
// angle = ||theta + 1e-8|| as the forward (m_rodrigues) has it, so theta = 0 is an ordinary point.
__device__ inline void vjp_rodrigues(const float *th, const float *dR, float *g) {
    const float ux = th[0] + 1e-8f, uy = th[1] + 1e-8f, uz = th[2] + 1e-8f;
    const float a = sqrtf(ux * ux + uy * uy + uz * uz);
    const float nx = th[0] / a, ny = th[1] / a, nz = th[2] / a;
    float s, c;
    sincosf(a, &s, &c);
    const float K[9] = {0.f, -nz, ny, nz, 0.f, -nx, -ny, nx, 0.f};
    float KK[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) KK[r * 3 + q] = K[r * 3] * K[q] + K[r * 3 + 1] * K[3 + q] + K[r * 3 + 2] * K[6 + q];
    float sk = 0.f, skk = 0.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) { sk += dR[e] * K[e]; skk += dR[e] * KK[e]; }
    float da = c * sk + s * skk;
    // H = s dR + (1 - c) (dR K^T + K^T dR)
    const float oc = 1.0f - c;
    float H[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float a1 = dR[r * 3] * K[q * 3] + dR[r * 3 + 1] * K[q * 3 + 1] + dR[r * 3 + 2] * K[q * 3 + 2];   // (dR K^T)[r][q]
            const float a2 = K[r] * dR[q] + K[3 + r] * dR[3 + q] + K[6 + r] * dR[6 + q];                            // (K^T dR)[r][q]
            H[r * 3 + q] = s * dR[r * 3 + q] + oc * (a1 + a2);
        }
    const float dn0 = H[7] - H[5], dn1 = H[2] - H[6], dn2 = H[3] - H[1];
    da = da - (dn0 * th[0] + dn1 * th[1] + dn2 * th[2]) / (a * a);
    const float q = da / a;
    g[0] = dn0 / a + q * ux;
    g[1] = dn1 / a + q * uy;
    g[2] = dn2 / a + q * uz;
}
}  // namespace

// grid (n), one wave per frame.  In: the pose state (GR, theta, beta), the reduced mesh-reverse row
//   ext[f][EXT] = dfeat[npf] | per joint (sum w dv (x) vp | sum w dv) as 3 rows of 4 | dbeta_mesh[nb] | dt ds
// and dchain[f][NJ][3] = dL/d(posed chain joints).  Out: dtheta[f][NJ*3], dbeta[f][nb].
// SMPL-X expression (bf_smplx_vjp_expr; all null / 0 otherwise, and the results are then the bits they are without these arguments):
// dJx[f][NJ*3] = Jx psi joins the rest joints; dexpr[f][ne] (null: not wanted) = dexpr_mesh[f][ne] + Jx^T dL/d(rest joints).
// Leaves to root over the levels of FitTab (level_start / level_joints); a parent takes its children's contributions in the
// order of its CSR child list - one writer per joint and step, no atomics.
extern "C" __global__ void __launch_bounds__(64)
bf_smpl_vjp_chain_kernel(FitTab T, const float *__restrict__ state, const float *__restrict__ ext, int ext_stride,
                         const float *__restrict__ dchain, float *__restrict__ dtheta, float *__restrict__ dbeta,
                         const float *__restrict__ dJx, const float *__restrict__ Jx, int ne, const float *__restrict__ dexpr_mesh,
                         float *__restrict__ dexpr) {
    constexpr int MJ = BF_GRAD_MAX_JOINTS;
    __shared__ float s_R[MJ * 9], s_GR[MJ * 9], s_J[MJ * 3], s_dGR[MJ * 9], s_dGt[MJ * 3], s_dJ[MJ * 3], s_cGR[MJ * 9], s_drel[MJ * 3];
    __shared__ float s_dR[MJ * 9];
    const int nj = T.nj, nb = T.nb, npf = T.npf, tid = threadIdx.x, f = blockIdx.x;
    StateView st = bf_state_view(const_cast<float *>(state) + (size_t)f * bf_state_stride(nj, npf, nb), nj, npf, nb);
    const float *row = ext + (size_t)f * ext_stride;
    // rotations (the forward's own arithmetic), chain rotations, rest joints J = Jt + Jd beta (l ascending, as the pose state forms them)
    if (tid < nj) {
        const int i = tid;
        m_rodrigues(st.theta[i * 3], st.theta[i * 3 + 1], st.theta[i * 3 + 2], s_R + i * 9);
#pragma unroll
        for (int e = 0; e < 9; ++e) s_GR[i * 9 + e] = st.GR[i * 9 + e];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float acc = 0.f;
            for (int l = 0; l < nb; ++l) acc += T.Jd[(i * 3 + k) * nb + l] * st.beta[l];
            s_J[i * 3 + k] = T.Jt[i * 3 + k] + acc;
            if (dJx) s_J[i * 3 + k] += dJx[((size_t)f * nj + i) * 3 + k];
        }
    }
    __syncthreads();
    // A_i.t = G_i.t - G_i.R J_i:  dGt = dchain + dAt,  dGR = dGR_mesh - dAt (x) J,  dJ = -G_i.R^T dAt
    if (tid < nj) {
        const int i = tid;
        const float *r = row + npf + i * 12;
        float dAt[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) dAt[a] = r[a * 4 + 3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s_dGt[i * 3 + a] = dchain[((size_t)f * nj + i) * 3 + a] + dAt[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s_dGR[i * 9 + a * 3 + b] = r[a * 4 + b] - dAt[a] * s_J[i * 3 + b];
        }
#pragma unroll
        for (int b = 0; b < 3; ++b)
            s_dJ[i * 3 + b] = -(s_GR[i * 9 + b] * dAt[0] + s_GR[i * 9 + 3 + b] * dAt[1] + s_GR[i * 9 + 6 + b] * dAt[2]);
    }
    __syncthreads();
    // kinematic chain, leaves to root
    for (int lev = T.n_levels - 1; lev >= 1; --lev) {
        const int ls = T.level_start[lev], cnt = T.level_start[lev + 1] - ls;
        if (tid < cnt) {
            const int i = T.level_joints[ls + tid], p = T.parents[i];
            const float *Gp = s_GR + p * 9, *dG = s_dGR + i * 9, *Ri = s_R + i * 9, *dt = s_dGt + i * 3;
            float rel[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) rel[k] = s_J[i * 3 + k] - s_J[p * 3 + k];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    s_dR[i * 9 + a * 3 + b] = Gp[a] * dG[b] + Gp[3 + a] * dG[3 + b] + Gp[6 + a] * dG[6 + b];                   // G_p.R^T dG_i
                    s_cGR[i * 9 + a * 3 + b] = (dG[a * 3] * Ri[b * 3] + dG[a * 3 + 1] * Ri[b * 3 + 1] + dG[a * 3 + 2] * Ri[b * 3 + 2]) +
                                               dt[a] * rel[b];                                                                   // dG_i R_i^T + dGt_i rel_i^T
                }
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const float d = Gp[b] * dt[0] + Gp[3 + b] * dt[1] + Gp[6 + b] * dt[2];                                          // G_p.R^T dGt_i
                s_drel[i * 3 + b] = d;
                s_dJ[i * 3 + b] += d;
            }
        }
        __syncthreads();
        const int ps = T.level_start[lev - 1], pcnt = T.level_start[lev] - ps;
        if (tid < pcnt) {
            const int p = T.level_joints[ps + tid];
            for (int q = T.child_start[p]; q < T.child_start[p + 1]; ++q) {
                const int c = T.child_list[q];
#pragma unroll
                for (int e = 0; e < 9; ++e) s_dGR[p * 9 + e] += s_cGR[c * 9 + e];
#pragma unroll
                for (int k = 0; k < 3; ++k) { s_dGt[p * 3 + k] += s_dGt[c * 3 + k]; s_dJ[p * 3 + k] -= s_drel[c * 3 + k]; }
            }
        }
        __syncthreads();
    }
    // root: dR_0 = dG_0, dJ_0 += dGt_0; the pose feature R_i - I of joints 1.. adds dfeat; Rodrigues reversed
    if (tid < nj) {
        const int i = tid;
        float dR[9], g[3], th[3];
        if (i == 0) {
#pragma unroll
            for (int e = 0; e < 9; ++e) dR[e] = s_dGR[e];
#pragma unroll
            for (int k = 0; k < 3; ++k) s_dJ[k] += s_dGt[k];
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) dR[e] = s_dR[i * 9 + e] + row[(i - 1) * 9 + e];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) th[k] = st.theta[i * 3 + k];
        vjp_rodrigues(th, dR, g);
#pragma unroll
        for (int k = 0; k < 3; ++k) dtheta[((size_t)f * nj + i) * 3 + k] = g[k];
    }
    __syncthreads();
    // dbeta = the mesh reverse's shapedirs part + Jd^T dJ (J rows ascending)
    if (tid < nb) {
        float acc = 0.f;
        for (int r = 0; r < nj * 3; ++r) acc += T.Jd[r * nb + tid] * s_dJ[r];
        dbeta[(size_t)f * nb + tid] = row[npf + nj * 12 + tid] + acc;
    }
    // dexpression = the expression reverse's vertex part + Jx^T dJ (J rows ascending); a lane walks the coefficients tid, tid + 64, ..:
    // a shape space (bf_model_set_shape_space) brings up to BF_SHAPE_EXT_MAX of them
    if (dexpr)
        for (int l = tid; l < ne; l += 64) {
            float acc = 0.f;
            for (int r = 0; r < nj * 3; ++r) acc += Jx[r * ne + l] * s_dJ[r];
            dexpr[(size_t)f * ne + l] = dexpr_mesh[(size_t)f * ne + l] + acc;
        }
}

// ---- the SMPL-X specific ends: what bf_smplx_forward / bf_smplx_vjp put before and behind the passes above

// grid (n), one wave per frame.  The blocks go into the optimiser-order parameter vector in LDS and every joint's theta is then
// bf_theta3 of it - the expressions bf_pose_state_kernel's packed path evaluates, so equal values give equal bits there and here.
// The jaw (th_kind 1: a constant of the packed path) takes `jaw` on top when it is given.  leye / reye / lh / rh / jaw may be
// null (= zeros).  Out: full[n][3 NJ], and the same thetas as bf_pose_state_kernel's non-packed path reads them:
// th_root[n][3], th_rest[n][3 (NJ - 1)].
extern "C" __global__ void __launch_bounds__(64)
bf_smplx_pose_assemble_kernel(FitTab T, const float *__restrict__ orient, const float *__restrict__ body_pose, const float *__restrict__ jaw,
                              const float *__restrict__ leye, const float *__restrict__ reye, const float *__restrict__ lh,
                              const float *__restrict__ rh, float *__restrict__ full, float *__restrict__ th_root, float *__restrict__ th_rest) {
    __shared__ float s_pk[BF_GRAD_MAX_NP];
    const int tid = threadIdx.x, nj = T.nj, np = T.np, n_pca = T.n_pca;
    const size_t f = blockIdx.x;
    const int off_leye = T.off_orient + 3, off_reye = T.off_orient + 6;
    for (int i = tid; i < np; i += 64) {
        float x = 0.f;
        if (i >= T.off_pose && i < T.off_pose + T.nbp) x = body_pose[f * T.nbp + (i - T.off_pose)];
        else if (i >= T.off_orient && i < off_leye) x = orient[f * 3 + (i - T.off_orient)];
        else if (i >= off_leye && i < off_reye) x = leye ? leye[f * 3 + (i - off_leye)] : 0.f;
        else if (i >= off_reye && i < T.off_lh) x = reye ? reye[f * 3 + (i - off_reye)] : 0.f;
        else if (i >= T.off_lh && i < T.off_rh) x = lh ? lh[f * n_pca + (i - T.off_lh)] : 0.f;
        else if (i >= T.off_rh && i < T.off_rh + n_pca) x = rh ? rh[f * n_pca + (i - T.off_rh)] : 0.f;
        s_pk[i] = x;
    }
    __syncthreads();
    if (tid < nj) {
        float th[3];
        bf_theta3(s_pk, tid, th, T.th_kind, T.th_off, T.pose_mean, T.hand_comp, n_pca, T.off_lh, T.off_rh);
        if (jaw && T.th_kind[tid] == 1) { th[0] += jaw[f * 3]; th[1] += jaw[f * 3 + 1]; th[2] += jaw[f * 3 + 2]; }
        float *dst = tid == 0 ? th_root + f * 3 : th_rest + f * 3 * (nj - 1) + 3 * (tid - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) { full[f * 3 * nj + tid * 3 + k] = th[k]; dst[k] = th[k]; }
    }
}

// One thread per frame: find_dynamic_lmk_idx_and_bcoords' row, the expression of bf_joints_body (joints_body.h) on the same state.
extern "C" __global__ void __launch_bounds__(64)
bf_smplx_dyn_row_kernel(MeshTab M, const float *__restrict__ state, int n, int *__restrict__ row) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    StateView st = bf_state_view(const_cast<float *>(state) + (size_t)f * bf_state_stride(M.nj, M.npf, M.nb), M.nj, M.npf, M.nb);
    const float *G = st.GR + M.neck_joint * 9;
    float yaw = atan2f(-G[6], sqrtf(G[0] * G[0] + G[3] * G[3]));
    int y = (int)rintf(fminf(-yaw * 180.0f / 3.14159265358979323846f, 39.f));
    if (y < 0) y = y < -39 ? 78 : 39 - y;
    row[f] = y;
}

// grid (n), one wave per frame: the reverse of bf_smplx_pose_assemble_kernel.  tot = dtheta (+ dfull_pose when given);
//   out[f][0 .. 3 NJ)            = tot: the thetas that are inputs themselves (root, body, jaw, eyes) are read from here
//   out[f][3 NJ + h n_pca + c]   = sum over k ascending of hand_comp[h][c][k] tot_hand_h[k]      (h = 0 left, 1 right; 45 entries)
extern "C" __global__ void __launch_bounds__(64)
bf_smplx_pose_reverse_kernel(FitTab T, const float *__restrict__ dtheta, const float *__restrict__ dfull, float *__restrict__ out) {
    __shared__ float s_hand[2 * 45];
    const int tid = threadIdx.x, nj = T.nj, n_pca = T.n_pca, stride = 3 * nj + 2 * n_pca;
    const size_t f = blockIdx.x;
    if (tid < nj) {
        const int kind = T.th_kind[tid], off = T.th_off[tid];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t i = f * 3 * nj + tid * 3 + k;
            const float g = dfull ? dtheta[i] + dfull[i] : dtheta[i];
            out[f * stride + tid * 3 + k] = g;
            if (kind >= 2) s_hand[(kind - 2) * 45 + off * 3 + k] = g;
        }
    }
    __syncthreads();
    if (tid < 2 * n_pca) {
        const int h = tid / n_pca;
        const float *comp = T.hand_comp + (size_t)tid * 45;          // [2][n_pca][45]
        float acc = 0.f;
        for (int k = 0; k < 45; ++k) acc += comp[k] * s_hand[h * 45 + k];
        out[f * stride + 3 * nj + tid] = acc;
    }
}

// One thread per element of rows[n][stride]: the row cut into the caller's blocks, dst[b][f][c - off[b]] = rows[f][c] for the block that
// holds column c (null dst, or no block: dropped).  This is what the host route does with memcpy after its copy back; a few hundred
// floats per frame go through plain loads and stores here, and nothing in it is worth tuning.
extern "C" __global__ void __launch_bounds__(256)
bf_block_scatter_kernel(const float *__restrict__ rows, int n, int stride, BfScatter S) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * stride) return;
    const size_t f = i / stride;
    const int c = (int)(i - f * stride);
    for (int b = 0; b < S.n_blocks && b < BF_SCATTER_MAX; ++b)
        if (S.dst[b] && c >= S.off[b] && c < S.off[b] + S.cnt[b]) S.dst[b][f * S.cnt[b] + (c - S.off[b])] = rows[i];
}
