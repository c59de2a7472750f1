// The SMPL-X specific ends of smplx.create(...).forward and of its reverse for gfx950 (smplx_grad_api.hip): what bf_smplx_forward /
// bf_smplx_vjp add around the pose-state kernel, the mesh passes, bf_ext_reduce_kernel and bf_smpl_vjp_chain_kernel.
//
//   bf_smplx_pose_assemble_kernel  the eight parameter blocks -> full_pose (hands = PCA . components, + pose_mean, jaw as an input)
//   bf_smplx_dyn_row_kernel        the contour-table row the neck chain's yaw selects (an output of the forward)
//   bf_smplx_vjp_fold_kernel       dL/d(joints135), dL/d(joints144), dL/dvertices -> dL/dvertices of the mesh reverse + dL/d(chain joints)
//   bf_smplx_pose_reverse_kernel   dL/dtheta (+ dL/dfull_pose) -> the pass-through thetas and the hand PCA coefficients' gradients
//
// No float atomics: every sum has a fixed order, so a call's bits do not depend on timing.
#include "bf_internal.h"

#define BF_XVJP_FOLD_THREADS 256
#define BF_XVJP_MAX_ALL 192      // chain + selector + extra + landmark joints the fold stages in LDS (SMPL-X: 55 + 21 + 0 + 68)
#define BF_XVJP_MAX_MAP 256      // joint_map entries (SMPL-X: 135)
#define BF_XVJP_MAX_SEL 64       // selector vertices (SMPL-X: 21)
#define BF_XVJP_MAX_LMK 96       // face landmarks (SMPL-X: 51 static + 17 on the contour), three (vertex, weight) entries each
#define BF_XVJP_MAX_NP 128       // packed parameters per frame (SMPL-X: 98)
#define BF_XVJP_MAX_JOINTS 64    // chain joints: one lane each

// grid (n), one wave per frame.  The blocks go into the optimiser-order parameter vector in LDS and every joint's theta is then
// bf_theta3 of it - the expressions bf_pose_state_kernel's packed path evaluates, so equal values give equal bits there and here.
// The jaw (th_kind 1: a constant of the packed path) takes `jaw` on top when it is given.  leye / reye / lh / rh / jaw may be
// null (= zeros).  Out: full[n][3 NJ], and the same thetas as bf_pose_state_kernel's non-packed path reads them:
// th_root[n][3], th_rest[n][3 (NJ - 1)].
extern "C" __global__ void __launch_bounds__(64)
bf_smplx_pose_assemble_kernel(FitTab T, const float *__restrict__ orient, const float *__restrict__ body_pose, const float *__restrict__ jaw,
                              const float *__restrict__ leye, const float *__restrict__ reye, const float *__restrict__ lh,
                              const float *__restrict__ rh, float *__restrict__ full, float *__restrict__ th_root, float *__restrict__ th_rest) {
    __shared__ float s_pk[BF_XVJP_MAX_NP];
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

// grid (ceil(NV / 256), n), 256 threads.  All joints in smplx order: chain | selector vertices | J_regressor_extra rows | landmarks.
// Per frame f:
//   dall[j] = sum over i ascending with joint_map[i] == j of djoints[i]  + djoints_all[j]
//   dchain[f][j] = dall[j] for the NJ chain joints (workgroup x = 0 writes it)
//   dv[f][v] = dvertices[f][v] + sum over s ascending with selector_ids[s] == v of dall[NJ + s]
//              + sum over e ascending of J_regressor_extra[e][v] dall[NJ + n_selector + e]
//              + sum over the landmark entries q = 3 l + c ascending with lmk_vid[f][q] == v of lmk_w[f][q] dall[first landmark + l]
// lmk_vid / lmk_w: the corner vertices and barycentric weights the forward recompute used for this frame (bf_joints_body); the
// row choice behind them is an integer look-up and carries no gradient.  Several landmarks share vertices, hence a gather.
// Any of dvertices / djoints / djoints_all may be null (= zero).
extern "C" __global__ void __launch_bounds__(BF_XVJP_FOLD_THREADS)
bf_smplx_vjp_fold_kernel(MeshTab M, const float *__restrict__ dvertices, const float *__restrict__ djoints, const float *__restrict__ djoints_all,
                         const int *__restrict__ lmk_vid, const float *__restrict__ lmk_w, float *__restrict__ dv, float *__restrict__ dchain) {
    __shared__ float s_dall[BF_XVJP_MAX_ALL * 3];
    __shared__ int s_map[BF_XVJP_MAX_MAP];
    __shared__ int s_sel[BF_XVJP_MAX_SEL];
    __shared__ int s_lv[BF_XVJP_MAX_LMK * 3];
    __shared__ float s_lc[BF_XVJP_MAX_LMK * 3 * 3];       // per entry: weight x the landmark's cotangent
    const int nj = M.nj, nv = M.nv, nsel = M.n_selector, ne = M.n_extra, nmap = M.n_joint_map, nlm = M.n_lmk_static + M.n_lmk_dyn;
    const int n_ori = nj + nsel, lm0 = n_ori + ne, n_all = lm0 + nlm;
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < nmap; i += BF_XVJP_FOLD_THREADS) s_map[i] = M.joint_map[i];
    for (int i = tid; i < nsel; i += BF_XVJP_FOLD_THREADS) s_sel[i] = M.selector_ids[i];
    for (int i = tid; i < nlm * 3; i += BF_XVJP_FOLD_THREADS) s_lv[i] = lmk_vid[(size_t)f * nlm * 3 + i];
    __syncthreads();
    for (int i = tid; i < n_all * 3; i += BF_XVJP_FOLD_THREADS) {
        const int j = i / 3, k = i - j * 3;
        float acc = 0.f;
        if (djoints) {
            const float *dj = djoints + (size_t)f * nmap * 3 + k;
            for (int q = 0; q < nmap; ++q)
                if (s_map[q] == j) acc += dj[q * 3];
        }
        if (djoints_all) acc += djoints_all[((size_t)f * n_all + j) * 3 + k];
        s_dall[i] = acc;
        if (j < nj && blockIdx.x == 0) dchain[((size_t)f * nj + j) * 3 + k] = acc;
    }
    __syncthreads();
    for (int i = tid; i < nlm * 9; i += BF_XVJP_FOLD_THREADS) {
        const int q = i / 3, k = i - q * 3, l = q / 3;
        s_lc[i] = lmk_w[(size_t)f * nlm * 3 + q] * s_dall[(lm0 + l) * 3 + k];
    }
    __syncthreads();
    const int v = blockIdx.x * BF_XVJP_FOLD_THREADS + tid;
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
        dv[o + k] = ((g + sel[k]) + ext[k]) + lmk[k];
    }
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
