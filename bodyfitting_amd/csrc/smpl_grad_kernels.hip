// Reverse of models.smpl.SMPL.forward (smplx lbs() + the wrapper of models/smpl.py:69-83) for gfx950: the two kernels the
// stand-alone vector-Jacobian product bf_smpl_vjp (smpl_grad_api.hip) adds around the dense schedule's reverse mesh pass.
//
//   bf_smpl_vjp_fold_kernel   dL/d(joints49), dL/d(joints45), dL/dvertices -> dL/dvertices of the mesh reverse + dL/d(posed chain joints)
//   bf_smpl_vjp_chain_kernel  the reduced mesh-reverse row + dL/d(posed chain joints) -> dL/dtheta, dL/dbeta
//
// The math is the reverse half of oracle/analytic.py: loss_grad, with the skinning sums taken from bf_ext_reduce_kernel's row.
// No float atomics: every sum has a fixed order, so a call's bits do not depend on timing.
#include "bf_internal.h"
#include "pose_state_body.h"

#define BF_VJP_FOLD_THREADS 256
#define BF_VJP_MAX_ALL 128     // chain + selector + extra joints the fold stages in LDS (SMPL: 24 + 21 + 9)
#define BF_VJP_MAX_MAP 256     // joint_map entries (SMPL: 49)
#define BF_VJP_MAX_JOINTS 64   // chain joints: one lane each in the chain kernel's single wave (SMPL: 24)

// grid (ceil(NV / 256), n), 256 threads.  Per frame f:
//   dall[j] = sum over i ascending with joint_map[i] == j of djoints[i]  (+ djoints_ori[j] for j < NJ + n_selector)
//   dchain[f][j] = dall[j] for the NJ chain joints (workgroup x = 0 writes it)
//   dv[f][v] = dvertices[f][v] + sum over s ascending with selector_ids[s] == v of dall[NJ + s]
//              + sum over e ascending of J_regressor_extra[e][v] dall[NJ + n_selector + e]
// Any of dvertices / djoints / djoints_ori may be null (= zero).
extern "C" __global__ void __launch_bounds__(BF_VJP_FOLD_THREADS)
bf_smpl_vjp_fold_kernel(MeshTab M, const float *__restrict__ dvertices, const float *__restrict__ djoints, const float *__restrict__ djoints_ori,
                        float *__restrict__ dv, float *__restrict__ dchain) {
    __shared__ float s_dall[BF_VJP_MAX_ALL * 3];
    __shared__ int s_map[BF_VJP_MAX_MAP];
    __shared__ int s_sel[BF_VJP_MAX_ALL];
    const int nj = M.nj, nv = M.nv, nsel = M.n_selector, ne = M.n_extra, nmap = M.n_joint_map;
    const int n_ori = nj + nsel, n_all = n_ori + ne;
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < nmap; i += BF_VJP_FOLD_THREADS) s_map[i] = M.joint_map[i];
    for (int i = tid; i < nsel; i += BF_VJP_FOLD_THREADS) s_sel[i] = M.selector_ids[i];
    __syncthreads();
    for (int i = tid; i < n_all * 3; i += BF_VJP_FOLD_THREADS) {
        const int j = i / 3, k = i - j * 3;
        float acc = 0.f;
        if (djoints) {
            const float *dj = djoints + (size_t)f * nmap * 3 + k;
            for (int q = 0; q < nmap; ++q)
                if (s_map[q] == j) acc += dj[q * 3];
        }
        if (djoints_ori && j < n_ori) acc += djoints_ori[((size_t)f * n_ori + j) * 3 + k];
        s_dall[i] = acc;
        if (j < nj && blockIdx.x == 0) dchain[((size_t)f * nj + j) * 3 + k] = acc;
    }
    __syncthreads();
    const int v = blockIdx.x * BF_VJP_FOLD_THREADS + tid;
    if (v >= nv) return;
    float sel[3] = {0.f, 0.f, 0.f}, ext[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < nsel; ++s)
        if (s_sel[s] == v) {
            sel[0] += s_dall[(nj + s) * 3]; sel[1] += s_dall[(nj + s) * 3 + 1]; sel[2] += s_dall[(nj + s) * 3 + 2];
        }
    for (int e = 0; e < ne; ++e) {
        const float w = M.j_extra[(size_t)e * nv + v];          // (row e over the vertices: coalesced)
        const float *d = s_dall + (n_ori + e) * 3;
        ext[0] += w * d[0]; ext[1] += w * d[1]; ext[2] += w * d[2];
    }
    const size_t o = ((size_t)f * nv + v) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = dvertices ? dvertices[o + k] : 0.f;
        dv[o + k] = (g + sel[k]) + ext[k];
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
// Leaves to root over the levels of FitTab (level_start / level_joints); a parent takes its children's contributions in the
// order of its CSR child list - one writer per joint and step, no atomics.
extern "C" __global__ void __launch_bounds__(64)
bf_smpl_vjp_chain_kernel(FitTab T, const float *__restrict__ state, const float *__restrict__ ext, int ext_stride,
                         const float *__restrict__ dchain, float *__restrict__ dtheta, float *__restrict__ dbeta) {
    constexpr int MJ = BF_VJP_MAX_JOINTS;
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
}
