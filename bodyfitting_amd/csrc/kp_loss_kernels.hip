// The stand-alone keypoint loss for gfx950: multiview_keypoint_loss (smplify/loss.py:139-230) with MaxMixturePrior's merged
// likelihood (smplify/prior.py:181-196), and its vector-Jacobian product with respect to the joints, the body pose and the betas.
// Host side: kp_loss_api.hip (bf_keypoint_loss).  The batch kernels' arithmetic for the same terms: bf_kp_loss_body (loss_bodies.h)
// and the GMM / angle / shape phases of the fit kernel; here the joints are an INPUT, so nothing of a body model is needed.
//
//   bf_keypoint_loss_kernel   grid (n problems), 512 threads, one workgroup per problem, four phases:
//     1. reprojection   thread (row j = tid % NLP, view slot vs = tid / NLP), NLP = rows padded to 32, slots = 512 / NLP: the slot
//                       takes the views v = vs (mod slots) in ascending order.  The cameras of 64 views at a time are staged in
//                       LDS (w2c[:3] and K as they come: the projection is the reference's two steps, cam = R X + t, pix = K cam);
//                       keypoints stream from global memory four views ahead.  An absent view is skipped before anything of it is read.
//                       The slots of a row are added in slot order, the rows' loss shares by one wave (lane l: rows l, l + 64, ...
//                       in order, then a fixed xor tree).
//     2. GMM            z_m = P_m^T d_m by one thread per (component, dof) - coalesced over the dof - then one wave per component
//                       for d . z (two rounds of lanes when the dimension is above 64), the first minimum by one thread, and
//                       y = P d of that component alone by four lanes per dof: the gradient is 0.5 (y + z) = 0.5 (P + P^T) d.
//     3. angle prior    on dofs 52, 55, 9, 12, by the threads that write those dofs' gradients
//     4. shape prior
// No atomics; every sum has one order that depends on the sizes alone, so equal inputs give equal bits and a problem's result does
// not depend on the problems beside it.
#include "bf_internal.h"
#include "kp_loss_kernels.h"
#include "wave_ops.h"

extern "C" __global__ void __launch_bounds__(BF_KPL_THREADS) bf_keypoint_loss_kernel(KpLossIO Q, HyperDev H) {
    __shared__ float4 s_part[BF_KPL_THREADS];                     // [slots][NLP] dL/dX and the loss share of (row, slot)
    __shared__ float s_cam[BF_KPL_CHUNK * 24];                    // per staged view: w2c[:3] (12) | K (9) | 3 unused
    __shared__ int s_pres[BF_KPL_CHUNK];
    __shared__ float s_ls[BF_KPL_MAX_ROWS];
    __shared__ float s_pose[BF_KPL_MAX_DIM];                      // the pose, zero-padded to the GMM's dimension
    __shared__ float s_z[BF_KPL_MAX_COMP * BF_KPL_MAX_DIM];       // (P_m^T d_m)[i]
    __shared__ float s_gg[BF_KPL_MAX_DIM];                        // the arg-min component's 0.5 (P + P^T) d
    __shared__ float s_ll[BF_KPL_MAX_COMP];
    __shared__ int s_best;
    const int T = BF_KPL_THREADS;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = Q.n_views, R = Q.n_rows;
    const float gd0 = Q.dterms ? Q.dterms[(size_t)p * 4] : 1.f, gd1 = Q.dterms ? Q.dterms[(size_t)p * 4 + 1] : 1.f;
    const float gd2 = Q.dterms ? Q.dterms[(size_t)p * 4 + 2] : 1.f, gd3 = Q.dterms ? Q.dterms[(size_t)p * 4 + 3] : 1.f;

    // ---- 1. reprojection (loss.py:22-43,45-51,132-136,156-203) ----
    {
        const int NLP = R > 0 ? (R + 31) & ~31 : 32, slots = T / NLP;         // (no rows: a priors-only call)
        const int j = tid % NLP, vs = tid / NLP;
        const bool active = vs < slots && j < R;
        const float ndiv = (V > 0 && Q.divisor) ? (float)Q.divisor[p] : 1.f;
        const float coeff = H.coeff, s2 = H.sigma2, kscale = -gd0 / (coeff * ndiv);
        float x0 = 0.f, x1 = 0.f, x2 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, ls = 0.f;
        if (active) {
            const float *x = Q.joints + ((size_t)p * R + j) * 3;
            x0 = x[0]; x1 = x[1]; x2 = x[2];
        }
        auto one_view = [&](const float *C, float kx, float ky, float kc) {
            const float *Km = C + 12;
            const float c0 = C[0] * x0 + C[1] * x1 + C[2] * x2 + C[3];
            const float c1 = C[4] * x0 + C[5] * x1 + C[6] * x2 + C[7];
            const float c2 = C[8] * x0 + C[9] * x1 + C[10] * x2 + C[11];
            const float p0 = Km[0] * c0 + Km[1] * c1 + Km[2] * c2;
            const float p1 = Km[3] * c0 + Km[4] * c1 + Km[5] * c2;
            const float p2 = Km[6] * c0 + Km[7] * c1 + Km[8] * c2;
            const float u = p0 / p2, w = p1 / p2;
            const float rx = (kx - u) / coeff, ry = (ky - w) / coeff;
            const float ax = s2 + rx * rx, ay = s2 + ry * ry, conf2 = kc * kc;
            ls += conf2 * (s2 * (rx * rx) / ax + s2 * (ry * ry) / ay);
            const float k = conf2 * kscale;
            const float du = k * (2.f * s2 * s2 * rx / (ax * ax)), dw = k * (2.f * s2 * s2 * ry / (ay * ay));
            const float q0 = du / p2, q1 = dw / p2, q2 = -(du * u + dw * w) / p2;
            const float d0 = Km[0] * q0 + Km[3] * q1 + Km[6] * q2;
            const float d1 = Km[1] * q0 + Km[4] * q1 + Km[7] * q2;
            const float d2 = Km[2] * q0 + Km[5] * q1 + Km[8] * q2;
            g0 += C[0] * d0 + C[4] * d1 + C[8] * d2;
            g1 += C[1] * d0 + C[5] * d1 + C[9] * d2;
            g2 += C[2] * d0 + C[6] * d1 + C[10] * d2;
        };
        for (int base = 0; base < V; base += BF_KPL_CHUNK) {
            const int cnt = min(BF_KPL_CHUNK, V - base);
            __syncthreads();                                      // (the previous chunk has been read)
            for (int i = tid; i < cnt * 21; i += T) {
                const int v = i / 21, e = i - v * 21;
                const size_t gv = (size_t)p * V + base + v;
                s_cam[v * 24 + e] = e < 12 ? Q.w2c[gv * 16 + e] : Q.K[gv * 9 + (e - 12)];
            }
            for (int i = tid; i < cnt; i += T) s_pres[i] = Q.present ? (Q.present[(size_t)p * V + base + i] != 0) : 1;
            __syncthreads();
            if (active) {
                const int end = base + cnt;
                const float *kp0 = Q.keypoints + ((size_t)p * V * R + j) * 3;          // + v * R * 3
                for (int v0 = base + (vs - base % slots + slots) % slots; v0 < end; v0 += 4 * slots) {
                    float kk[4][3];
                    bool ok[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int vv = v0 + q * slots;
                        ok[q] = vv < end && s_pres[(vv < end ? vv : base) - base] != 0;
                        kk[q][0] = 0.f; kk[q][1] = 0.f; kk[q][2] = 0.f;
                        if (ok[q]) { const float *kp = kp0 + (size_t)vv * R * 3; kk[q][0] = kp[0]; kk[q][1] = kp[1]; kk[q][2] = kp[2]; }
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (ok[q]) one_view(s_cam + (v0 + q * slots - base) * 24, kk[q][0], kk[q][1], kk[q][2]);
                }
            }
        }
        if (tid < slots * NLP) s_part[tid] = make_float4(g0, g1, g2, ls);
        __syncthreads();
        if (tid < R) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q = 0; q < slots; ++q) { const float4 b = s_part[q * NLP + tid]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
            if (Q.djoints) { float *o = Q.djoints + ((size_t)p * R + tid) * 3; o[0] = a.x; o[1] = a.y; o[2] = a.z; }
            s_ls[tid] = a.w;
        }
        __syncthreads();
        if (wave == 0) {
            float acc = 0.f;
            for (int q = lane; q < R; q += 64) acc += s_ls[q];
            acc = bf_wave_sum(acc);
            if (lane == 0 && Q.terms) Q.terms[(size_t)p * 4] = acc / ndiv;
        }
    }

    // ---- 2. + 3. the GMM prior (prior.py:181-196) and the angle prior (loss.py:54-61) ----
    if (Q.poses) {
        const int D = Q.gmm_dim, M = Q.g_prec ? Q.gmm_comp : 0, PD = Q.pose_dim;
        for (int i = tid; i < BF_KPL_MAX_DIM; i += T) { s_pose[i] = i < PD ? Q.poses[(size_t)p * PD + i] : 0.f; s_gg[i] = 0.f; }
        __syncthreads();
        for (int it = tid; it < M * D; it += T) {
            const int m = it / D, i = it - m * D;
            const float *Pm = Q.g_prec + (size_t)m * D * D, *mu = Q.g_means + (size_t)m * D;
            float z = 0.f;
            for (int jj = 0; jj < D; ++jj) z += Pm[(size_t)jj * D + i] * (s_pose[jj] - mu[jj]);
            s_z[m * BF_KPL_MAX_DIM + i] = z;
        }
        __syncthreads();
        for (int m = wave; m < M; m += T / 64) {
            const float *mu = Q.g_means + (size_t)m * D;
            float a = 0.f;
            for (int i = lane; i < D; i += 64) a += s_z[m * BF_KPL_MAX_DIM + i] * (s_pose[i] - mu[i]);      // (69 dofs: a second round of five lanes)
            a = bf_wave_sum(a);
            if (lane == 0) s_ll[m] = 0.5f * a - Q.g_logw[m];
        }
        __syncthreads();
        if (tid == 0) {
            int best = M > 0 ? 0 : -1;
            for (int m = 1; m < M; ++m)
                if (s_ll[m] < s_ll[best]) best = m;               // strict: ties go to the lowest component, as torch.min returns it
            s_best = best;
        }
        __syncthreads();
        const int best = s_best;
        if (best >= 0) {
            // four lanes per dof (a dimension of at most 128 = 512 / 4), joined by two shuffles inside their wave
            const int i = tid >> 2, q = tid & 3;
            const float *Pm = Q.g_prec + (size_t)best * D * D, *mu = Q.g_means + (size_t)best * D;
            float y = 0.f;
            if (i < D)
                for (int jj = q; jj < D; jj += 4) y += Pm[(size_t)i * D + jj] * (s_pose[jj] - mu[jj]);
            y += __shfl_xor(y, 1);
            y += __shfl_xor(y, 2);
            if (q == 0 && i < D) s_gg[i] = 0.5f * (y + s_z[best * BF_KPL_MAX_DIM + i]);
        }
        __syncthreads();
        if (tid < PD && Q.dposes) {
            float g = gd1 * H.w_pose * s_gg[tid];
            const float sg = tid == 52 ? 1.f : (tid == 55 || tid == 9 || tid == 12) ? -1.f : 0.f;
            if (sg != 0.f) { const float e = expf(s_pose[tid] * sg); g += gd2 * H.w_angle * (2.f * sg * (e * e)); }
            Q.dposes[(size_t)p * PD + tid] = g;
        }
        if (tid == 0 && Q.terms) {
            const float e0 = expf(s_pose[52]), e1 = expf(-s_pose[55]), e2 = expf(-s_pose[9]), e3 = expf(-s_pose[12]);
            Q.terms[(size_t)p * 4 + 1] = best >= 0 ? H.w_pose * s_ll[best] : 0.f;
            Q.terms[(size_t)p * 4 + 2] = H.w_angle * (e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3);
        }
    } else if (tid == 0 && Q.terms) {
        Q.terms[(size_t)p * 4 + 1] = 0.f;
        Q.terms[(size_t)p * 4 + 2] = 0.f;
    }

    // ---- 4. shape prior (loss.py:214) ----
    if (Q.betas) {
        const int NB = Q.n_betas;
        if (tid < NB && Q.dbetas) Q.dbetas[(size_t)p * NB + tid] = gd3 * H.w_shape * (2.f * Q.betas[(size_t)p * NB + tid]);
        if (tid == 64 && Q.terms) {
            float a = 0.f;
            for (int i = 0; i < NB; ++i) { const float b = Q.betas[(size_t)p * NB + i]; a += b * b; }
            Q.terms[(size_t)p * 4 + 3] = H.w_shape * a;
        }
    } else if (tid == 64 && Q.terms) Q.terms[(size_t)p * 4 + 3] = 0.f;
}
