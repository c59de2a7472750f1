// Shared by the LBAM inpainting kernels (inpaint_kernels.hip) and their host side (inpaint_api.hip): the descriptor of one
// attention convolution and its epilogues.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum {
    IP_EPI_RAW = 0,   // y0 = conv(x), y1 = conv(xm) (test hook)
    IP_EPI_ENC = 1,   // ForwardAttentionLayer + LeakyReLU: y0 = leaky(conv(x) * gaussA(conv(xm))), y1 = relu(conv(xm))^0.8
    IP_EPI_REV = 2,   // ReverseMaskConv: y0 = gaussA(conv(x)), y1 = relu(conv(x))^0.8
    IP_EPI_DEC = 3,   // ReverseAttention, the deconv half: y0 = leaky(deconv(x) * aux0)
    IP_EPI_OUT = 4    // dc7, (tanh + 1) / 2 and Inpainter's blend: y0 = o * (1 - aux1) + aux0 * aux1 (aux0, aux1 4 floats per pixel)
};

// One 4 x 4 convolution, stride 2, padding 1 (deconv = 0), or one ConvTranspose2d(4, 2, 1) as four 2 x 2 phases (deconv = 1), on
// NHWC fp32 as an implicit GEMM: M = n x the GEMM's pixel grid (conv: the Ho x Wo outputs; deconv: the Hi x Wi inputs, one output
// per phase each), N = cout, K = 16 cin in (ky, kx, ci) order (deconv: 4 cin in (ty, tx, ci) order, per phase).  Weights are packed
// [K][coutp] (deconv: four phases of that, py-major).  A second A operand xm with its own weights wm (ForwardAttentionLayer's
// maskConv) runs over the same K in the same launch.  cin, ldx and ldxm are multiples of 4 and the operands 16-byte aligned.
// splits > 1: K is cut into chunks of kper and each chunk's sums go to `part`, [phase][split][M][coutp] per operand; the reduction
// kernel adds them in split order and runs the epilogue.
struct IpConv {
    const float *x, *xm, *w, *wm;
    float *y0, *y1;
    const float *aux0, *aux1;
    float *part;
    int ldx, ldxm, cin, cout, coutp, ld0, ld1, ldaux;
    int n, Hi, Wi, Ho, Wo;
    int deconv, epi, splits, kper;
    float ga, gmu, gs1, gs2;      // GaussActivation (a, mu, sigma1, sigma2), clamped
};

// the kernels of inpaint_kernels.hip, declared once for the definitions and the host file that launches them
#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" __global__ void bf_ip_prepare_kernel(long long npx, const uint8_t *img, const uint8_t *msk, float4 *x, float4 *mk, float4 *rmk);
extern "C" __global__ void bf_ip_enc_kernel(IpConv p);
extern "C" __global__ void bf_ip_rev128_kernel(IpConv p);
extern "C" __global__ void bf_ip_rev64_kernel(IpConv p);
extern "C" __global__ void bf_ip_dec128_kernel(IpConv p);
extern "C" __global__ void bf_ip_dec64_kernel(IpConv p);
extern "C" __global__ void bf_ip_reduce_kernel(IpConv p, int dual);
extern "C" __global__ void bf_ip_faces_kernel(int n_faces, int H, int W, const uint8_t *img, const float *uv, uint8_t *sel, int *err);
extern "C" __global__ void bf_ip_fill_kernel(int n_faces, int H, int W, const float *uv, const uint8_t *sel, uint8_t *mask);
extern "C" __global__ void bf_ip_morph_kernel(int op, int k, int n, int H, int W, int C, const uint8_t *in, uint8_t *out);
extern "C" __global__ void bf_ip_quantize_kernel(long long count, const float *out, uint8_t *img, uint8_t *mask);
extern "C" __global__ void bf_ip_combine_kernel(long long count, const uint8_t *img, const uint8_t *img2, const uint8_t *mask, const uint8_t *mask_d, uint8_t *out);
#pragma GCC visibility pop
