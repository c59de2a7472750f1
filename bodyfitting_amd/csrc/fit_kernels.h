// What fit_kernels.hip defines for other files, declared once; it includes this itself, so a prototype that differs from its definition does not compile.
#pragma once
#include "bf_internal.h"

#pragma GCC visibility push(hidden)       // (a kernel's host-side handle does not follow -fvisibility: see the Makefile)
extern "C" hipError_t bf_fit_launch_table(const FitTab *T, const FrameIO *io, const HyperDev *hp, int n_iters, int mode, const float *adam_tab, int adam_t0,
                                          size_t smem, hipStream_t stream, hipEvent_t done);
extern "C" void bf_fit_image_segments(int nj, int nb, int npf, int ns, int nl, int np, int seg[6]);
extern "C" size_t bf_fit_smem_bytes(int nj, int nb, int npf, int ns, int nl, int np, int nviews);
extern "C" bool bf_fit_is_sized_smpl(const FitTab *T);
extern "C" hipError_t bf_fit_launch(const FitTab *T, const FrameIO *io, const HyperDev *hp, int n_iters, int mode, const float *adam_tab, int adam_t0, size_t smem,
                                    hipStream_t stream, hipEvent_t done);
#pragma GCC visibility pop
