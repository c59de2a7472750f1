#!/usr/bin/env python3
"""The differentiable SMPL-X model behind smplx.create on one GPU (not part of the bench.py contract): per call, the forward
(DeviceModel.forward_smplx = bf_smplx_forward) and the forward + backward (forward, then DeviceModel.vjp_smplx = bf_smplx_vjp with
cotangents on vertices, the 144 joints and full_pose) at n = 1, 8, 64 and 256 parameter sets on the 10,475-vertex synthetic SMPL-X,
and next to them, re-measured in the same process, the SMPL figures of tools/bench_smpl_grad.py with the ratio.  Wall time from a
host clock around whole calls (each call synchronises the device before it returns), host staging included; the median of --reps
calls after --warmup.  One JSON object per line.   usage: python tools/bench_smplx_grad.py [--reps R] [--warmup W] [--sizes 1,8,64,256]

--shape-space NB,NE widens the model to NB betas and NE expression coefficients (synthetic.widen_shape_space; bf_model_set_shape_space):
betas are then [n, NB], --expression times the calls with expression[n, NE], and every row carries the algorithmic direction bytes of
a call - 12 NV L bytes of directions, L = NB - 10 + NE, walked once per frame by the kernels behind bf_model_set_expression and once
per block of 8 frames by the wide ones (the environment variable BF_SHAPE_EXT_WIDE=1 sends any width through those).

The backward's device time comes from a separate run under
`rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/bench_smplx_grad.py --no-smpl`;
`python tools/bench_smplx_grad.py --summarize <dir>/<name>_results.db` then prints, per n and per kind of call (forward / vjp), the
mean device time of every kernel per call (a call = the dispatches from one bf_smplx_pose_assemble_kernel to the next; the buffer
copies of the staging are the runtime's copy kernels)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bodyfitting_amd import native as N, synthetic as S   # noqa: E402
from bench_smpl_grad import summarize, timed                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--no-smpl", action="store_true", help="skip the SMPL comparison (the run under the profiler)")
    ap.add_argument("--expression", action="store_true", help="time every call with expression coefficients as well (expr_* columns; "
                    "--summarize lists those calls as 'forward +expression' / 'vjp +expression')")
    ap.add_argument("--shape-space", metavar="NB,NE", help="betas and expression coefficients of the model (default: the synthetic model's 10,10)")
    ap.add_argument("--summarize", metavar="DB", help="print the kernel split of a rocprofv3 run of this tool and exit")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, opens="bf_smplx_pose_assemble_kernel")
    gmm = S.make_gmm(seed=0)
    model = S.make_model("smplx", seed=0)
    if a.shape_space:
        model = S.widen_shape_space(model, *(int(v) for v in a.shape_space.split(",")), seed=0)
    dev = N.DeviceModel(model, gmm, device=0)
    n_ext = dev.n_betas - dev.n_core_betas + dev.n_expression
    smpl = None if a.no_smpl else N.DeviceModel(S.make_model("smpl", seed=0), gmm, device=0)
    rng = np.random.default_rng(0)
    f32 = lambda sd, *shape: rng.normal(0, sd, shape).astype(np.float32)          # noqa: E731
    for n in (int(s) for s in a.sizes.split(",")):
        p = (f32(0.7, n, dev.n_betas), f32(0.8, n, 3), f32(0.3, n, 63), f32(0.2, n, 3), f32(0.2, n, 3), f32(0.2, n, 3), f32(0.4, n, 6), f32(0.4, n, 6))
        cot = dict(dverts=f32(1, n, dev.n_verts, 3), djoints_all=f32(1, n, dev.n_joints_all, 3), dfull_pose=f32(1, n, 3 * dev.n_joints))
        fwd = timed(lambda: dev.forward_smplx(*p), a.reps, a.warmup)
        bwd = timed(lambda: dev.vjp_smplx(*p, **cot), a.reps, a.warmup)
        both = timed(lambda: (dev.forward_smplx(*p), dev.vjp_smplx(*p, **cot)), a.reps, a.warmup)
        row = {"n": n, "verts": dev.n_verts, "reps": a.reps,
               "forward_ms": round(fwd[0], 3), "forward_min_ms": round(fwd[1], 3),
               "vjp_ms": round(bwd[0], 3), "vjp_min_ms": round(bwd[1], 3),
               "forward_backward_ms": round(both[0], 3), "forward_backward_min_ms": round(both[1], 3),
               "forward_backward_per_frame_us": round(both[0] * 1e3 / n, 1)}
        # one walk over the directions: the forward's vertex delta; the vjp's forward walks them again and its reverse the second copy
        walks = -(-n // 8) if dev.shape_ext_wide else n
        row.update(n_betas=dev.n_betas, n_expression=dev.n_expression, wide_kernels=dev.shape_ext_wide,
                   direction_bytes_per_walk=12 * dev.n_verts * n_ext, direction_walks_forward=walks, direction_walks_vjp=2 * walks)
        if a.expression and dev.n_expression:          # the same calls with expression[n, n_expression] (bf_smplx_forward_expr / bf_smplx_vjp_expr)
            e = f32(0.7, n, dev.n_expression)
            x_fwd = timed(lambda: dev.forward_smplx(*p, expression=e), a.reps, a.warmup)
            x_bwd = timed(lambda: dev.vjp_smplx(*p, **cot, expression=e), a.reps, a.warmup)
            x_both = timed(lambda: (dev.forward_smplx(*p, expression=e), dev.vjp_smplx(*p, **cot, expression=e)), a.reps, a.warmup)
            row.update(expr_forward_ms=round(x_fwd[0], 3), expr_vjp_ms=round(x_bwd[0], 3), expr_forward_backward_ms=round(x_both[0], 3),
                       expr_forward_backward_min_ms=round(x_both[1], 3), expr_over_plain=round(x_both[0] / both[0], 3))
        if smpl is not None:
            q = (np.ascontiguousarray(p[0][:, :10]), p[1], f32(0.3, n, 69))
            sc = (f32(1, n, smpl.n_verts, 3), f32(1, n, smpl.n_joint_map, 3), f32(1, n, smpl.n_joints + smpl.n_selector, 3))
            s_both = timed(lambda: (smpl.forward(*q), smpl.vjp(*q, *sc)), a.reps, a.warmup)
            s_bwd = timed(lambda: smpl.vjp(*q, *sc), a.reps, a.warmup)
            row.update(smpl_forward_backward_ms=round(s_both[0], 3), smpl_vjp_ms=round(s_bwd[0], 3),
                       forward_backward_over_smpl=round(both[0] / s_both[0], 2), vjp_over_smpl=round(bwd[0] / s_bwd[0], 2))
        print(json.dumps(row), flush=True)
    dev.close()
    if smpl is not None:
        smpl.close()


if __name__ == "__main__":
    main()
