#!/usr/bin/env python3
"""The differentiable drop-in models.smpl.SMPL on one GPU (not part of the bench.py contract): per call, the forward
(DeviceModel.forward = bf_smpl_forward) and the forward + backward (forward, then DeviceModel.vjp = bf_smpl_vjp with cotangents on
vertices, joints and joints_ori) at n = 1, 8, 64 and 256 parameter sets on the 6,890-vertex synthetic SMPL.  Wall time from a
host clock around whole calls (each call synchronises the device before it returns), host staging included; the median of --reps
calls after --warmup.  One JSON object per line.   usage: python tools/bench_smpl_grad.py [--reps R] [--warmup W] [--sizes 1,8,64,256]

The kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/bench_smpl_grad.py`;
`python tools/bench_smpl_grad.py --summarize <dir>/<name>_results.db` then prints, per n and per kind of call (forward / vjp), the mean
device time of every kernel per call (a call = the dispatches from one bf_pose_state_kernel to the next; the buffer copies of the
staging are the runtime's copy kernels)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bodyfitting_amd import native as N, synthetic as S   # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def summarize(db, opens="bf_pose_state_kernel"):
    """`opens`: the kernel whose dispatch starts a call of the tool that was traced"""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, grid_x, workgroup_x, duration from kernels order by start").fetchall()
    calls, cur = [], None
    for name, gx, wx, dur in rows:
        if name.startswith(opens):
            cur = {"n": gx // wx, "kernels": {}}
            calls.append(cur)
        if cur is not None:
            k = "copies (runtime)" if name.startswith("__amd_rocclr") else name.split("(")[0]
            cur["kernels"][k] = cur["kernels"].get(k, 0.0) + dur * 1e-3
    groups = {}
    for c in calls:
        kind = ("vjp" if "bf_model_vjp_fold_kernel" in c["kernels"] else "forward") + (" +expression" if "bf_expr_chain_kernel" in c["kernels"] or "bf_shape_ext_chain_kernel" in c["kernels"] else "")
        groups.setdefault((c["n"], kind), []).append(c["kernels"])
    for (n, kind), cs in sorted(groups.items()):
        names = sorted({k for c in cs for k in c})
        mean = {k: round(sum(c.get(k, 0.0) for c in cs) / len(cs), 2) for k in names}
        print(json.dumps({"n": n, "call": kind, "calls": len(cs), "device_us_per_call": round(sum(mean.values()), 1), "kernels_us": mean}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--summarize", metavar="DB", help="print the kernel split of a rocprofv3 run of this tool and exit")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    model, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    dev = N.DeviceModel(model, gmm, device=0)
    rng = np.random.default_rng(0)
    for n in (int(s) for s in a.sizes.split(",")):
        betas = rng.normal(0, 0.7, (n, 10)).astype(np.float32)
        orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
        pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
        dv = rng.normal(0, 1, (n, dev.n_verts, 3)).astype(np.float32)
        dj = rng.normal(0, 1, (n, dev.n_joint_map, 3)).astype(np.float32)
        djo = rng.normal(0, 1, (n, dev.n_joints + dev.n_selector, 3)).astype(np.float32)
        fwd = timed(lambda: dev.forward(betas, orient, pose), a.reps, a.warmup)
        bwd = timed(lambda: dev.vjp(betas, orient, pose, dv, dj, djo), a.reps, a.warmup)
        both = timed(lambda: (dev.forward(betas, orient, pose), dev.vjp(betas, orient, pose, dv, dj, djo)), a.reps, a.warmup)
        print(json.dumps({"n": n, "verts": dev.n_verts, "reps": a.reps,
                          "forward_ms": round(fwd[0], 3), "forward_min_ms": round(fwd[1], 3),
                          "vjp_ms": round(bwd[0], 3), "vjp_min_ms": round(bwd[1], 3),
                          "forward_backward_ms": round(both[0], 3), "forward_backward_min_ms": round(both[1], 3),
                          "forward_backward_per_frame_us": round(both[0] * 1e3 / n, 1)}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
