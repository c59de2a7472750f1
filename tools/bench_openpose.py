"""OpenPose body estimator throughput on one GPU (synthetic weights `synthetic.make_openpose_weights(0)`, synthetic 512 x 512 views).

Prints one JSON line: views/s for a 48-view frame of 512 x 512 images (Body.__call__ per view: maps, peaks, limb scores and the host
assembly), ms per view at n = 1, the share of the frame spent after the maps (peaks, limb scores, host assembly), and - with
--stats, a rocprofv3 `--kernel-trace --stats` kernel_stats.csv of this same run - the achieved TF/s of the stages' 7 x 7
convolutions (bf_op_conv7_kernel; useful FLOPs, 185 input channels for Mconv1) and its share of the 157.3 TF fp32-MFMA peak.

Usage:  python tools/bench_openpose.py [--views 48] [--batch 16] [--reps 2] [--stats kernel_stats.csv]
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bodyfitting_amd import openpose as O, synthetic as S          # noqa: E402

PEAK_TF = 157.3


def conv7_flops(H, W, views):
    """useful FLOPs of the 7 x 7 layers for `views` images of H x W at the four scales"""
    per_px = 2 * 49 * 2 * (185 * 128 + 4 * 128 * 128)             # both branches: Mconv1 (185 in) and Mconv2..5, per stage
    total = 0
    for d in O.scale_dims(H, W):
        total += (d[2] // 8) * (d[3] // 8) * per_px * 5
    return total * views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    net = O.OpenPose(S.make_openpose_weights(0), device=0, max_batch=a.batch, max_h=a.size, max_w=a.size)
    base = S.make_hmr_images(0, ((a.size, a.size),) * 4)
    views = np.stack([base[i % 4][:, :, ::-1] for i in range(a.views)])
    net.detect_many(views[:1])                                         # warm-up (allocations at the single-view size)
    t0 = time.perf_counter()
    net.detect_many(views[:1])
    one = time.perf_counter() - t0
    net.detect_many(views)                                             # warm-up at the batch size
    frame, maps = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        net.detect_many(views)
        frame.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for s in range(0, a.views, a.batch):
            chunk = np.ascontiguousarray(views[s:s + a.batch])
            O._lib.check(net._lib.bf_openpose_maps(net._h, len(chunk), a.size, a.size, net._u8(chunk), None, None), "bf_openpose_maps")
        maps.append(time.perf_counter() - t0)
    f, m = min(frame), min(maps)
    res = {"metric": "openpose_views_per_s", "views": a.views, "size": a.size, "views_per_s": a.views / f, "frame_s": f,
           "ms_per_view_n1": one * 1e3, "post_share": max(0.0, (f - m) / f)}
    if a.stats and os.path.exists(a.stats):
        # every view this run pushed through the network: 2 single ones, then the frame 1 + 2 * reps times
        n_views = 2 + a.views * (1 + 2 * a.reps)
        with open(a.stats) as fh:
            for row in csv.DictReader(fh):
                if row.get("Name", "").startswith("bf_op_conv7_kernel"):
                    ns = float(row["TotalDurationNs"])
                    tf = conv7_flops(a.size, a.size, n_views) / ns / 1e3
                    res.update(conv7_ms_per_view=ns / 1e6 / n_views, conv7_tflops=tf, conv7_peak_share=tf / PEAK_TF)
    net.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
