"""OpenPose hand estimator throughput on one GPU (synthetic weights `synthetic.make_openpose_hand_weights(0)`, synthetic 512 x 512
views with two square hand boxes each, as util.handDetect gives them).

Prints one JSON line: the time of one frame (every hand of every view through Hand.__call__: crops, network at four scales, maps,
Gaussian filter, component pick), hands per second, the frame's useful FLOPs from the layer shapes (Mconv1 with its 150 input
channels), and - with --stats, the kernel_stats.csv or results .db of a rocprofv3 `--kernel-trace --stats` run of this same
command - the achieved TF/s of the stages' 7 x 7 convolutions (bf_op_conv7_kernel) and its share of the 157.3 TF fp32-MFMA peak.

Usage:  python tools/bench_openpose_hand.py [--views 48] [--batch 16] [--reps 2] [--stats kernel_stats.csv | results.db]
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
from bodyfitting_amd import openpose_hand as OH, synthetic as S          # noqa: E402

PEAK_TF = 157.3


def hand_flops(side):
    """useful FLOPs of one square crop at the four scales -> (all convolutions, the stages' 7 x 7 ones)"""
    total = conv7 = 0
    for _, _, Hp, Wp in OH.hand_scale_dims(side, side):
        px, div = Hp * Wp, 1
        for v in OH.HAND_VGG:
            if v == "pool":
                div *= 4
                continue
            total += 2 * v[3] * v[3] * v[1] * v[2] * px // div
        q = px // 64
        for _, cin, cout, k in OH.HAND_STAGE1:
            total += 2 * k * k * cin * cout * q
        for _ in range(5):
            for _, cin, cout, k in OH.HAND_STAGE_T:
                f = 2 * k * k * cin * cout * q
                total += f
                conv7 += f if k == 7 else 0
    return total, conv7


def conv7_ns(path):
    """total bf_op_conv7_kernel time of a rocprofv3 run: its kernel_stats.csv, or its results database (.db)"""
    if path.endswith(".db"):
        import sqlite3
        row = sqlite3.connect(path).execute("select sum(end - start) from kernels where name like 'bf_op_conv7_kernel%'").fetchone()
        return float(row[0] or 0)
    with open(path) as fh:
        return sum(float(r["TotalDurationNs"]) for r in csv.DictReader(fh) if r.get("Name", "").startswith("bf_op_conv7_kernel"))


def frame_boxes(views, size):
    boxes = []
    for v in range(views):
        a = 96 + 16 * (v % 6)
        boxes.append((v, 40 + 3 * v, 60 + 2 * v, a, a))
        b = 128 + 8 * (v % 5)
        boxes.append((v, size - b - 30, size - b - 20 - v, b, b))
    return boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    net = OH.OpenPoseHand(S.make_openpose_hand_weights(0), device=0, max_hands=a.batch, max_h=a.size, max_w=a.size)
    base = S.make_hmr_images(0, ((a.size, a.size),) * 4)
    views = np.ascontiguousarray(np.stack([base[i % 4][:, :, ::-1] for i in range(a.views)]))
    boxes = frame_boxes(a.views, a.size)
    net.detect(views, boxes)                                           # warm-up (allocations)
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        net.detect(views, boxes)
        times.append(time.perf_counter() - t0)
    f = min(times)
    flops = [hand_flops(b[3]) for b in boxes]
    total, conv7 = sum(x[0] for x in flops), sum(x[1] for x in flops)
    res = {"metric": "openpose_hand_frame_s", "views": a.views, "hands": len(boxes), "size": a.size, "frame_s": f,
           "hands_per_s": len(boxes) / f, "frame_tflop": total / 1e12, "frame_tflops_achieved": total / f / 1e12}
    if a.stats and os.path.exists(a.stats):
        runs = 1 + a.reps                                              # every frame this run pushed through the network
        ns = conv7_ns(a.stats)
        if ns:
            tf = conv7 * runs / ns / 1e3
            res.update(conv7_ms_per_frame=ns / 1e6 / runs, conv7_tflops=tf, conv7_peak_share=tf / PEAK_TF)
    net.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
