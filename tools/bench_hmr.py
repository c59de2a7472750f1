"""HMR on the MI355X: batch-1 latency, images/s at n = 32 and 256, the share of the fp32-MFMA peak, and a genebody-style frame (HMR on
the keyframe, then the 1 x 48 x 100 fit) against the fit alone.  Synthetic weights (synthetic.make_hmr_weights) and 512 x 512 images; prints one JSON line.

    python tools/bench_hmr.py [--reps 20]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_hmr.py --reps 3`."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bodyfitting_amd import hmr as H, native as N, synthetic as S  # noqa: E402

PEAK_FP32_MFMA = 157.3e12


def flops_per_image():
    """2 x multiply-adds of the convolutions and the regressor (x3), from the layer shapes"""
    macs, size = 0, 112
    for conv, _, cin, cout, k, s, p in H.conv_layers():
        if conv == "conv1":
            macs += 112 * 112 * cout * cin * k * k
            size = 56
            continue
        if conv.endswith("conv2"):
            out = (size + 2 * p - k) // s + 1
            macs += out * out * cout * cin * k * k
            conv2_out = out
        elif conv.endswith("conv3"):
            macs += conv2_out * conv2_out * cout * cin
        elif conv.endswith("downsample.0"):
            macs += conv2_out * conv2_out * cout * cin
            size = conv2_out
        else:                                                       # conv1 of a block, 1 x 1 at the block input size
            macs += size * size * cout * cin
    macs += 3 * (2205 * 1024 + 1024 * 1024 + 1024 * 157)
    return 2 * macs


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    sd, mean = S.make_hmr_weights(0)
    img = S.make_hmr_images(0, ((512, 512),))[0]
    fl = flops_per_image()
    out = {"gflop_per_image": fl / 1e9}
    net = H.HMR(sd, mean, device=0, max_batch=256)
    for n in (1, 32, 256):
        batch = np.ascontiguousarray(np.stack([img] * n))
        t = timed(lambda: net.regress(batch), max(2, args.reps // (1 if n == 1 else 4)))
        out[f"n{n}_ms"] = t * 1e3
        out[f"n{n}_images_per_s"] = n / t
        out[f"n{n}_peak_fraction"] = n * fl / t / PEAK_FP32_MFMA
    # a genebody frame: HMR on the keyframe image (post-processing included), then the 1 x 48 x 100 fit
    model, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    prob = S.make_problem(model, frame=0, n_views=48)
    dev = N.DeviceModel(model, gmm, device=0)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    batch = N.FrameBatch(dev, 1, 48)
    batch.set_cameras(c2w, K); batch.set_keypoints(kp, ndiv)

    def fit_only():
        batch.set_init(betas, pose)
        batch.fit(100)
        batch.get_params()

    def frame():
        b, p = net.predict([img], np.asarray(prob["c2ws"][25])[None])
        batch.set_init(b, p)
        batch.fit(100)
        batch.get_params()
    out["fit_1x48x100_ms"] = timed(fit_only, args.reps) * 1e3
    out["hmr_plus_fit_ms"] = timed(frame, args.reps) * 1e3
    batch.close(); dev.close(); net.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
