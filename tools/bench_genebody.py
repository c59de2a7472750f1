"""GeneBody view preparation and one whole runner frame on the GPU, on a seeded synthetic 48-view capture of 2448 x 2048 views (no dataset
needed).  Record: profiles/genebody_bench.md.

Reports, per frame of 48 views at load size 512:
  - ViewPrep (bbox + prepare) wall time, synchronised, and its device-timed parts from HIP events: mask upload, bbox kernels, crop
    upload, prepare kernel, download;
  - the bytes moved and the upload's share of the host-link bound (PCIe Gen5 x16, 63 GB/s); the host buffers are pageable numpy arrays;
  - the bbox kernel's mask bytes per second against HBM;
  - the numpy restatement (tests' checker, image_cropping + cv2_resize_linear) on one core for 8 views, scaled to 48 - cv2 is absent,
    so this is numpy, not OpenCV;
  - with --runner, one whole runner frame (decode, prepare, PNG writes, OpenPose, HMR, fit, files) with synthetic weights and model,
    the second of two frames (the first pays for weight uploads and allocations).

Usage:  python tools/bench_genebody.py [--reps 10] [--runner] [--out results.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
H, W, N, L = 2048, 2448, 48, 512
LINK_GBS, HBM_GBS = 63.0, 8000.0


def capture(seed=0, frames=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    imgs, msks = [], []
    for v in range(N):
        cy, cx = H / 2 + rng.uniform(-200, 200), W / 2 + rng.uniform(-500, 500)
        m = (((yy - cy) / 800) ** 2 + ((xx - cx) / 250) ** 2 < 1).astype(np.uint8) * 255
        ph = 0.37 * v
        img = np.stack([128 + 100 * np.sin(xx / 37 + ph), 128 + 90 * np.cos(yy / 23 - ph), 128 + 80 * np.sin((xx + yy) / 51)], -1)
        imgs.append(img.astype(np.uint8))
        msks.append(m)
    return imgs, msks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runner", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from bodyfitting_amd import genebody as GB
    imgs, msks = capture()
    cams = {"K": np.tile(np.array([[1500, 0, W / 2], [0, 1500, H / 2], [0, 0, 1]], np.float32), (N, 1, 1)),
            "RT": np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))}
    views = list(range(N))
    prep = GB.ViewPrep(device=0, L=L, max_views=N, max_h=H, max_w=W)
    GB.prepare_frame(imgs, msks, cams, views, GB.MASK_FRAMES, True, L, prep=prep)       # warm: allocations, code objects
    walls, parts = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        GB.prepare_frame(imgs, msks, cams, views, GB.MASK_FRAMES, True, L, prep=prep)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms, by = prep.last_timing()
        parts.append(ms)
    ms = np.median(np.stack(parts), 0)
    up_bytes = int(by[0] + by[1])
    res = {
        "views": N, "view_hw": [H, W], "load_size": L, "reps": args.reps, "host_buffers": "pageable",
        "prepare_frame_wall_ms_median": float(np.median(walls)), "prepare_frame_wall_ms_min": float(np.min(walls)),
        "device_ms": {"mask_upload": float(ms[0]), "bbox_kernels": float(ms[1]), "bbox_download": float(ms[2]),
                      "crop_upload": float(ms[3]), "prepare_kernel": float(ms[4]), "download": float(ms[5])},
        "bytes": {"masks_up": int(by[0]), "crops_up": int(by[1]), "down": int(by[2])},
    }
    up_ms = float(ms[0] + ms[3])
    res["upload_GBs"] = up_bytes / up_ms / 1e6
    res["upload_share_of_link_bound"] = res["upload_GBs"] / LINK_GBS
    res["link_bound_ms_all_bytes"] = (up_bytes + int(by[2])) / LINK_GBS / 1e6
    res["bbox_kernel_GBs"] = int(by[0]) / float(ms[1]) / 1e6
    res["bbox_share_of_hbm"] = res["bbox_kernel_GBs"] / HBM_GBS
    import genebody_cases as G
    t0 = time.perf_counter()
    G.prepare_frame_numpy(imgs[:8], msks[:8], {"K": cams["K"][:8], "RT": cams["RT"][:8]}, views[:8], GB.MASK_FRAMES, True, L)
    res["numpy_one_core_ms_8_views"] = (time.perf_counter() - t0) * 1e3
    res["numpy_one_core_ms_48_views_scaled"] = res["numpy_one_core_ms_8_views"] * 6
    prep.close()
    if args.runner:
        res["runner"] = runner_frame(imgs, msks, cams)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def runner_frame(imgs, msks, cams):
    """two frames through python -m bodyfitting_amd.genebody's runner, synthetic weights; the second frame's stage times"""
    from PIL import Image
    from bodyfitting_amd import assets, genebody as GB, synthetic as S
    from concurrent.futures import ThreadPoolExecutor
    assets.register_model(S.make_model("smpl", seed=0), "smpl", "neutral")
    assets.register_gmm(S.make_gmm(seed=0))
    sd, mean = S.make_hmr_weights(0)
    assets.register_hmr(sd, mean)
    assets.register_openpose(S.make_openpose_weights(0))
    tmp = tempfile.mkdtemp(prefix="genebody_bench_")
    root = os.path.join(tmp, "capture")
    np.save(os.path.join(root + "_annots.npy"), {"cams": cams}, allow_pickle=True)
    os.makedirs(root, exist_ok=True)
    os.replace(root + "_annots.npy", os.path.join(root, "annots.npy"))

    def write(job):
        kind, v, f = job
        d = os.path.join(root, "bench", kind, "%02d" % v)
        os.makedirs(d, exist_ok=True)
        if kind == "image":
            Image.fromarray(imgs[v]).save(os.path.join(d, "%04d.jpg" % f), quality=95)
        else:
            Image.fromarray(msks[v]).save(os.path.join(d, "%04d.png" % f))

    with ThreadPoolExecutor(GB.io_threads()) as ex:
        list(ex.map(write, [(k, v, f) for k in ("image", "mask") for v in range(N) for f in range(2)]))
    a = GB.config_parser().parse_args(["--target_dir", root, "--output_dir", os.path.join(tmp, "out"), "--subject", "bench"])
    a.num_iters = 600
    r = GB.runner(a)
    out = {}
    for frame in (0, 1):
        t = {}
        t0 = time.perf_counter()
        data = r.get_data(frame)
        t["get_data_ms"] = (time.perf_counter() - t0) * 1e3
        t1 = time.perf_counter()
        r.run_openpose(frame, data)
        t["openpose_ms"] = (time.perf_counter() - t1) * 1e3
        t1 = time.perf_counter()
        kp = r.read_openpose(frame)
        r.run_smplify(frame, data, kp)
        t["read_json_hmr_fit_files_ms"] = (time.perf_counter() - t1) * 1e3
        t1 = time.perf_counter()
        r.run_output(frame)
        t["output_ms"] = (time.perf_counter() - t1) * 1e3
        t["frame_ms"] = (time.perf_counter() - t0) * 1e3
        t["views_kept"] = len(data[4])
        out[f"frame{frame}"] = t
    r.close()
    return out


if __name__ == "__main__":
    main()
