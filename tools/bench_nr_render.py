"""Wall time per iteration of the torch loop of smplify/texture_fitting.py:262-270 on the drop-in `neural_renderer` (two renders,
sum |scan_img - smpl_img|, loss.backward(), torch.optim.Adam on host tensors) next to the fused `bf_texfit_step` on the same
meshes and views: render 512 x 512 with 2 x 2 super-sampling, texture size 4, the SMPL topology (13,776 faces) and an 81,920-face
scan.  Synthetic meshes.  Also the parts of one drop-in iteration (host clock around each call).  Device time of the kernels:
run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_nr_render.py --iters 20` and read bf_nr_* / bf_tex_*.
A record, not a gate: profiles/nr_render_bench.md."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bodyfitting_amd import neural_renderer as nr      # noqa: E402
from bodyfitting_amd import texture_fitting as TF      # noqa: E402
from texfit_cases import icosphere                     # noqa: E402


def scan_mesh(level, ts):
    rng = np.random.default_rng(0)
    v, f = icosphere(level)
    v = (v * np.array([0.45, 0.8, 0.4], np.float32) * (1 + 0.05 * np.sin(9 * v[:, 1:2])) + np.array([0, 0.9, 0], np.float32)).astype(np.float32)
    return v, f, rng.uniform(0, 1, (len(f), ts, ts, ts, 3)).astype(np.float32)


def smpl_mesh(ts):
    d = np.load(ROOT / "bodyfitting_amd" / "data" / "template_smpl_6890.npz")
    v = d["verts"].astype(np.float32)
    v = (v - (v.max(0) + v.min(0)) / 2 + np.array([0, 0.9, 0], np.float32)).astype(np.float32)
    f = d["faces"].astype(np.int32)
    return v, f, np.full((len(f), ts, ts, ts, 3), 0.5, np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--scan-level", type=int, default=6)      # 81,920 faces
    a = ap.parse_args()
    ts = 4
    scan, fit = scan_mesh(a.scan_level, ts), smpl_mesh(ts)
    center, dist = TF.scene_bound(scan[0])
    ring = TF.gen_cam_views(center, 18, dist, gl=True)
    n = a.image
    K = np.array([[[n, 0, n // 2], [0, n, n // 2], [0, 0, 1]]], np.float32)

    fused = TF.Renderer(n, ts, near=0.0, far=2 * dist)
    fused.set_mesh(fused.TARGET, scan); fused.set_mesh(fused.FITTED, fit)
    for i in range(5):
        fused.step(ring[i], 1e-2)
    t0 = time.perf_counter()
    for i in range(a.iters):
        fused.step(ring[i % 18], 1e-2)
    fused_ms = 1e3 * (time.perf_counter() - t0) / a.iters
    fused.close()

    r = nr.Renderer(image_size=n, K=K, orig_size=n, near=0.0, far=2 * dist, background_color=[1, 1, 1], fill_back=False,
                    light_intensity_ambient=1.0, light_intensity_directional=0.0)
    to = lambda x: torch.from_numpy(np.array(x))[None]         # noqa: E731
    scan_v, scan_f, scan_t = to(scan[0]), to(scan[1]), to(scan[2])
    smpl_v, smpl_f = to(fit[0]), to(fit[1])
    smpl_t = to(fit[2]).requires_grad_(True)
    opt = torch.optim.Adam([smpl_t], lr=1e-2)
    parts = {k: [] for k in ("render_scan", "render_smpl", "loss", "backward", "adam")}
    total = []
    for i in range(a.iters + 5):
        pose = ring[i % 18]
        R, t = to(pose[:3, :3].astype(np.float32)), to(pose[:3, 3].astype(np.float32))[None]
        c = [time.perf_counter()]
        opt.zero_grad()
        scan_img = r.render_rgb(scan_v, scan_f, scan_t, R=R, t=t); c.append(time.perf_counter())
        smpl_img = r.render_rgb(smpl_v, smpl_f, smpl_t, R=R, t=t); c.append(time.perf_counter())
        loss = torch.sum(torch.abs(scan_img - smpl_img)); c.append(time.perf_counter())
        loss.backward(); c.append(time.perf_counter())
        opt.step(); c.append(time.perf_counter())
        if i >= 5:
            total.append(c[-1] - c[0])
            for k, d in zip(parts, np.diff(c)):
                parts[k].append(d)
    r.close()
    med = lambda x: 1e3 * float(np.median(x))                  # noqa: E731
    print(json.dumps({"metric": "nr_dropin_loop_ms_per_iteration", "value": med(total), "fused_bf_texfit_step_ms": fused_ms, "image": n,
                      "scan_faces": len(scan[1]), "fit_faces": len(fit[1]), "parts_ms": {k: med(v) for k, v in parts.items()},
                      "loss_last": float(loss.detach())}))


if __name__ == "__main__":
    main()
