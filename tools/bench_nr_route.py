"""A user's torch loop on the drop-in `neural_renderer.Renderer` with every tensor on cuda:0: this tree's device route, this tree's
host route (BF_TORCH_DEVICE_ROUTE=0) and the PARENT commit, which has the host route only.

    python tools/bench_nr_route.py --parent-root DIR [--reps 5] [--iters 60] [--out profiles/nr_device_route.json]
    python tools/bench_nr_route.py --child device --workload texture --iters 20      (one measurement: what a profiler is pointed at)

Workloads, all at 512 x 512 with 2 x 2 super-sampling, texture size 4, the SMPL topology (13,776 faces) and an 81,920-face scan
(tools/bench_nr_render.py's synthetic meshes):
    texture     the loop of smplify/texture_fitting.py:257-276 as written: K a numpy array in the constructor, fresh cuda R / t per
                step, two render_rgb, sum |a - b|, backward, torch.optim.Adam on the fitted textures
    silhouette  geometry_grad on: render_silhouettes of the SMPL mesh against a fixed target, backward to the vertices, Adam
    colour      geometry_grad on: a lit render_rgb of the scan against a fixed image, backward to vertices AND textures, Adam on both
Timing: a host clock around `iters` steps, ending in torch.cuda.synchronize(), behind five warm-up steps; ms per iteration.  The
route is read once per process, so every measurement is a process of its own; this process never touches the GPU.  The children
alternate device, host, parent, device, ... one at a time; the median and range per side are printed and written as JSON.  The
yardstick is the parent commit: DIR is a checkout of it with its library built (`--child parent` imports that tree)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = ("texture", "silhouette", "colour")
WARMUP = 5


def child(side, root, workload, iters, image):
    os.environ["BF_TORCH_DEVICE_ROUTE"] = "1" if side == "device" else "0"
    os.environ["BF_NR_DEVICE_ROUTE"] = "1"
    import numpy as np
    import torch                                    # (before the library: the device route needs the shared runtime)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import bodyfitting_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(bodyfitting_amd.__file__))) == os.path.realpath(root), bodyfitting_amd.__file__
    from bodyfitting_amd import native as N, neural_renderer as nr, texture_fitting as TF
    from bench_nr_render import scan_mesh, smpl_mesh

    dev = torch.device("cuda:0")
    ts, n = 4, image
    scan, fit = scan_mesh(6, ts), smpl_mesh(ts)
    assert len(scan[1]) == 81920 and len(fit[1]) == 13776
    center, dist = TF.scene_bound(scan[0])
    ring = TF.gen_cam_views(center, 18, dist, gl=True)
    K = np.array([[[n, 0, n // 2], [0, n, n // 2], [0, 0, 1]]], np.float32)
    to = lambda x: torch.from_numpy(np.array(x)).to(dev)[None]         # noqa: E731
    stats = lambda: dict(N.dev_route_stats(), **(N.nr_route_stats() if hasattr(N, "nr_route_stats") else {}))      # noqa: E731

    def camera(i):
        pose = ring[i % 18]
        return torch.cuda.FloatTensor(pose[:3, :3].reshape([1, 3, 3])), torch.cuda.FloatTensor(pose[:3, 3].reshape([1, 1, 3]))

    if workload == "texture":
        r = nr.Renderer(image_size=n, fill_back=False, camera_mode='projection', orig_size=n, light_intensity_ambient=1.0,
                        light_intensity_directional=0, near=0, far=2 * dist, background_color=[1, 1, 1], K=K)
        scan_v, scan_f, scan_t = to(scan[0]), to(scan[1]), to(scan[2])
        smpl_v, smpl_f, smpl_t = to(fit[0]), to(fit[1]), to(fit[2])
        smpl_t.requires_grad = True
        optimizer = torch.optim.Adam([smpl_t], lr=1e-2)

        def step(i):
            R, t = camera(i)
            scan_img = r.render_rgb(scan_v, scan_f, scan_t, R=R, t=t)
            smpl_img = r.render_rgb(smpl_v, smpl_f, smpl_t, R=R, t=t)
            loss = torch.sum(torch.abs(scan_img - smpl_img))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            return loss
    else:
        colour = workload == "colour"
        mesh = scan if colour else fit
        r = nr.Renderer(image_size=n, K=K, orig_size=n, near=0, far=2 * dist, background_color=[1, 1, 1])
        r.geometry_grad = True
        R0, t0 = camera(3)
        v0, faces, tex0 = to(mesh[0]), to(mesh[1]), to(mesh[2])
        with torch.no_grad():
            moved = v0 + torch.tensor([0.02, -0.01, 0.0], device=dev)
            target = r.render_rgb(moved, faces, tex0, R=R0, t=t0) if colour else r.render_silhouettes(moved, faces, R=R0, t=t0)
        vv = v0.clone().requires_grad_(True)
        tex = tex0.clone().requires_grad_(True)
        optimizer = torch.optim.Adam([vv, tex] if colour else [vv], lr=1e-3)

        def step(i):
            img = r.render_rgb(vv, faces, tex, R=R0, t=t0) if colour else r.render_silhouettes(vv, faces, R=R0, t=t0)
            loss = ((img - target) ** 2).sum()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            return loss

    for i in range(WARMUP):
        step(i)
    torch.cuda.synchronize()
    s0 = stats()
    t0_ = time.perf_counter()
    for i in range(iters):
        loss = step(WARMUP + i)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0_) / iters
    s1 = stats()
    calls = {k: (s1[k] - s0[k]) / iters for k in s1}
    if side == "device":
        assert calls["host_calls"] == 0 and calls["dev_calls"] > 0, calls
    elif "dev_calls" in calls:
        assert calls["dev_calls"] == 0, calls
    print(json.dumps({"side": side, "workload": workload, "iters": iters, "image": n, "ms_per_iteration": ms, "loss_last": float(loss.detach()),
                      "calls_per_iteration": calls}))
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", choices=("device", "host", "parent"))
    ap.add_argument("--workload", choices=WORKLOADS, default="texture")
    ap.add_argument("--workloads", nargs="+", choices=WORKLOADS, default=list(WORKLOADS))
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5, help="measurements per side and workload, each a process of its own")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child == "parent" and not a.parent_root:
            ap.error("--child parent needs --parent-root")
        return child(a.child, os.path.abspath(a.parent_root) if a.child == "parent" else REPO, a.workload, a.iters, a.image)
    sides = ("device", "host") + (("parent",) if a.parent_root else ())
    runs = []
    for workload in a.workloads:
        for rep in range(a.reps):
            for side in sides:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--workload", workload, "--iters", str(a.iters), "--image", str(a.image)]
                if a.parent_root:
                    cmd += ["--parent-root", os.path.abspath(a.parent_root)]
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                if done.returncode != 0:            # (a child that failed ends the run: nothing more is started on the card)
                    sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                    return done.returncode
                runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
                print(f"{workload:10s} rep {rep} {side:6s}: {runs[-1]['ms_per_iteration']:.3f} ms per iteration", flush=True)
    summary = []
    for workload in a.workloads:
        row = {"workload": workload}
        for side in sides:
            t = [r["ms_per_iteration"] for r in runs if r["workload"] == workload and r["side"] == side]
            row[side] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "n": len(t)}
        yard = "parent" if a.parent_root else "host"
        row["yardstick"] = yard
        row["yardstick_minus_device_ms"] = row[yard]["median_ms"] - row["device"]["median_ms"]
        row["larger_range_ms"] = max(row[s]["max_ms"] - row[s]["min_ms"] for s in (yard, "device"))
        row["device_faster_beyond_both_ranges"] = row["yardstick_minus_device_ms"] > row["larger_range_ms"]
        if a.parent_root:
            row["host_minus_parent_ms"] = row["host"]["median_ms"] - row["parent"]["median_ms"]
            row["host_reproduces_parent"] = abs(row["host_minus_parent_ms"]) <= row["parent"]["max_ms"] - row["parent"]["min_ms"]
        summary.append(row)
    print(json.dumps({"summary": summary}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"iters": a.iters, "image": a.image, "summary": summary, "runs": runs}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
