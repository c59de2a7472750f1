"""The keypoint stage of a user's torch loop (smplify.py:177-213) with everything on cuda:0, device route against host route.

    python tools/bench_torch_route.py [--reps 5] [--iters 100] [--views 48] [--out profiles/torch_device_route.json]
    python tools/bench_torch_route.py --child device --batch 1          (one measurement: what the parent starts)

Workload: the full 6890-vertex SMPL, 48 views, 100 Adam iterations of [SMPL.forward, multiview_keypoint_loss, backward, step] -
config 2's shape - at one model evaluation per step, and at 64 (one model call on 64 parameter sets; the keypoint loss, whose batch
is 1 as the reference's, reads row 0, and a torch sum over all 64 rows' joints sends a cotangent through every row).
Timing: a host clock around the loop, ending in torch.cuda.synchronize(), after a warm-up loop of the same shapes.
The route is read once per process (BF_TORCH_DEVICE_ROUTE), so every measurement is a child process of its own; this process never
touches the GPU.  The children alternate device, host, device, ... one at a time; medians and min-max per (route, batch) are printed
and written as JSON.  The yardstick is the host route of the same build.

    python tools/bench_torch_route.py --stage smpld [--reps 5] [--iters 100] [--out profiles/torch_device_route_smpld.json]

The SMPL+D stage instead (smplify.py:229-245 as written): compute_normal_torch, point_cloud_loss_mesh_grid, normal_loss_mesh_grid,
normal_laplacian_smoothness, backward, Adam on the displacement - the full SMPL-X topology (10,475 vertices, 20,908 faces) against
config 5's synthetic scan (83,784 triangles), all tensors on cuda:0, 100 iterations behind one warm-up step per process.
`--child ROUTE --stage smpld --iters K` is one such process: what a profiler is pointed at.

    python tools/bench_torch_route.py --stage mask --parent-root DIR [--reps 5] [--iters 100] [--out profiles/torch_device_route_mask.json]

The keypoint stage with the silhouette term (smplify.py:177-213 with use_mask=True): the 6,890-vertex SMPL, 8 views with their
keypoints, 8 masks of 512 x 512 and their contours (extract_countours, once), parameters, cameras and masks on cuda:0; a step is
[SMPL.forward, the similarity, multiview_keypoint_loss, multview_mask_loss, loss = body + 5 * mask, backward, Adam].  The yardstick
is the PARENT commit, never this tree's own host route: DIR is a checkout of it with its library built, and the children alternate
this tree, the parent, this tree, ... (`--child device` / `--child parent`)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(route, batch, iters, views, loops):
    os.environ["BF_TORCH_DEVICE_ROUTE"] = "1" if route == "device" else "0"
    import numpy as np
    import torch                                    # (before the library: the device route needs the shared runtime)
    sys.path.insert(0, REPO)
    from bodyfitting_amd import _autograd, assets, loss as L, native as N, synthetic as S
    from bodyfitting_amd.prior import MaxMixturePrior
    from bodyfitting_amd.smpl import SMPL

    model, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    assets.register_gmm(gmm)
    assets.register_model(model, "smpl", "neutral")
    body, prior = SMPL(gender="neutral"), MaxMixturePrior()
    prob = S.make_problem(model, frame=0, n_views=views)
    w2c = torch.tensor(np.stack([np.linalg.inv(np.asarray(c, np.float64)) for c in prob["c2ws"]]).astype(np.float32))
    K = np.asarray(prob["Ks"], np.float32)
    use = list(range(views))
    rng = np.random.default_rng(0)
    init = (np.zeros((batch, 10), np.float32), np.tile(np.asarray(prob["init_pose"], np.float32).reshape(1, 72)[:, :3], (batch, 1)),
            np.tile(np.asarray(prob["init_pose"], np.float32).reshape(1, 72)[:, 3:], (batch, 1)))
    init = tuple(a + rng.normal(0, 0.01, a.shape).astype(np.float32) for a in init)

    def loop():
        x = [torch.tensor(a, device="cuda:0", requires_grad=True) for a in init]
        opt = torch.optim.Adam(x, lr=1e-2)
        for _ in range(iters):
            opt.zero_grad()
            out = body(betas=x[0], global_orient=x[1], body_pose=x[2])
            total, _ = L.multiview_keypoint_loss(w2c, K, prob["keypoints"], out.joints[:1] * 0.3, x[2][:1], x[0][:1], use, prior)
            if batch > 1:
                total = total + 1e-3 * out.joints.square().sum()
            total.backward()
            opt.step()
        torch.cuda.synchronize()
        return float(total)

    probe = [torch.zeros(3, device="cuda:0")]
    took = _autograd.chosen_route(probe, type("Offer", (), {"device": 0})())
    assert took == route, f"asked for the {route} route, the process takes the {took} route"
    loop()                                          # warm-up: the same shapes
    times, stats0 = [], N.dev_route_stats()
    for _ in range(loops):
        t0 = time.perf_counter()
        last = loop()
        times.append(time.perf_counter() - t0)
    stats1 = N.dev_route_stats()
    print(json.dumps({"route": route, "batch": batch, "iters": iters, "views": views, "seconds": times, "final_loss": last,
                      "calls": {k: stats1[k] - stats0[k] for k in stats1}}))


def child_smpld(route, iters, loops):
    os.environ["BF_TORCH_DEVICE_ROUTE"] = "1" if route == "device" else "0"
    import numpy as np
    import torch                                    # (before the library: the device route needs the shared runtime)
    sys.path.insert(0, REPO)
    from bodyfitting_amd import _autograd, native as N, synthetic as S
    from bodyfitting_amd.loss import normal_laplacian_smoothness, normal_loss_mesh_grid, point_cloud_loss_mesh_grid
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    from bodyfitting_amd.normals import compute_normal_torch

    device = torch.device("cuda:0")
    model = S.make_model("smplx", seed=0)
    _, scan_verts, scan_faces = S.make_scan_problem_smplx(model, 0, n_views=4, subdivide=1)
    faces = np.asarray(model["faces"], np.int64).reshape(-1, 3)
    nv = int(np.asarray(model["v_template"]).shape[0])
    assert nv == 10475 and len(scan_faces) == 83784, (nv, len(scan_faces))
    # the fitted body the stage starts from: the scan's own first 10,475 vertices (the posed body the scan was subdivided from, with
    # the scan's noise) moved off the surface by a smooth centimetre
    rng = np.random.default_rng(3)
    body = scan_verts[:nv] + 0.01 * np.sin(7.0 * scan_verts[:nv, ::-1]) + rng.normal(0, 0.002, (nv, 3))
    tris = scan_verts[scan_faces]
    face_norms = torch.from_numpy(np.cross(tris[::, 1] - tris[::, 0], tris[::, 2] - tris[::, 0])).float().to(device)
    constant_scale = float((scan_verts.max(0) - scan_verts.min(0))[1] / 1.7)
    pointsearcher = MeshGridSearcher(verts=scan_verts, faces=scan_faces)
    body_vertices = torch.from_numpy(body.astype(np.float32)).reshape(1, -1, 3).to(device)
    smpl_faces = torch.from_numpy(faces).long().to(device)

    def loop(n):
        disp = torch.zeros_like(body_vertices)
        disp.requires_grad = True
        optimizer = torch.optim.Adam([disp], lr=5e-2, betas=(0.9, 0.999))
        for _ in range(n):
            deformed_verts = body_vertices + disp
            deformed_norms = compute_normal_torch(deformed_verts, smpl_faces)
            icp_loss = point_cloud_loss_mesh_grid(pointsearcher, deformed_verts)
            norm_loss = normal_loss_mesh_grid(pointsearcher, deformed_verts, face_norms, deformed_norms)
            smoothness = normal_laplacian_smoothness(deformed_norms, smpl_faces)
            loss = icp_loss + (norm_loss + smoothness) * constant_scale * 0.1
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        torch.cuda.synchronize()
        return float(loss.detach())

    took = _autograd.chosen_route([body_vertices], type("Offer", (), {"device": 0})())
    assert took == route, f"asked for the {route} route, the process takes the {took} route"
    first = loop(1)                                 # warm-up: one step of the same shapes
    times, stats0 = [], N.dev_route_stats()
    for _ in range(loops):
        t0 = time.perf_counter()
        last = loop(iters)
        times.append(time.perf_counter() - t0)
    stats1 = N.dev_route_stats()
    print(json.dumps({"route": route, "batch": 1, "stage": "smpld", "iters": iters, "seconds": times, "first_loss": first, "final_loss": last,
                      "calls": {k: stats1[k] - stats0[k] for k in stats1}}))
    pointsearcher.close()


def child_mask(side, root, iters, loops):
    """one process of --stage mask: `side` "device" = this tree on the device route, "parent" = the tree at `root` as it routes"""
    if side == "device":
        os.environ["BF_TORCH_DEVICE_ROUTE"] = "1"
    import numpy as np
    import torch                                    # (before the library: the device route needs the shared runtime)
    sys.path.insert(0, root)
    import bodyfitting_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(bodyfitting_amd.__file__))) == os.path.realpath(root), bodyfitting_amd.__file__
    from bodyfitting_amd import assets, native as N, synthetic as S
    from bodyfitting_amd.loss import extract_countours, multiview_keypoint_loss, multview_mask_loss
    from bodyfitting_amd.prior import MaxMixturePrior
    from bodyfitting_amd.smpl import SMPL

    device = torch.device("cuda:0")
    views = 8
    model, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    assets.register_gmm(gmm)
    assets.register_model(model, "smpl", "neutral")
    body, prior = SMPL(gender="neutral"), MaxMixturePrior()
    prob = S.make_problem(model, frame=0, n_views=views, mask_frames=list(range(views)))
    w2cs = torch.inverse(torch.tensor(np.asarray(prob["c2ws"], np.float32))).to(device)           # smplify.py:131-135
    Ks = torch.tensor(np.asarray(prob["Ks"], np.float32)).to(device)
    masks = torch.tensor((np.array(prob["masks"]) > 128).astype(np.float32)).to(device)            # smplify.py:139
    assert tuple(masks.shape) == (views, 512, 512) and int(np.asarray(model["v_template"]).shape[0]) == 6890
    mask_ids = [prob["use_frames"].index(f) for f in prob["mask_frames"]]
    mask_w2cs, mask_Ks = w2cs[mask_ids], Ks[mask_ids]
    contours = extract_countours(masks)                                                            # smplify.py:144
    constant_scale = prob.get("constant_scale", 0.3)
    faces = np.asarray(model["faces"], np.int64)[None]
    pose0 = np.asarray(prob["init_pose"], np.float32).reshape(1, 72)
    init = (np.zeros((1, 3), np.float32), np.ones((1, 1), np.float32), pose0[:, 3:], np.asarray(prob["init_betas"], np.float32).reshape(1, -1),
            pose0[:, :3])

    def loop(n):
        x = [torch.tensor(a, device=device, requires_grad=True) for a in init]
        global_transl, body_scale, body_pose, betas, global_orient = x
        optimizer = torch.optim.Adam(x, lr=1e-2, betas=(0.9, 0.999))
        for _ in range(n):
            smpl_output = body(betas=betas, global_orient=global_orient, body_pose=body_pose)
            model_joints = (smpl_output.joints + global_transl) * body_scale * constant_scale
            body_vertices = (smpl_output.vertices + global_transl) * body_scale * constant_scale
            body_loss, _ = multiview_keypoint_loss(w2cs, Ks, prob["keypoints"], model_joints, body_pose, betas, prob["use_frames"], prior,
                                                   imsize=prob["imsize"])
            mask_loss = multview_mask_loss(contours, masks, body_vertices, faces, mask_w2cs, mask_Ks, prob["mask_frames"], imsize=prob["imsize"])
            loss = body_loss + 5 * mask_loss
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        torch.cuda.synchronize()
        return float(loss.detach())

    first = loop(1)                                 # warm-up: one step of the same shapes
    times, stats0 = [], N.dev_route_stats()
    for _ in range(loops):
        t0 = time.perf_counter()
        last = loop(iters)
        times.append(time.perf_counter() - t0)
    stats1 = N.dev_route_stats()
    print(json.dumps({"route": side, "batch": 1, "stage": "mask", "iters": iters, "seconds": times, "first_loss": first, "final_loss": last,
                      "contour_points": [int(len(c)) for c in contours], "calls": {k: stats1[k] - stats0[k] for k in stats1}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", choices=("device", "host", "parent"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5, help="measurements per (route, batch), each a process of its own")
    ap.add_argument("--loops", type=int, default=1, help="timed loops per process, behind its warm-up loop")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stage", choices=("keypoint", "smpld", "mask"), default="keypoint",
                    help="smpld: the SMPL+D loop (one evaluation per step); mask: the keypoint stage with the silhouette term, against --parent-root")
    ap.add_argument("--parent-root", default=None, help="--stage mask: a checkout of the parent commit with its library built")
    a = ap.parse_args()
    if a.stage == "mask":
        if a.child:
            return child_mask(a.child, a.parent_root if a.child == "parent" else REPO, a.iters, a.loops)
        if not a.parent_root or not os.path.isdir(os.path.join(a.parent_root, "bodyfitting_amd")):
            ap.error("--stage mask measures against the parent commit: --parent-root DIR (a checkout of it, built)")
        a.batches = [1]
    sides = ("device", "parent") if a.stage == "mask" else ("device", "host")
    if a.child:
        return child_smpld(a.child, a.iters, a.loops) if a.stage == "smpld" else child(a.child, a.batch, a.iters, a.views, a.loops)
    if a.stage == "smpld":
        a.batches = [1]
    runs = []
    for batch in a.batches:
        for rep in range(a.reps):
            for route in sides:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--batch", str(batch), "--iters", str(a.iters),
                       "--views", str(a.views), "--loops", str(a.loops), "--stage", a.stage]
                if a.parent_root:
                    cmd += ["--parent-root", os.path.abspath(a.parent_root)]
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                if done.returncode != 0:            # (a child that failed ends the run: nothing more is started on the card)
                    sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                    return done.returncode
                runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
                print(f"batch {batch:3d} rep {rep} {route:6s}: " + " ".join(f"{t * 1e3:.1f}" for t in runs[-1]["seconds"]) + " ms", flush=True)
    summary = []
    for batch in a.batches:
        row = {"batch": batch}
        for route in sides:
            t = [s for r in runs if r["batch"] == batch and r["route"] == route for s in r["seconds"]]
            row[route] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "n": len(t)}
        spread = max(row[r]["max_ms"] - row[r]["min_ms"] for r in sides)
        row[f"{sides[1]}_minus_device_ms"] = row[sides[1]]["median_ms"] - row["device"]["median_ms"]
        row["larger_spread_ms"] = spread
        row["device_faster_beyond_spread"] = row[f"{sides[1]}_minus_device_ms"] > spread
        summary.append(row)
    result = {"stage": a.stage, "iters": a.iters, "views": a.views, "summary": summary, "runs": runs}
    print(json.dumps({"summary": summary}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
