#!/usr/bin/env python3
"""The user's own SMPL+D loop (smplify.py:236-245) on the drop-in functions - compute_normal_torch, point_cloud_loss_mesh_grid,
normal_loss_mesh_grid, normal_laplacian_smoothness with torch.optim.Adam - on one GPU: a record, not part of the bench.py contract.
Writes profiles/scan_losses_bench.md (or --out).  Per size (the 690-vertex model against its 1,376-face scan; the 6,890-vertex model
against its scan subdivided once, 55,104 faces - the ~83k-face scan of BASELINE config 5 is the SMPL-X body's and has no SMPL fit
beside it):
  * wall time per iteration of the drop-in loop, median of --iters iterations after --warmup, and the part of it spent inside the
    five native calls (staging, launches, the device synchronise, the copies back);
  * device time per kernel and per host <-> device copy from `rocprofv3 --kernel-trace --memory-copy-trace --stats`, in a run of its
    own: a child process started BEFORE this process touches the GPU runs the same loop under the profiler (--child);
  * next to them, torch's float32 CPU loop over oracle.mesh_oracle with the same searcher, and `fit_displacement` (the fused stage)
    per iteration.
usage: python tools/bench_scan_losses.py [--iters I] [--warmup W] [--out FILE] [--no-profile]"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bodyfitting_amd import native as N, synthetic as S   # noqa: E402

SIZES = (("nv = 690, scan 1,376 faces", 690, 0), ("nv = 6,890, scan 55,104 faces", None, 1))
NATIVE_CALLS = ("vertex_normals", "vertex_normals_vjp", "normal_laplacian", "normal_loss")


def problem(nv, subdivide):
    """-> (model, base mesh [NV,3] = the scan's own vertices 5 mm off, scan verts, scan faces)"""
    model = S.make_model("smpl", seed=0, nv=nv)
    prob, sv, sf = S.make_scan_problem(model, frame=0, n_views=8)
    base = (sv + np.random.default_rng(1).normal(0, 0.005, sv.shape)).astype(np.float32)
    if subdivide:
        sv, sf = S.subdivide_mesh(sv, sf, subdivide)
    return model, prob, base, np.ascontiguousarray(sv, np.float32), np.ascontiguousarray(sf, np.int32)


def loop(fns, searcher, base, faces, sv, sf, iters):
    """smplify.py:229-245 -> the seconds each iteration took"""
    import torch
    compute_normal_torch, point_loss, normal_loss, laplacian = fns
    tris = sv[sf]
    face_norms = torch.from_numpy(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])).float()
    constant_scale = float((sv.max(0) - sv.min(0))[1] / 1.7)
    body_vertices = torch.tensor(base).reshape(1, -1, 3)
    disp = torch.zeros_like(body_vertices)
    disp.requires_grad = True
    optimizer = torch.optim.Adam([disp], lr=5e-2, betas=(0.9, 0.999))
    smpl_faces = torch.from_numpy(np.asarray(faces)).long()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        deformed_verts = body_vertices + disp
        deformed_norms = compute_normal_torch(deformed_verts, smpl_faces)
        icp_loss = point_loss(searcher, deformed_verts)
        norm_loss = normal_loss(searcher, deformed_verts, face_norms, deformed_norms)
        smoothness = laplacian(deformed_norms, smpl_faces)
        loss = icp_loss + (norm_loss + smoothness) * constant_scale * 0.1
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        ts.append(time.perf_counter() - t0)
    return ts


def dropin_fns():
    from bodyfitting_amd import loss as L
    from bodyfitting_amd.normals import compute_normal_torch
    return compute_normal_torch, L.point_cloud_loss_mesh_grid, L.normal_loss_mesh_grid, L.normal_laplacian_smoothness


def oracle_fns():
    """torch float32 on the CPU over the oracle's formulas; the search is the searcher's, as in the reference"""
    import torch
    from oracle import mesh_oracle as MO

    def point_loss(searcher, pts):
        near, _ = searcher.nearest_points(pts.reshape(-1, 3))
        return MO.point_cloud_loss(pts, near)

    def normal_loss(searcher, pts, face_norms, norms):
        _, ids = searcher.nearest_points(pts.reshape(-1, 3))
        return MO.normal_loss(face_norms[ids.long()], norms)

    return (lambda v, f: MO.compute_normal_torch(v.reshape(-1, 3), f)), point_loss, normal_loss, MO.normal_laplacian_smoothness


def child(iters, warmup):
    """the run under the profiler: the same loop, nothing else on the device"""
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    for _, nv, sub in SIZES:
        model, _, base, sv, sf = problem(nv, sub)
        s = MeshGridSearcher(sv, sf)
        loop(dropin_fns(), s, base, model["faces"], sv, sf, warmup + iters)
        s.close()


def device_times(iters, warmup):
    """-> {"kernels": {name: total us}, "copies": total us, "iterations": n} over both sizes, or a string saying why there are none"""
    import sqlite3
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-d", d, "-o", "sl", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--iters", str(iters), "--warmup", str(warmup)]
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
        dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
        if run.returncode != 0 or not dbs:
            return f"rocprofv3 run failed ({run.returncode}): {run.stderr[-300:]}"
        con = sqlite3.connect(dbs[0])
        rows = con.execute("select name, duration from kernels").fetchall()
        try:
            copies = con.execute("select count(*), sum(duration) from memory_copies").fetchone()
        except sqlite3.Error as e:
            copies = (0, None, str(e))
    kernels = {}
    for name, dur in rows:
        k = kernels.setdefault(name.split("(")[0], [0, 0.0])
        k[0] += 1
        k[1] += dur * 1e-3
    return {"kernels": kernels, "copies": copies, "iterations": len(SIZES) * (iters + warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan_losses_bench.md"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (device times: not measured)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.iters, a.warmup)
    # the profiled run first: this process has not opened the GPU yet
    dev = "not measured (--no-profile)" if a.no_profile else device_times(min(a.iters, 20), a.warmup)
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    rows = []
    for label, nv, sub in SIZES:
        model, prob, base, sv, sf = problem(nv, sub)
        s = MeshGridSearcher(sv, sf)
        # time inside the native calls: thin wrappers around them for this measurement only
        inside = [0.0]

        def clocked(f):
            def g(*args, **kw):
                t0 = time.perf_counter()
                try:
                    return f(*args, **kw)
                finally:
                    inside[0] += time.perf_counter() - t0
            return g

        saved = {k: getattr(N, k) for k in NATIVE_CALLS}
        for k in NATIVE_CALLS:
            setattr(N, k, clocked(saved[k]))
        s._scan.point_loss = clocked(s._scan.point_loss)
        loop(dropin_fns(), s, base, model["faces"], sv, sf, a.warmup)
        inside[0] = 0.0
        ts = loop(dropin_fns(), s, base, model["faces"], sv, sf, a.iters)
        native_ms = inside[0] / a.iters * 1e3
        for k in NATIVE_CALLS:
            setattr(N, k, saved[k])
        cpu = loop(oracle_fns(), s, base, model["faces"], sv, sf, max(3, a.iters // 5))
        s.close()
        # the fused stage on the same model and scan
        dm = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
        scan = N.Scan(sv, sf)
        c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
        b = N.FrameBatch(dm, 1, 8)
        b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_scans([scan])
        b.fit(30); b.sync()
        b.fit_displacement(a.warmup); b.sync()
        t0 = time.perf_counter()
        b.fit_displacement(a.iters); b.sync()
        fused_ms = (time.perf_counter() - t0) / a.iters * 1e3
        b.close(); scan.close(); dm.close()
        row = {"size": label, "dropin_ms": round(float(np.median(ts)) * 1e3, 3), "dropin_min_ms": round(float(np.min(ts)) * 1e3, 3),
               "in_native_calls_ms": round(native_ms, 3), "torch_cpu_f32_ms": round(float(np.median(cpu)) * 1e3, 3), "fused_ms": round(fused_ms, 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(a.out, "w") as f:
        f.write("# The SMPL+D loop on the drop-in functions, one MI355X (tools/bench_scan_losses.py)\n\n")
        f.write("One iteration = smplify.py:237-245 as a user writes it: `compute_normal_torch`, `point_cloud_loss_mesh_grid`,\n"
                "`normal_loss_mesh_grid`, `normal_laplacian_smoothness`, `loss.backward()`, `torch.optim.Adam.step()` - five native calls\n"
                "(normals, point loss, normal loss, Laplacian, the normals' VJP), each through host memory.  Wall: host clock per iteration,\n"
                f"median (minimum) of {a.iters} after {a.warmup}.  torch CPU: the same loop in float32 over `oracle.mesh_oracle`, searching with the\n"
                "same searcher.  Fused: `fit_displacement` (`bf_fit_displacement`, nothing crosses PCIe inside it) per iteration.  The 6,890-vertex\n"
                "row's scan is the body's own scan subdivided once (55,104 faces), not the ~83k-face SMPL-X scan.  A record, not a gate.\n\n")
        f.write("| size | drop-in loop, ms / iteration | inside the native calls, ms | torch CPU float32, ms | fused stage, ms |\n|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['size']} | {r['dropin_ms']} ({r['dropin_min_ms']}) | {r['in_native_calls_ms']} | {r['torch_cpu_f32_ms']} | {r['fused_ms']} |\n")
        f.write("\n")
        if isinstance(dev, dict):
            n_it = dev["iterations"]
            total = sum(v[1] for v in dev["kernels"].values())
            f.write(f"Device time, both sizes together, per iteration over {n_it} profiled iterations (`rocprofv3 --kernel-trace --memory-copy-trace`):\n\n")
            f.write("| kernel | launches / iteration | device us / iteration |\n|---|---|---|\n")
            for name, (cnt, us) in sorted(dev["kernels"].items(), key=lambda kv: -kv[1][1]):
                f.write(f"| `{name}` | {cnt / n_it:.2f} | {us / n_it:.2f} |\n")
            f.write(f"| all kernels | | {total / n_it:.2f} |\n\n")
            c = dev["copies"]
            if c[1] is not None:
                f.write(f"Host <-> device copies: {c[0] / n_it:.1f} per iteration, {c[1] * 1e-3 / n_it:.2f} us of device time per iteration.\n\n")
            else:
                f.write(f"Host <-> device copies: not measured ({c[2] if len(c) > 2 else 'no records'}).\n\n")
            mean_native = float(np.mean([r["in_native_calls_ms"] for r in rows])) * 1e3
            f.write(f"The kernels account for {total / n_it:.0f} us of the {mean_native:.0f} us (mean of the sizes) an iteration spends inside the native calls: "
                    "the rest is the host round trips - staging, launches, the device synchronise and the copies back.\n")
        else:
            f.write(f"Device times: {dev}\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
