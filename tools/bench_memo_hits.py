"""The host cost of the torch drop-ins' memo hits (bodyfitting_amd/_memo.py and its users): what every optimisation step pays to
be told "seen before".  CPU tensors, the native objects stood in: no GPU and no library are needed.

    python tools/bench_memo_hits.py --parent-root DIR [--reps 5] [--out profiles/tensor_memo.json]
    python tools/bench_memo_hits.py --child ROOT              (one repeat of the tree at ROOT: what the line above starts)

Five hit paths: `_cameras_for` and `_views_for` at 8 and 48 views (keypoints as tensors and as arrays), `topology_for` with tensor and
with array faces (1,376 faces), `_silhouette_for` with extract_countours' own hand-outs, and the renderer's `_meshes_for` with
unchanged tensors.  A repeat is a process of its own that times every row with timeit, best of three; the repeats alternate DIR - a
checkout of the parent commit - and this tree.  The condition per row: this tree's median over the repeats is no greater than the
parent's maximum."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import timeit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FACES = 1376


def child(root):
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import bodyfitting_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(bodyfitting_amd.__file__))) == os.path.realpath(root), bodyfitting_amd.__file__
    from bodyfitting_amd import loss as L, native, neural_renderer as nr, normals

    class Topology:
        dev_route_device = None

        def __init__(self, n_verts, faces, device=0):
            self.n_verts, self.device = n_verts, device

    class Silhouette:
        dev_route_device = None

        def __init__(self, masks, contours=None, device=0, contour_select=0):
            self.n_views, self.device = len(masks), device
            square = np.array([[1, 1], [1, 6], [6, 6], [6, 1]], np.float32)
            self._contours = [square] * self.n_views if contours is None else contours

        def contours(self):
            return self._contours

        def close(self):
            pass

    class NrMesh:
        def __init__(self, renderer, vertices, faces, texture_size):
            pass

        def set_textures(self, textures):
            pass

        def close(self):
            pass

    native.Topology, native.Silhouette, native.NrMesh = Topology, Silhouette, NrMesh
    rng = np.random.default_rng(0)
    rows = {}

    def row(name, call, number):
        call()                                              # the miss that builds the entry
        before = dict(L.VIEW_STATS), dict(L.CAMERA_STATS)
        rows[name] = min(timeit.repeat(call, number=number, repeat=3)) / number * 1e6
        assert (dict(L.VIEW_STATS), dict(L.CAMERA_STATS)) == before, f"{name}: the timed calls were not hits"

    for views in (8, 48):
        w2cs = [torch.tensor(rng.normal(size=(4, 4)).astype(np.float32)) for _ in range(views)]
        Ks = [torch.tensor(rng.normal(size=(3, 3)).astype(np.float32)) for _ in range(views)]
        cpu = torch.device("cpu")
        row(f"_cameras_for, {views} views", lambda: L._cameras_for("bench", (w2cs, Ks), views, cpu), 2000)
        for kind in ("tensor", "array"):
            pose = [rng.normal(size=(25, 3)).astype(np.float32) for _ in range(views)]
            keypoints = [{"pose": torch.tensor(p) if kind == "tensor" else p} for p in pose]
            row(f"_views_for, {views} views, {kind} keypoints", lambda: L._views_for(w2cs, Ks, keypoints, views, False, L.SKELETON_LENGTH), 500)
    faces = rng.integers(0, 690, (N_FACES, 3))
    faces_t = torch.tensor(faces)
    row("topology_for, tensor faces", lambda: normals.topology_for("bench", faces_t, 690, 0), 20000)
    row("topology_for, array faces", lambda: normals.topology_for("bench", faces, 690, 0), 5000)
    masks = torch.zeros((4, 8, 8))
    masks[:, 1:7, 1:7] = 1
    contours = L.extract_countours(masks)
    made = []
    real = native.Silhouette
    native.Silhouette = lambda *a, **k: (made.append(1), real(*a, **k))[1]
    row("_silhouette_for, extract_countours' hand-outs", lambda: L._silhouette_for("bench", masks, contours, 0), 20000)
    assert not made, "_silhouette_for built an object"
    r = nr.Renderer()
    v, f = torch.zeros((1, 690, 3)), faces_t[None]
    tex = torch.zeros((1, N_FACES, 2, 2, 2, 3))
    sent = []
    row("Renderer._meshes_for, unchanged tensors",
        lambda: r._meshes_for(None, 0, v, f, lambda: v.numpy(), lambda: f.numpy(), tex, lambda: (sent.append(1), tex.numpy())[1]), 20000)
    assert len(sent) == 1, "the textures went up again"
    print(json.dumps({"root": root, "us_per_call": rows}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", default=None, help="the tree to time, once")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a repeat may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.child))
    if not a.parent_root or not os.path.isdir(os.path.join(a.parent_root, "bodyfitting_amd")):
        ap.error("--parent-root DIR: a checkout of the parent commit")
    sides = {"parent": os.path.abspath(a.parent_root), "tree": REPO}
    runs = {side: [] for side in sides}
    for rep in range(a.reps):
        for side, root in sides.items():
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], capture_output=True, text=True, timeout=a.timeout)
            if done.returncode != 0:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                return done.returncode
            runs[side].append(json.loads(done.stdout.strip().splitlines()[-1])["us_per_call"])
    summary, ok = [], True
    print(f"{'hit path':58s} {'parent: median (min - max)':>30s} {'this tree: median (min - max)':>32s}")
    for name in runs["tree"][0]:
        row = {"row": name}
        for side in sides:
            t = [r[name] for r in runs[side]]
            row[side] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
        row["holds"] = row["tree"]["median_us"] <= row["parent"]["max_us"]
        ok &= row["holds"]
        summary.append(row)
        cell = lambda s: f"{row[s]['median_us']:8.2f} ({row[s]['min_us']:.2f} - {row[s]['max_us']:.2f})"          # noqa: E731
        print(f"{name:58s} {cell('parent'):>30s} {cell('tree'):>32s}  {'ok' if row['holds'] else 'SLOWER'}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"reps": a.reps, "summary": summary, "runs": runs}, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
