"""The seeded synthetic RenderPeople tree and stand-ins shared by tools/gen_rp_golden.py (which runs the reference's apps/rp_fitting.py
and smplify/body_fitting.py's check_smpl_fitting on them) and the tests (which rebuild them from the seed and compare).

- `write_tree(root)`: <root>/<subject>/<name>.obj scans (contents unread by the stand-ins), one nested a level deeper, and a
  `_30k.obj` decoy beside one of them;
- `fake_render`: render_texture_mesh's signature, seeded by the scan's folder and file name: 8 views of uint8 images and masks,
  float64 world-to-camera GL poses and float64 Ks;
- `people(image)`: the people a detector "finds" in an RGB view, seeded by the view's bytes (the reference's openpose.bin stand-in
  writes them for the PNG it reads, the runner's detector stand-in for the array it is given);
- `overlay_cases()`: (image, verts, c2w, K) of check_smpl_fitting with points off the image and on its edges.
"""
from __future__ import annotations

import json
import os

import numpy as np

L = 48                                          # the load size of the runner cases
VIEWS = 8
SCANS = (("alice", "alice.obj"), ("bob", "rp_bob_posed_100k.obj"), (os.path.join("batch2", "carol"), "carol.obj"))
DECOY = ("alice", "alice_30k.obj")


def write_tree(root):
    for folder, name in SCANS + (DECOY,):
        os.makedirs(os.path.join(root, folder), exist_ok=True)
        with open(os.path.join(root, folder, name), "w") as f:
            f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    return root


def _seed(file):
    name = os.path.basename(os.path.dirname(file)) + "/" + os.path.basename(file)
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def fake_render(file, imgsize=512, viewnum=8, white_bkgd=False, pose_only=False):
    """render_texture_mesh(file, imgsize, viewnum, white_bkgd, pose_only) -> (imgs, masks, poses, Ks) or (poses, Ks), seeded arrays"""
    rng = np.random.default_rng(_seed(file))
    poses, Ks = [], []
    for _ in range(viewnum):
        P = np.eye(4)
        P[:3, :3] = _rotation(rng)
        P[:3, 3] = rng.normal(0, 2, 3)
        poses.append(P)
        Ks.append(np.array([[imgsize * rng.uniform(0.9, 1.1), 0, imgsize / 2], [0, imgsize * rng.uniform(0.9, 1.1), imgsize / 2],
                            [0, 0, 1]]))
    if pose_only:
        return poses, Ks
    imgs = [rng.integers(0, 256, (imgsize, imgsize, 3), dtype=np.uint8) for _ in range(viewnum)]
    masks = [(rng.random((imgsize, imgsize)) < 0.4).astype(np.uint8) * 255 for _ in range(viewnum)]
    if white_bkgd:
        imgs = [im | (255 - m)[..., None] for im, m in zip(imgs, masks)]
    return imgs, masks, poses, Ks


def people(image):
    """0, 1 or 2 people ([25, 3] float64: x, y in the image, confidence in (0, 1]) seeded by the RGB view's bytes"""
    im = np.asarray(image)
    rng = np.random.default_rng(int(im.astype(np.int64).sum()) % (2 ** 32))
    out = []
    for _ in range(int(rng.integers(0, 3))):
        p = np.zeros((25, 3))
        p[:, 0] = np.round(rng.uniform(0, im.shape[1], 25), 3)
        p[:, 1] = np.round(rng.uniform(0, im.shape[0], 25), 3)
        p[:, 2] = np.round(rng.uniform(0.05, 1, 25), 3)
        out.append(p)
    return out


def write_people_json(path, ps):
    """openpose.bin's JSON of those people (infer_openpose.py's layout)"""
    doc = {"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": np.asarray(p).flatten().tolist()} for p in ps]}
    with open(path, "w") as f:
        json.dump(doc, f)


def overlay_cases():
    """(image, verts, c2w, K) - the runner's c2w (inv of a GL pose, float32), float32 K - plus cameras with exact-pixel and edge
    points"""
    rng = np.random.default_rng(11)
    out = []
    for k in range(4):
        H, W = (40, 56) if k % 2 else (48, 48)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        P = np.eye(4)
        P[:3, :3] = _rotation(rng)
        P[:3, 3] = rng.normal(0, 0.3, 3)
        P[2, 3] += 4.0 if k < 3 else -4.0                     # world to camera; the last one looks away (z < 0 still projects)
        c2w = np.linalg.inv(P).astype(np.float32)
        K = np.array([[W * 1.1, 0, W / 2], [0, W * 1.1, H / 2], [0, 0, 1]], np.float32)
        verts = rng.normal(0, 0.6, (400, 3)).astype(np.float32)
        out.append((img, verts, c2w, K))
    # an identity camera: vertices on exact pixels, on the edges, off by a little on each side, behind and on the camera plane
    H, W = 20, 30
    img = np.zeros((H, W, 3), np.uint8)
    K = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    pix = [(0, 0), (W - 1, H - 1), (5, 7), (-0.3, 4), (4, -0.3), (W - 0.01, 3), (3, H - 0.01), (W, 3), (3, H), (0, H - 1), (W - 1, 0)]
    verts = [(x, y, 1.0) for x, y in pix] + [(0.5, 0.5, -1.0), (-12.0, -9.0, -1.0), (0.1, 0.1, 0.0)]
    out.append((img, np.asarray(verts, np.float32), np.eye(4, dtype=np.float32), K))
    return out
