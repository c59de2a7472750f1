"""The seeded synthetic GeneBody captures and crop cases shared by tools/gen_genebody_golden.py (which runs the reference's
apps/genebody_fitting.py on them) and the tests (which rebuild them from the seed and compare).

A capture is the GeneBody layout: <root>/annots.npy ({'cams': {'K': [48, 3, 3], 'RT': [48, 4, 4]}}, float32) and
<root>/<subject>/{image,mask}/<view %02d>/<frame %04d>.png, masks from synthetic.render_mask of the synthetic SMPL template on a ring
of 48 cameras, then edited: shifted against the borders, a patch of values 1..128 (inside the box, outside `> 128`), one black view and
one dim view in frame 0.  Images are smooth RGB textures, PNG (lossless, so the decode is the same bytes everywhere).
"""
from __future__ import annotations

import os

import numpy as np

N_VIEWS = 48
H, W = 64, 96
SUBJECTS = ("zhuna", "wuwenyan")
FRAMES = 2
# (subject, frame, use_mask, load_size) of the stored get_data outputs
DATA_CASES = (("zhuna", 0, True, 40), ("zhuna", 1, False, 40), ("wuwenyan", 0, True, 56))
BLACK_VIEW, DIM_VIEW = 5, 9                 # frame 0: all zeros, all 5 (np.mean <= 10: dropped)


def view_mask(model, view, seed=0, h=H, w=W):
    """the silhouette of view `view` [h, w] uint8 with the capture's edits"""
    from bodyfitting_amd import synthetic as S
    verts = np.asarray(model["v_template"], np.float64)
    size = max(h, w)
    c2ws, Ks = S.ring_cameras(N_VIEWS, imsize=size, focal=float(size), centre=verts.mean(0).tolist())
    m = S.render_mask(verts, c2ws[view], Ks[view], imsize=size, radius=2)
    top = (size - h) // 2
    m = m[top:top + h, :w].copy()
    rng = np.random.default_rng(seed * 1000 + view)
    shift = int(rng.integers(-w // 2, w // 2 + 1))
    if view % 6 == 2:
        shift = -w                              # pushed against the left border
    elif view % 6 == 4:
        shift = w                               # ... and the right one
    ys, xs = np.nonzero(m)
    out = np.zeros_like(m)
    dx = int(np.clip(shift, -xs.min(), w - 1 - xs.max()))
    out[ys, xs + dx] = m[ys, xs]
    if view % 4 == 3:                            # a patch the box counts and `> 128` masks out
        y0, x0 = ys.min() + 2, xs.min() + dx
        out[y0:y0 + 6, max(x0 - 4, 0):x0 + 3] = rng.integers(1, 129, (6, min(x0 + 3, w) - max(x0 - 4, 0)), dtype=np.uint8)
    return out


def view_image(view, frame, seed=0, h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = 0.37 * view + 0.11 * frame + seed
    img = np.stack([128 + 100 * np.sin(xx / 7.0 + ph), 128 + 90 * np.cos(yy / 5.0 - ph), 128 + 80 * np.sin((xx + yy) / 9.0 + 2 * ph)], -1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def cameras(seed=0):
    rng = np.random.default_rng(seed + 77)
    K = np.zeros((N_VIEWS, 3, 3), np.float32)
    K[:, 0, 0] = rng.uniform(80, 120, N_VIEWS)
    K[:, 1, 1] = K[:, 0, 0] * rng.uniform(0.98, 1.02, N_VIEWS)
    K[:, 0, 2] = W / 2 + rng.uniform(-3, 3, N_VIEWS)
    K[:, 1, 2] = H / 2 + rng.uniform(-3, 3, N_VIEWS)
    K[:, 2, 2] = 1
    RT = np.tile(np.eye(4, dtype=np.float32), (N_VIEWS, 1, 1))
    RT[:, :3, 3] = rng.normal(0, 2, (N_VIEWS, 3)).astype(np.float32)
    return {"K": K, "RT": RT}


def write_capture(root, subjects=SUBJECTS, frames=FRAMES, seed=0, mask_views_only=False):
    """the capture under `root` (see the module docstring).  mask_views_only: every image black except the mask views 1, 7, ..., 43"""
    from PIL import Image
    from bodyfitting_amd import synthetic as S
    from bodyfitting_amd.genebody import MASK_FRAMES
    model = S.make_model("smpl", seed=0)
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "annots.npy"), {"cams": cameras(seed)}, allow_pickle=True)
    masks = [view_mask(model, v, seed) for v in range(N_VIEWS)]
    for subject in subjects:
        for v in range(N_VIEWS):
            for kind in ("image", "mask"):
                os.makedirs(os.path.join(root, subject, kind, "%02d" % v), exist_ok=True)
            for f in range(frames):
                img = view_image(v, f, seed)
                if (f == 0 and v == BLACK_VIEW) or (mask_views_only and v not in MASK_FRAMES):
                    img[:] = 0
                elif f == 0 and v == DIM_VIEW:
                    img[:] = 5
                Image.fromarray(img).save(os.path.join(root, subject, "image", "%02d" % v, "%04d.png" % f))
                Image.fromarray(np.roll(masks[v], f, axis=0)).save(os.path.join(root, subject, "mask", "%02d" % v, "%04d.png" % f))
    return root


def crop_masks(seed=0, n=300):
    """masks that reach every branch of image_cropping: random boxes of random values in random sizes, tall-narrow and wide-short
    images (size > w, size > h), boxes against each border, single pixels"""
    rng = np.random.default_rng(seed + 5)
    out = []
    for k in range(n):
        kind = k % 6
        if kind == 0:
            h, w = int(rng.integers(40, 80)), int(rng.integers(4, 16))          # tall and narrow: size > w
        elif kind == 1:
            h, w = int(rng.integers(4, 16)), int(rng.integers(40, 80))          # wide and short: size > h
        else:
            h, w = int(rng.integers(2, 90)), int(rng.integers(2, 90))
        m = np.zeros((h, w), np.uint8)
        if kind == 5:
            m[rng.integers(0, h), rng.integers(0, w)] = rng.integers(1, 256)
        else:
            t, l = int(rng.integers(0, h)), int(rng.integers(0, w))
            b, r = int(rng.integers(t, h)), int(rng.integers(l, w))
            if kind == 3:
                t = 0
            elif kind == 4:
                r = w - 1
            m[t:b + 1, l:r + 1] = rng.integers(1, 256, (b + 1 - t, r + 1 - l), dtype=np.uint8)
            m[t:b + 1, l:r + 1] *= rng.random((b + 1 - t, r + 1 - l)) < 0.7
            m[t, l] = m[b, r] = 200
        out.append(m)
    return out


def prepare_frame_numpy(images, masks, annots, views, mask_frames, use_mask, L):
    """get_data's per-view lines (genebody_fitting.py:119-140) in numpy: image_cropping, the > 128 mask, the crop and the two
    INTER_LINEAR resizes - the host restatement the device path is compared with"""
    from bodyfitting_amd.genebody import cv2_resize_linear, image_cropping
    cams = annots["cams"] if "cams" in annots else annots
    Ks, Rts, use_frames, mask_out, imgs, msks = [], [], [], [], [], []
    for i, view in enumerate(views):
        img, msk = np.asarray(images[i]), np.asarray(masks[i])
        top, left, bottom, right = image_cropping(msk)
        img = img * (msk > 128)[..., None]
        img = cv2_resize_linear(img[top:bottom, left:right].copy(), (L, L))
        if np.mean(img) > 10:
            use_frames.append(view)
            imgs.append(img)
            if view in mask_frames and use_mask:
                msks.append(cv2_resize_linear(msk[top:bottom, left:right].copy(), (L, L)))
                mask_out.append(view)
            K, Rt = cams["K"][i].copy(), cams["RT"][i].copy()
            K[0, 2] -= left
            K[1, 2] -= top
            K[0, :] *= L / float(right - left)
            K[1, :] *= L / float(bottom - top)
            Ks.append(K.astype(np.float32))
            Rts.append(Rt.astype(np.float32))
    return imgs, msks, Ks, Rts, use_frames, mask_out


def read_frame(root, subject, views, frame):
    """the decoded images and masks of one frame, as the runner's get_data reads them"""
    from bodyfitting_amd.genebody import read_image
    base = os.path.join(root, subject)
    names = sorted(os.listdir(os.path.join(base, "image", "00")))
    mnames = sorted(os.listdir(os.path.join(base, "mask", "00")))
    imgs = [read_image(os.path.join(base, "image", "%02d" % v, names[frame])) for v in views]
    msks = [read_image(os.path.join(base, "mask", "%02d" % v, mnames[frame])) for v in views]
    return imgs, msks
