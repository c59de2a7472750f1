"""The reference's mesh-data texture entry points on the HIP path, for apps/rp_fitting.py:
  * `render_texture_mesh` / `gen_cam_views` of utils/renderer.py (the 8 views `render_data` renders from a textured scan);
  * `TextureFitting(smpl_uv_dir, ...)(output_dir, smpld_dir, scan_dir)` of smplify/texture_fitting.py:173-301 and its helpers
    `load_obj_uv`, `create_smpld_uv`, `sphere2rot`, `to8b`, `render_texture_map`.
`dropin/utils/renderer.py` and `dropin/smplify/texture_fitting.py` re-export them, so the reference's import lines resolve here.
Files are read by `obj_textures.load_obj` (nr.load_obj), the loop is `texture_fitting.TextureFitting.fit`, every render is
libbodyfit's (bf_texfit_*).  No torch, neural_renderer or CUDA import on this path.

`TextureFitting(inpaint=True)` runs the LBAM inpainter, its hole mask and post-processing on the GPU (inpaint.Inpainter).

Two things differ from the reference on purpose: `video.mp4` (both places) is not written - there is no video encoder here - and
`render_texture_mesh(..., pose_only=True)` reads only the `v` lines, so a mesh without textures no longer raises in that mode.
"""
from __future__ import annotations

import os
import shutil
import sys

import numpy as np

from . import inpaint as IP
from . import obj_textures as OT
from . import texture_fitting as TF

ROUND_VIEWS, ROUND_VIEW_ITERS = TF.ROUND_VIEWS, TF.ROUND_VIEW_ITERS


def gen_cam_views(center, viewnum, dist, gl=False):
    """utils/renderer.py:7-25, written as the reference writes it (np.linspace angles): world-to-camera poses on a ring"""
    def viewmatrix(z, up, translation):
        vec3 = z / np.linalg.norm(z)
        up = up / np.linalg.norm(up)
        vec1 = np.cross(up, vec3)
        vec2 = np.cross(vec3, vec1)
        view = np.stack([vec1, vec2, vec3, translation], axis=1)
        return np.concatenate([view, np.array([[0, 0, 0, 1]])], axis=0)
    cam_poses = []
    cv2gl = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]]) if gl else np.eye(4)
    for theta in np.linspace(0, 2 * np.pi, viewnum + 1)[:-1]:
        z = np.array([np.cos(theta), 0, -np.sin(theta)]) * dist
        cam_poses.append(cv2gl @ np.linalg.inv(viewmatrix(z, np.array([0, 1, 0]), z + center)))
    return cam_poses


def sphere2rot(rad, theta, phi, t=(0, 0, 0)):
    """smplify/texture_fitting.py:63-83, written as the reference writes it: camera-to-world pose looking at `t`"""
    def normalize(x):
        return x / np.linalg.norm(x)
    transl = np.array([rad * np.sin(theta) * np.sin(phi), rad * np.cos(theta), rad * np.sin(theta) * np.cos(phi)])
    z = normalize(-transl)
    right = np.array([np.sin(phi + np.pi / 2), 0, np.cos(phi + np.pi / 2)])
    y = normalize(np.cross(z, right))
    x = normalize(np.cross(y, z))
    R = np.eye(4)
    R[:3, :3] = np.stack([x, y, z], axis=1)
    R[:3, 3] = transl + np.array(t)
    return R


def to8b(x):
    """texture_fitting.py:41.  It flips the channel axis, undoing the caller's [:, :, ::-1]: smpl.png and the render / debug images
    are RGB (texture_fitting.render_texture_map returns the other order)"""
    return (np.clip(np.flip(x, 2), 0, 1) * 255).astype(np.uint8)


def scene_bound(verts):
    """the bounding-box centre (float32) and dist = height / 0.8 with the float32 height divided in float64 - numpy 1's promotion of a
    float32 scalar over a Python float, the environment of texture_fitting.py:235-239 and utils/renderer.py:29-37 (numpy 2 would
    divide in float32)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    center = (v.max(0) + v.min(0)) / 2.0
    bound = v.max(0) - v.min(0)
    return center, np.float64(bound[1]) / 0.8


def _imwrite(path, img):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img)).save(path)


def _no_video(path):
    print(f"{path} not written: no video encoder on this path", file=sys.stderr)


def render_texture_mesh(file, imgsize=512, viewnum=8, white_bkgd=False, pose_only=False, device=0):
    """utils/renderer.py:27-61 -> (imgs [uint8 H x W x 3 RGB], masks [uint8 H x W], poses [world-to-camera 4x4, GL axes], Ks);
    pose_only=True -> (poses, Ks)"""
    if pose_only:
        vert = OT.load_vertices(file)
    else:
        vert, face, tex = OT.load_obj(file, normalization=False, load_texture=True, device=device)
    center, dist = scene_bound(vert)
    K = np.array([[imgsize, 0, imgsize / 2], [0, imgsize, imgsize / 2], [0, 0, 1]])
    poses = gen_cam_views(center, viewnum, dist, gl=True)
    Ks = [K for _ in range(viewnum)]
    if pose_only:
        return poses, Ks
    far = 2 * dist
    r = TF.Renderer(imgsize, tex.shape[1], near=0.0, far=far, background=(0.0, 0.0, 0.0), K=K, orig_size=imgsize, device=device)
    imgs, masks = [], []
    try:
        r.set_mesh(r.TARGET, (vert, face, tex))
        for pose in poses:
            rgb, depth = r.render_rgbd(r.TARGET, pose)
            image = (np.clip(rgb.transpose((1, 2, 0))[:imgsize, :imgsize, :], 0, 1) * 255).astype(np.uint8)
            mask = (np.clip((depth[:imgsize, :imgsize] < np.float32(far)), 0, 1) * 255).astype(np.uint8)
            if white_bkgd:
                image = image + (255 - mask[..., None])
            imgs.append(image)
            masks.append(mask)
    finally:
        r.close()
    return imgs, masks, poses, Ks


def load_obj_uv(filename):
    """texture_fitting.py:14-59: the UV corners (u, 1 - v) of every face of an OBJ -> float32 [NF, 3, 2]"""
    with open(filename) as f:
        lines = f.readlines()
    uv = []
    for line in lines:
        s = line.split()
        if len(s) != 0 and s[0] == 'vt':
            uv.append([float(s[1]), 1 - float(s[2])])
    uv = np.vstack(uv).astype(np.float32)
    faces_t = []
    for line in lines:
        s = line.split()
        if len(s) != 0 and s[0] == 'f':
            vs = s[1:]
            vt = [int(t.split('/')[1]) if '/' in t and '//' not in t else 0 for t in vs]
            for i in range(len(vs) - 2):
                faces_t.append((vt[0], vt[i + 1], vt[i + 2]))
    return uv[np.vstack(faces_t).astype(np.int32) - 1]


def create_smpld_uv(output_dir, smpld_dir, smpl_uv_dir, tex_img_size):
    """texture_fitting.py:85-117: the SMPL+D OBJ `output_dir` = the `v ` lines of `smpld_dir`, then per `mtllib` of the UV OBJ
    `mtllib` + `usemtl <its last newmtl>`, then the UV OBJ's `vt ` / `f ` lines in their order; the MTL is copied next to it and a
    tex_img_size^2 texture of grey 128 written under its last `map_Kd` name"""
    new_lines = []
    with open(smpld_dir) as f_v:
        new_lines += [line for line in f_v.readlines() if line.startswith("v ")]
    with open(smpl_uv_dir) as f_uv:
        lines = f_uv.readlines()
    for line in lines:
        if line.startswith('mtllib'):
            mtl = os.path.join(os.path.dirname(smpl_uv_dir), line.split()[1])
            new_mtl = os.path.join(os.path.dirname(output_dir), line.split()[1])
            if os.path.abspath(mtl) != os.path.abspath(new_mtl):
                shutil.copy(mtl, new_mtl)
            mtl_name = tex_dir = None
            with open(mtl) as f_mtl:
                for m_line in f_mtl.readlines():
                    if m_line.startswith("newmtl"):
                        mtl_name = m_line.split()[1]
                    elif m_line.startswith("map_Kd"):
                        tex_dir = m_line.split()[1]
            if mtl_name is None or tex_dir is None:
                raise ValueError(f"{mtl}: the SMPL UV material needs a newmtl and a map_Kd line")
            new_lines += [f"mtllib {line.split()[1]}\n", f"usemtl {mtl_name}\n"]
            _imwrite(os.path.join(os.path.dirname(output_dir), tex_dir), np.ones([tex_img_size, tex_img_size, 3], dtype=np.uint8) * 128)
        if line.startswith("f "):
            new_lines.append(line)
        elif line.startswith("vt "):
            new_lines.append(line)
    with open(output_dir, 'w') as f_smpl:
        f_smpl.writelines(new_lines)


def _uv_obj(filename):
    """what Renderer.render_texture (neural_renderer/renderer.py:294-332) reads from an OBJ: the `vt` lines (float64, as Python
    parses them) and the 0-based vt index of every face corner (index 0 / missing -> the last vt, negatives wrap)"""
    lines = OT._read_lines(filename)
    uv = []
    for line in lines:
        s = line.split()
        if len(s) != 0 and s[0] == 'vt':
            uv.append([float(v) for v in s[1:3]])
    uv = np.vstack(uv).astype(np.float64)
    faces = []
    for line in lines:
        s = line.split()
        if len(s) != 0 and s[0] == 'f':
            vs = s[1:]
            vt = [OT._corner_vt(t) for t in vs]
            for i in range(len(vs) - 2):
                faces.append((vt[0], vt[i + 1], vt[i + 2]))
    faces = np.vstack(faces).astype(np.int64) - 1
    if (faces >= len(uv)).any() or (faces < -len(uv)).any():
        raise IndexError(f"{filename}: a face refers to a vt line that does not exist")
    return uv, (faces % len(uv)).astype(np.int32)


def render_texture_map(renderer, objdir, textures=None, morph=False):
    """texture_fitting.py:149-171: the UV-space image of `textures` (default: the renderer's fitted ones) over the UV OBJ `objdir`
    -> uint8 [H, W, 3] RGB (the reference's to8b).  morph=True: pixels the UV triangles do not cover (depth >= 2) take the 3 x 3
    erosion of the image, as cv2.erode / cv2.dilate give it (bf_morph_u8)"""
    uv, uv_faces = _uv_obj(objdir)
    rgb, depth = renderer.render_texture(uv, uv_faces, textures)
    tex_img = to8b(rgb.transpose((1, 2, 0))[:, :, ::-1])
    if morph:
        device = renderer.device
        valid_mask = (depth[:, :, None] < 2).astype(np.uint8)
        valid_mask2 = IP.morph_u8(IP.MORPH_DILATE, 3, valid_mask[:, :, 0], device)[:, :, None]
        tex_img2 = IP.morph_u8(IP.MORPH_ERODE, 3, tex_img, device)
        tex_img = (valid_mask2 - valid_mask) * tex_img2 + valid_mask * tex_img + (1 - valid_mask2) * tex_img2
    return tex_img


class TextureFitting:
    """smplify/texture_fitting.py:173-301.  inpaint=True resolves the LBAM weights here (`assets.get_inpainter()`: the registered
    ones, else external/LBAM_NoBN_ParisStreetView.pth; neither raises assets.InpainterWeightsMissing) and runs the network on the
    GPU, opened on the first `inpaint`.  `debug` is taken for its truth value (apps/rp_fitting.py passes distutils' `debug`
    function)."""

    def __init__(self, smpl_uv_dir, tex_img_size=1024, render_img_size=512, lrate=1e-2, iter_num=200, debug=False, render=True,
                 inpaint=False, logging=False, device=0):
        self.debug, self.render, self.iter_num, self.lrate = debug, render, iter_num, lrate
        self.tex_img_size, self.img_size, self.is_inpaint, self.logging = tex_img_size, render_img_size, inpaint, logging
        self.smpl_uv_dir, self.device = smpl_uv_dir, device
        self.inpainter = None
        if self.is_inpaint:
            from . import assets
            self._inpaint_weights = assets.get_inpainter()

    def inpaint(self, img):
        """texture_fitting.py:191-214 on the GPU: the hole mask of the UV faces with grey samples, Inpainter(img, mask), the uint8
        round trip and the erode / dilate post-processing -> uint8 [H, W, 3]"""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        uv = load_obj_uv(self.smpl_uv_dir)
        uv = uv * img.shape[0]
        if self.inpainter is None:
            weights = getattr(self, "_inpaint_weights", None)
            if weights is None:
                from . import assets
                weights = assets.get_inpainter()
            self.inpainter = IP.Inpainter.from_packed(weights, device=self.device)
        return self.inpainter.texture(img, uv)

    def views(self, center, dist):
        """the view of every iteration (:255-263): five rounds of the 18-view ring, then sphere2rot at np.random.uniform(0, pi),
        np.random.uniform(0, 2 pi) from the global generator, inverted"""
        round_poses = gen_cam_views(center, ROUND_VIEWS, dist, gl=True)
        poses = []
        for i in range(self.iter_num):
            if i < ROUND_VIEW_ITERS * len(round_poses):
                pose = round_poses[i % len(round_poses)]
            else:
                pose = np.linalg.inv(sphere2rot(dist, np.random.uniform(0, np.pi), np.random.uniform(0, np.pi * 2), t=center))
            poses.append(pose)
        return poses

    def __call__(self, output_dir, smpld_dir, scan_dir):
        os.makedirs(output_dir, exist_ok=True)
        smpld_uv_dir = os.path.join(output_dir, os.path.basename(smpld_dir))
        create_smpld_uv(smpld_uv_dir, smpld_dir, self.smpl_uv_dir, self.tex_img_size)
        smpl = OT.load_obj(smpld_uv_dir, normalization=False, load_texture=True, device=self.device)
        scan = OT.load_obj(scan_dir, normalization=False, load_texture=True, device=self.device)
        center, dist = scene_bound(scan[0])
        poses = self.views(center, dist)
        debug_dir = os.path.join(output_dir, 'debug')
        if self.debug:
            os.makedirs(debug_dir, exist_ok=True)

        def before_step(i, pose, r):                  # :272-275: the fitted mesh as this iteration renders it, before the step
            if self.debug:
                img = r.render_rgb(r.FITTED, pose)
                _imwrite(os.path.join(debug_dir, f"{i}.png"), to8b(img.transpose((1, 2, 0))[:, :, ::-1][:self.img_size, :self.img_size, :]))

        out = {}

        def after_fit(r):
            if self.render:                           # :281-285, render_compare (:119-147)
                render_dir = os.path.join(output_dir, 'render')
                os.makedirs(render_dir, exist_ok=True)
                for i, pose in enumerate(gen_cam_views(center, 36, dist, gl=True)):
                    if self.logging:
                        print(f"rendering {i}th view")
                    scan_img = to8b(r.render_rgb(r.TARGET, pose).transpose((1, 2, 0))[:, :, ::-1])
                    smpl_img = to8b(r.render_rgb(r.FITTED, pose).transpose((1, 2, 0))[:, :, ::-1])
                    _imwrite(os.path.join(render_dir, f"{i:04d}.png"), np.hstack((scan_img, smpl_img)))
                _no_video(os.path.join(render_dir, 'video.mp4'))
            print("generating smpl texture...")
            out['tex_img'] = render_texture_map(r, self.smpl_uv_dir)

        fitter = TF.TextureFitting(self.img_size, self.lrate, self.iter_num, logging=self.logging, device=self.device)
        textures, losses = fitter.fit(smpl, scan, poses=poses, far=2 * dist, before_step=before_step, after_fit=after_fit)
        if self.debug:
            _no_video(os.path.join(debug_dir, 'video.mp4'))
        tex_img = out['tex_img']
        if self.is_inpaint:
            tex_img = self.inpaint(tex_img)
        _imwrite(os.path.join(output_dir, "smpl.png"), tex_img)
        self.textures, self.losses = textures, losses
        return textures, losses
