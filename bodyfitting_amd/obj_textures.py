"""`nr.load_obj` of neural_renderer (thirdparty/neural_renderer/neural_renderer/load_obj.py) without torch: the OBJ / MTL / texture
image files are read here, the per-face texture cubes are made on the GPU (bf_texfit_load_textures, csrc/tex_kernels.hip).

The parsing follows load_obj.py literally, including what looks wrong there:
  * polygons are fan-triangulated (v0, v[i+1], v[i+2]);
  * a face corner's `vt` index is that of `v/vt` and `v/vt/vn`; `v`, `v//vn` give index 0, which after the `- 1` is the LAST `vt`
    line (numpy's wraparound), and a negative `vt` index wraps the same way; no `vt` line at all is np.vstack([])'s ValueError;
  * a face's material is the last `usemtl` before it ('' before any); the MTL's `Kd` fills its material's faces, then every
    `map_Kd` image (only `split()[1]`, relative to the OBJ's directory) overwrites its material's faces; every line starting
    with `mtllib` loads the textures again and the last one wins; none with load_texture=True is 'Failed to load textures.'
  * images are decoded with PIL as skimage.io.imread does through imageio's pillow plugin: grey images are stacked to three
    channels, RGBA drops alpha, palette images are converted to RGB(A).
Deviations, all refusals of input the reference mishandles: a `v` index below 1 is a ValueError (torch's indexing would wrap it),
an image that is not 8-bit with 1, 3 or 4 channels is a ValueError naming the file (the reference reads a 16-bit PNG as values up
to 257 and a 2-channel image out of bounds), texture_size < 2 is a ValueError (the reference divides 0 by 0).
Wrapping is applied once per face.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _lib

TEXTURE_WRAPPING = {'REPEAT': 0, 'MIRRORED_REPEAT': 1, 'CLAMP_TO_EDGE': 2, 'CLAMP_TO_BORDER': 3}
DEFAULT_FILL = np.float32(0.5)          # torch.zeros(...) + 0.5 (load_obj.py:74)


def _rows(rows, dtype):
    """np.vstack(rows).astype(dtype), the fast way when every row has the same length (np.vstack's own error otherwise)"""
    if rows:
        try:
            a = np.array(rows)
        except ValueError:
            a = None
        if a is not None and a.ndim == 2:
            return a.astype(dtype)
    return np.vstack(rows).astype(dtype)


def _read_lines(filename):
    with open(filename) as f:
        return f.readlines()


def load_mtl(filename_mtl):
    """load_obj.py:13-29 -> (colors {material: float64[<=3]}, texture_filenames {material: file name as written})"""
    texture_filenames, colors, material_name = {}, {}, ''
    for line in _read_lines(filename_mtl):
        s = line.split()
        if len(s) != 0:
            if s[0] == 'newmtl':
                material_name = s[1]
            if s[0] == 'map_Kd':
                texture_filenames[material_name] = s[1]
            if s[0] == 'Kd':
                colors[material_name] = np.array(list(map(float, s[1:4])))
    return colors, texture_filenames


def read_image(filename):
    """skimage.io.imread(filename) as load_obj.py:84-92 uses it -> uint8 [H, W, 3], top row first"""
    from PIL import Image
    with Image.open(filename) as im:
        if im.mode == 'P':                                   # imageio's pillow plugin: palette -> its RGB(A)
            im = im.convert('RGBA' if 'transparency' in im.info else 'RGB')
        a = np.asarray(im)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (1, 3, 4))):
        raise ValueError(f"{filename}: texture images must be 8-bit with 1, 3 or 4 channels (got {a.dtype} {a.shape})")
    if a.ndim == 2:
        a = np.stack((a,) * 3, -1)
    elif a.shape[2] == 1:
        a = np.repeat(a, 3, 2)
    return np.ascontiguousarray(a[:, :, :3])


def _corner_vt(token):
    return int(token.split('/')[1]) if '/' in token and '//' not in token else 0


def parse_textures(filename_obj, filename_mtl, lines=None, timing=None):
    """The host half of load_textures (load_obj.py:31-95).  -> dict(face_uv float32 [NF, 3, 2], face_image int32 [NF] (-1: none),
    face_fill float32 [NF, 3], images [uint8 [H, W, 3]], image_files [path]); `timing` (a dict) receives the seconds spent decoding
    images (decode_s)"""
    lines = _read_lines(filename_obj) if lines is None else lines
    vt, faces, material_names, material_name = [], [], [], ''
    for line in lines:
        s = line.split()
        if len(s) == 0:
            continue
        if s[0] == 'vt':
            vt.append([float(v) for v in s[1:3]])
        elif s[0] == 'f':
            vs = s[1:]
            v0 = _corner_vt(vs[0])
            for i in range(len(vs) - 2):
                faces.append((v0, _corner_vt(vs[i + 1]), _corner_vt(vs[i + 2])))
                material_names.append(material_name)
        elif s[0] == 'usemtl':
            material_name = s[1]
    vt = _rows(vt, np.float32)
    face_uv = np.ascontiguousarray(vt[_rows(faces, np.int32) - 1])            # (numpy indexing: 0 and negatives wrap)
    colors, texture_filenames = load_mtl(filename_mtl)
    names = np.array(material_names)
    face_fill = np.full((len(names), 3), DEFAULT_FILL, np.float32)
    for name, color in colors.items():
        sel = names == name
        if sel.any():
            face_fill[sel] = np.broadcast_to(color, (3,)).astype(np.float32)
    face_image = np.full(len(names), -1, np.int32)
    images, image_files, decoded = [], [], {}
    for name, fn in texture_filenames.items():
        path = os.path.join(os.path.dirname(filename_obj), fn)
        key = os.path.abspath(path)
        if key not in decoded:
            decoded[key] = len(images)
            t0 = time.perf_counter()
            images.append(read_image(path))
            if timing is not None:
                timing['decode_s'] = timing.get('decode_s', 0.0) + time.perf_counter() - t0
            image_files.append(path)
        face_image[names == name] = decoded[key]
    return dict(face_uv=face_uv, face_image=face_image, face_fill=face_fill, images=images, image_files=image_files)


def run_load_textures(job, texture_size, texture_wrapping='REPEAT', use_bilinear=True, device=0, timing=None):
    """bf_texfit_load_textures on what parse_textures returned -> float32 [NF, ts, ts, ts, 3]; `timing` (a dict) receives the
    upload / kernel / download milliseconds"""
    ts = int(texture_size)
    if ts < 2:
        raise ValueError(f"texture_size must be at least 2 (got {texture_size}): the texel positions divide by texture_size - 1")
    if texture_wrapping not in TEXTURE_WRAPPING:
        raise KeyError(texture_wrapping)
    lib = _lib.load()
    uv = np.ascontiguousarray(job['face_uv'], np.float32)
    fimg = np.ascontiguousarray(job['face_image'], np.int32)
    fill = np.ascontiguousarray(job['face_fill'], np.float32)
    imgs = [np.ascontiguousarray(a, np.uint8) for a in job['images']]
    if any(a.ndim != 3 or a.shape[2] != 3 for a in imgs):
        raise ValueError("images must be uint8 [H, W, 3] (obj_textures.read_image)")
    n = len(imgs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in imgs])
    hs = np.array([a.shape[0] for a in imgs] or [0], np.int32)
    ws = np.array([a.shape[1] for a in imgs] or [0], np.int32)
    out = np.empty((len(fimg), ts, ts, ts, 3), np.float32)
    ms = np.zeros(3, np.float32)
    _lib.check(lib.bf_texfit_load_textures(int(device), len(fimg), _lib.fptr(uv), _lib.iptr(fimg), _lib.fptr(fill), n,
                                           C.cast(ptrs, C.POINTER(C.c_void_p)), _lib.iptr(hs), _lib.iptr(ws), ts,
                                           TEXTURE_WRAPPING[texture_wrapping], int(bool(use_bilinear)), _lib.fptr(out), _lib.fptr(ms)),
               "bf_texfit_load_textures")
    if timing is not None:
        timing.update(upload_ms=float(ms[0]), kernel_ms=float(ms[1]), download_ms=float(ms[2]))
    return out


def load_vertices(filename_obj, lines=None):
    """the `v` lines (load_obj.py:105-114) -> float32 [NV, 3]"""
    lines = _read_lines(filename_obj) if lines is None else lines
    verts = []
    for line in lines:
        s = line.split()
        if len(s) != 0 and s[0] == 'v':
            verts.append([float(v) for v in s[1:4]])
    return _rows(verts, np.float32)


def load_faces(filename_obj, lines=None):
    """the `f` lines (load_obj.py:116-128), fan-triangulated -> int32 [NF, 3], 0-based"""
    lines = _read_lines(filename_obj) if lines is None else lines
    faces = []
    for line in lines:
        s = line.split()
        if len(s) != 0 and s[0] == 'f':
            vs = s[1:]
            v0 = int(vs[0].split('/')[0])
            for i in range(len(vs) - 2):
                faces.append((v0, int(vs[i + 1].split('/')[0]), int(vs[i + 2].split('/')[0])))
    faces = _rows(faces, np.int32) - 1
    if (faces < 0).any():
        raise ValueError(f"{filename_obj}: a face refers to a vertex index below 1 (relative indices are not supported)")
    return faces


def normalize_vertices(vertices):
    """load_obj.py:141-146: the four in-place float32 steps into a unit cube centred at zero"""
    v = np.array(vertices, np.float32)
    v -= v.min(0)[None, :]
    v /= np.abs(v).max()
    v *= 2
    v -= v.max(0)[None, :] / 2
    return v


def mtllib_files(filename_obj, lines):
    """every line starting with `mtllib` names an MTL relative to the OBJ (load_obj.py:132-135)"""
    return [os.path.join(os.path.dirname(filename_obj), line.split()[1]) for line in lines if line.startswith('mtllib')]


def load_obj(filename_obj, normalization=True, texture_size=4, load_texture=False, texture_wrapping='REPEAT', use_bilinear=True,
             device=0):
    """nr.load_obj with numpy results: -> (vertices float32 [NV, 3], faces int32 [NF, 3]) or, with load_texture,
    (vertices, faces, textures float32 [NF, ts, ts, ts, 3]) made on HIP device `device`"""
    lines = _read_lines(filename_obj)
    vertices = load_vertices(filename_obj, lines)
    faces = load_faces(filename_obj, lines)
    textures = None
    if load_texture:
        if int(texture_size) < 2:
            raise ValueError(f"texture_size must be at least 2 (got {texture_size}): the texel positions divide by texture_size - 1")
        mtls = mtllib_files(filename_obj, lines)
        if not mtls:
            raise Exception('Failed to load textures.')
        for m in mtls[:-1]:
            load_mtl(m)                          # (each is loaded by the reference too - a missing one raises - and then replaced)
        job = parse_textures(filename_obj, mtls[-1], lines)
        textures = run_load_textures(job, texture_size, texture_wrapping, use_bilinear, device)
    if normalization:
        vertices = normalize_vertices(vertices)
    if load_texture:
        return vertices, faces, textures
    return vertices, faces
