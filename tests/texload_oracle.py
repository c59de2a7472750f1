"""numpy restatement of neural_renderer's load_textures_cuda_kernel (thirdparty/neural_renderer/neural_renderer/cuda/
load_textures_cuda_kernel.cu), one call = one launch of the reference: `load_textures(image, faces, textures, is_update, wrapping,
use_bilinear)` with image float32 [H, W, 3] (already flipped and / 255, as load_obj.py:84-96 passes it), faces float32 [NF, 3, 2]
(the faces' `vt` corners), textures float32 [NF, ts, ts, ts, 3] (updated faces are overwritten, a new array is returned),
is_update int32 [NF].  TEST INFRASTRUCTURE ONLY.

float32 throughout, every operation rounded where the kernel rounds it (numpy never fuses a multiply-add):
  * dim_k = (index along axis k) / (ts - 1.) in double, stored as float; if 0 < dim0 + dim1 + dim2 each is divided by that float sum;
  * the face's corners are wrapped ONCE (the reference wraps the shared array in place from every thread of the face - DESIGN.md
    section 2): REPEAT mod(x, 1), MIRRORED_REPEAT mod(x, 1) or 1 - mod(x, 1) by mod(x, 2) < 1, CLAMP_TO_EDGE min / max,
    with mod(x, y) = fmod(x, y) for x > 0 and y + fmod(x, y) otherwise;
  * pos = ((c0 * dim0 + c1 * dim1) + c2 * dim2) * float(W - 1) (and H - 1 for v);
  * bilinear: the four taps (y0, x0), (y1, x0), (y0, x1), (y1, x1) with y1 = min(int(pos_y + 1), H - 1) (the + 1 in float),
    x1 = min(int(pos_x) + 1, W - 1), accumulated from 0 in that order;
  * nearest: C's round(), half AWAY from zero (numpy's np.round is half to even, so it is not used);
  * CLAMP_TO_BORDER writes 0 to every texel of an updated face.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE, CLAMP_TO_BORDER = 0, 1, 2, 3


def texel_dims(ts):
    """-> float32 [ts^3, 3]: the barycentric position of every texel of a cube, in the kernel's texel order"""
    i = np.arange(ts ** 3)
    d = np.stack([(i // (ts * ts)) % ts, (i // ts) % ts, i % ts], 1).astype(np.float64) / (ts - 1.)
    d = d.astype(F32)
    s = ((d[:, 0] + d[:, 1]).astype(F32) + d[:, 2]).astype(F32)
    pos = 0 < s
    d[pos] = (d[pos] / s[pos, None]).astype(F32)
    return d


def cmod(x, y):
    x = np.asarray(x, F32)
    y = F32(y)
    r = np.fmod(x, y).astype(F32)
    return np.where(x > 0, r, (y + r).astype(F32)).astype(F32)


def wrap(c, wrapping):
    c = np.asarray(c, F32)
    if wrapping == REPEAT:
        return cmod(c, 1)
    if wrapping == MIRRORED_REPEAT:
        m1 = cmod(c, 1)
        return np.where(cmod(c, 2) < 1, m1, (F32(1) - m1).astype(F32)).astype(F32)
    if wrapping == CLAMP_TO_EDGE:
        return np.maximum(np.minimum(c, F32(1)), F32(0)).astype(F32)
    return c


def round_half_away(x):
    x = np.asarray(x, F32)
    a = np.abs(x)
    fl = np.floor(a)
    r = fl + ((a - fl) >= F32(0.5))
    return (np.sign(x) * r).astype(np.int64)


def load_textures(image, faces, textures, is_update, wrapping, use_bilinear):
    image = np.asarray(image, F32)
    tex = np.array(textures, F32)
    nf, ts = tex.shape[0], tex.shape[1]
    upd = np.nonzero(np.asarray(is_update) != 0)[0]
    if len(upd) == 0:
        return tex
    flat = tex.reshape(nf, ts ** 3, 3)
    if wrapping == CLAMP_TO_BORDER:
        flat[upd] = 0
        return tex
    d = texel_dims(ts)                                                      # [T, 3]
    faces = np.asarray(faces, F32).reshape(-1, 3, 2)
    for k in range(0, len(upd), 8192):                                      # (in chunks of faces: the temporaries are [U, T, 3])
        chunk = upd[k:k + 8192]
        flat[chunk] = _sample(image, wrap(faces[chunk], wrapping), d, use_bilinear)
    return tex


def _sample(image, c, d, use_bilinear):
    """the texels of the faces whose wrapped corners are c[U, 3, 2] -> [U, T, 3]"""
    H, W = image.shape[:2]

    def pos(axis, size):
        p = ((c[:, None, 0, axis] * d[None, :, 0]).astype(F32) + (c[:, None, 1, axis] * d[None, :, 1]).astype(F32)).astype(F32)
        p = (p + (c[:, None, 2, axis] * d[None, :, 2]).astype(F32)).astype(F32)
        return (p * F32(size - 1)).astype(F32)                              # [U, T]
    px, py = pos(0, W), pos(1, H)
    if use_bilinear:
        x0, y0 = px.astype(np.int64), py.astype(np.int64)                   # (truncation: the positions are >= 0)
        wx1 = (px - x0.astype(F32)).astype(F32); wx0 = (F32(1) - wx1).astype(F32)
        wy1 = (py - y0.astype(F32)).astype(F32); wy0 = (F32(1) - wy1).astype(F32)
        y1 = np.minimum((py + F32(1)).astype(F32).astype(np.int64), H - 1)
        x1 = np.minimum(x0 + 1, W - 1)
        col = F32(0)
        for (yy, xx, w) in ((y0, x0, (wx0 * wy0).astype(F32)), (y1, x0, (wx0 * wy1).astype(F32)),
                            (y0, x1, (wx1 * wy0).astype(F32)), (y1, x1, (wx1 * wy1).astype(F32))):
            col = (col + (image[yy, xx] * w[..., None]).astype(F32)).astype(F32)
        return col
    return image[round_half_away(py), round_half_away(px)]


def load_job(job, texture_size, wrapping, use_bilinear):
    """What bf_texfit_load_textures computes from obj_textures.parse_textures's arrays, the reference's way: the fill, then one
    launch per image on the faces that use it (image flipped and / 255 on the host, as load_obj.py:84-96)."""
    ts = int(texture_size)
    nf = len(job['face_image'])
    tex = np.broadcast_to(np.asarray(job['face_fill'], F32)[:, None, None, None, :], (nf, ts, ts, ts, 3)).copy()
    for j, img in enumerate(job['images']):
        image = (np.asarray(img).astype(F32) / 255.)[::-1]
        tex = load_textures(image, job['face_uv'], tex, (job['face_image'] == j).astype(np.int32), wrapping, use_bilinear)
    return tex
