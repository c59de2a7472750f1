"""The reference's texture inpainter (models/inpaint.py `Inpainter`, `LBAMModel(4, 3)`) and the hole mask and post-processing of
`TextureFitting.inpaint` (smplify/texture_fitting.py:191-214) on the GPU.

The network, the input preparation, the hole mask (face test and triangle fill), and the morphology run in `libbodyfit.so`
(csrc/inpaint_kernels.hip, inpaint_api.hip).  This module reads and packs the weights, and holds the numpy restatements the
kernels are held to: the face test and OpenCV's filled-contour rule (`hole_mask`, `fill_triangle`), cv2.erode / cv2.dilate with
a rectangle (`erode`, `dilate`), and the post-processing (`postprocess`).

Weights: `LBAM_NoBN_ParisStreetView.pth` (state-dict keys of LBAMModel, e.g. `ec1.conv.conv.weight`, `reverseConv1.activationFuncG_A.a`,
`dc7.weight`), read without torch by hmr.load_checkpoint, or a state dict registered with `assets.register_inpainter(...)`.  They
stay resident on the device in fp32.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _lib

ENC = (4, 64, 128, 256, 512, 512, 512, 512)          # ec1..ec7: ENC[l-1] -> ENC[l]
REV = (3, 64, 128, 256, 512, 512, 512)               # reverseConv1..6
DEC = ((512, 512), (1024, 512), (1024, 512), (1024, 256), (512, 128), (256, 64), (128, 3))   # dc1..dc7 (cin, cout)
# GaussActivation.forward's clamps (a, mu, sigma1, sigma2)
GAUSS_LO_64 = np.array([1.01, 0.1, 0.5, 0.5])
GAUSS_HI_64 = np.array([6.0, 3.0, 2.0, 2.0])
GAUSS_NAMES = ("a", "mu", "sigma1", "sigma2")
SIDE_MULTIPLE = 128                                  # seven stride-2 halvings and the decoder's concatenations
# ConvTranspose2d(4, 2, 1) as four 2 x 2 phases: output row 2j + py reads input row j + DY[py][t] with kernel row KY[py][t]
DY = ((0, -1), (1, 0))
KY = ((1, 3), (0, 2))


def expected_keys():
    """LBAMModel(4, 3).state_dict()'s keys -> shapes (no biases, no BatchNorm: the NoBN model)"""
    keys = collections.OrderedDict()
    for l in range(1, 8):
        cin, cout = ENC[l - 1], ENC[l]
        keys[f"ec{l}.conv.conv.weight"] = (cout, cin, 4, 4)
        keys[f"ec{l}.conv.maskConv.weight"] = (cout, 3 if cin == 4 else cin, 4, 4)
        for g in GAUSS_NAMES:
            keys[f"ec{l}.conv.activationFuncG_A.{g}"] = ()
    for l in range(1, 7):
        keys[f"reverseConv{l}.reverseMaskConv.weight"] = (REV[l], REV[l - 1], 4, 4)
        for g in GAUSS_NAMES:
            keys[f"reverseConv{l}.activationFuncG_A.{g}"] = ()
    for t in range(1, 7):
        cin, cout = DEC[t - 1]
        keys[f"dc{t}.conv.weight"] = (cin, cout, 4, 4)
    keys["dc7.weight"] = DEC[6] + (4, 4)
    return keys


def match_state(state, filename="LBAM_NoBN_ParisStreetView.pth"):
    """the state dict as load_state_dict(strict=True) takes it, as float32 arrays; a missing, unexpected or misshapen key raises
    ValueError naming it"""
    want = expected_keys()
    for key in state:
        if key not in want:
            raise ValueError(f"{filename}: unexpected key {key!r} (LBAMModel(4, 3) has no such parameter)")
    out = {}
    for key, shape in want.items():
        if key not in state:
            raise ValueError(f"{filename}: missing key {key!r} (LBAMModel(4, 3) needs every parameter)")
        a = np.asarray(state[key], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{filename}: {key!r} has shape {a.shape}, LBAMModel(4, 3) expects {shape}")
        out[key] = a
    return out


def load_weights(path):
    """LBAM_NoBN_*.pth -> matched float32 state dict, without torch"""
    from .hmr import load_checkpoint
    return match_state(load_checkpoint(path), path)


def gauss_params(state, prefix, dtype=np.float32):
    """(a, mu, sigma1, sigma2) of one GaussActivation as its forward uses them: clamped in place in the model's dtype (torch.clamp
    rounds the bounds to it, so a float64 model clamps to 1.01, a float32 one to float32(1.01))"""
    raw = np.array([np.float32(state[f"{prefix}.activationFuncG_A.{g}"]) for g in GAUSS_NAMES], dtype)
    return np.minimum(np.maximum(raw, GAUSS_LO_64.astype(dtype)), GAUSS_HI_64.astype(dtype))


def _pack_conv(w, cin_pad=None):
    """Conv2d weight [cout, cin, 4, 4] -> [16 * cinp][coutp] in (ky, kx, ci) order, cin and cout padded to 4 with zeros"""
    cout, cin = w.shape[:2]
    cp, co = cin_pad or (cin + 3) // 4 * 4, (cout + 3) // 4 * 4
    out = np.zeros((4, 4, cp, co), np.float32)
    out[:, :, :cin, :cout] = w.transpose(2, 3, 1, 0)
    return out.reshape(-1)


def _pack_deconv(w):
    """ConvTranspose2d weight [cin, cout, 4, 4] -> per phase (py, px) [4 * cin][coutp] in (ty, tx, ci) order"""
    cin, cout = w.shape[:2]
    co = (cout + 3) // 4 * 4
    out = np.zeros((2, 2, 2, 2, cin, co), np.float32)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    out[py, px, ty, tx, :, :cout] = w[:, :, KY[py][ty], KY[px][tx]]
    return out.reshape(-1)


def pack(state):
    """the matched state dict -> one float32 array in the order inpaint_api.hip walks the layers: reverseConv1..6, then per
    encoder level ec1..7 conv then maskConv, then dc1..dc7 (four phases each), then the clamped Gauss parameters (a, mu, sigma1,
    sigma2) of reverseConv1..6 and ec1..7"""
    parts, gauss = [], []
    for l in range(1, 7):
        parts.append(_pack_conv(state[f"reverseConv{l}.reverseMaskConv.weight"]))
        gauss.append(gauss_params(state, f"reverseConv{l}"))
    for l in range(1, 8):
        parts.append(_pack_conv(state[f"ec{l}.conv.conv.weight"]))
        parts.append(_pack_conv(state[f"ec{l}.conv.maskConv.weight"], ENC[l - 1] if l == 1 else None))
        gauss.append(gauss_params(state, f"ec{l}.conv"))
    for t in range(1, 7):
        parts.append(_pack_deconv(state[f"dc{t}.conv.weight"]))
    parts.append(_pack_deconv(state["dc7.weight"]))
    return np.ascontiguousarray(np.concatenate(parts + gauss), dtype=np.float32)


def check_size(H, W):
    if H % SIDE_MULTIPLE or W % SIDE_MULTIPLE or H < 1 or W < 1:
        raise ValueError(f"LBAM inpainting needs H and W that are multiples of {SIDE_MULTIPLE} (seven halvings); got {H} x {W}")


def _u8_images(a, what):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"{what}: expected uint8 [H, W, 3] images, got {a.dtype} {a.shape[1:] if a.ndim == 4 else a.shape}")
    return np.ascontiguousarray(a)


# ---------------------------------------------------------------------------------------------------------------------------------
# TextureFitting.inpaint: the hole mask
# ---------------------------------------------------------------------------------------------------------------------------------
def sample_dims():
    """texture_fitting.py:196-199: the 63 rows of {0..3}^3 without (0, 0, 0), each divided by its sum (float64)"""
    dims = np.array([[x, y, z] for x in range(4) for y in range(4) for z in range(4)][1:])
    return dims / np.sum(dims, axis=1, keepdims=True)


def select_faces(img, uv):
    """texture_fitting.py:200-204's face test: uv float32 [NF, 3, 2] in pixels -> bool [NF], the faces with more than 63 / 6 grey
    samples (every channel strictly between 118 and 138).  Indexing is numpy's: a negative index wraps, one past the end raises
    IndexError."""
    dims = sample_dims()
    sel = np.zeros(len(uv), bool)
    for i, face in enumerate(uv):
        f = (dims @ face).astype(np.int32)
        px = img[f[:, 1], f[:, 0], :]
        m = (px > np.ones(3) * 118) & (px < np.ones(3) * 138)
        tri = np.sum(m, axis=-1) == 3
        sel[i] = np.sum(np.array(tri).astype(np.int32)) > len(tri) / 6
    return sel


def sample_points_fma(uv):
    """the face test's sample coordinates as the kernel computes them: fma(d2, u2, fma(d1, u1, d0 * u0)) in float64, truncated ->
    int64 [NF, 63, 2].  numpy's `dims @ face` goes through BLAS; where it rounds differently a sample can truncate differently
    (tests report such samples).  Exact via integer arithmetic on the float64 values' rationals."""
    from fractions import Fraction
    dims = sample_dims()
    out = np.zeros((len(uv), 63, 2), np.int64)
    for i, face in enumerate(np.asarray(uv, np.float64)):
        for r in range(63):
            for c in range(2):
                a = float(Fraction(dims[r, 0]) * Fraction(face[0, c]))
                a = float(Fraction(dims[r, 1]) * Fraction(face[1, c]) + Fraction(a))
                a = float(Fraction(dims[r, 2]) * Fraction(face[2, c]) + Fraction(a))
                out[i, r, c] = int(a)
    return out


XY_SHIFT, XY_ONE = 16, 1 << 16


def _cdiv(a, b):
    """C's integer division (truncation toward zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clip_line(W, H, p1, p2):
    """OpenCV 4.1.2 clipLine(Size2l, Point2l&, Point2l&) -> (inside, p1, p2)"""
    (x1, y1), (x2, y2) = p1, p2
    right, bottom = W - 1, H - 1
    if W <= 0 or H <= 0:
        return False, p1, p2

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8
    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * (x2 - x1) / (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * (x2 - x1) / (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * (y2 - y1) / (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * (y2 - y1) / (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def line8(mask, p1, p2):
    """OpenCV's Line(img, pt1, pt2, color, 8): LineIterator(img, pt1, pt2, 8, leftToRight=true) over the clipped segment, every
    pixel set to 255"""
    H, W = mask.shape[:2]
    (x1, y1), (x2, y2) = p1, p2
    if not (0 <= x1 < W and 0 <= x2 < W and 0 <= y1 < H and 0 <= y2 < H):
        ok, (x1, y1), (x2, y2) = clip_line(W, H, (x1, y1), (x2, y2))
        if not ok:
            return
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    if dy > dx:                                        # major axis y
        dmaj, dmin, maj, mnr = dy, dx, (0, sy), (1, 0)
    else:
        dmaj, dmin, maj, mnr = dx, dy, (1, 0), (0, sy)
    err = dmaj - 2 * dmin
    x, y = x1, y1
    for _ in range(dmaj + 1):
        mask[y, x] = 255
        step = err < 0
        err += -2 * dmin + (2 * dmaj if step else 0)
        x += maj[0] + (mnr[0] if step else 0)
        y += maj[1] + (mnr[1] if step else 0)


def fill_triangle(mask, tri):
    """cv2.drawContours(mask, [tri], 0, 255, -1) for one int32 [3, 2] (x, y) triangle, LINE_8, shift 0, as OpenCV 4.1.2 runs it:
    CollectPolyEdges draws every edge of the closed contour p0 p1 p2 p0 (starting with p0 -> p0) with Line and collects the
    non-horizontal ones in 16.16 fixed point (x << 16, dx truncated); FillEdgeCollection then sets, on every row y0 <= y < y1 of the
    two active edges, the pixels from (x_left + 0xFFFF) >> 16 to x_right >> 16, clipped to the image.  mask: uint8 [H, W] or
    [H, W, C], written in place."""
    H, W = mask.shape[:2]
    pts = [tuple(int(v) for v in tri[i]) for i in (0, 1, 2, 0)]
    edges = []
    p0 = pts[-1]
    for p1 in pts:
        line8(mask, p0, p1)
        if p0[1] != p1[1]:
            top, bot = (p0, p1) if p0[1] < p1[1] else (p1, p0)
            dx = _cdiv((p1[0] << XY_SHIFT) - (p0[0] << XY_SHIFT), p1[1] - p0[1])
            edges.append((top[1], bot[1], top[0] << XY_SHIFT, dx))
        p0 = p1
    if len(edges) < 2:
        return
    for y in range(min(e[0] for e in edges), min(max(e[1] for e in edges), H)):
        xs = [x + (y - y0) * dx for y0, y1, x, dx in edges if y0 <= y < y1]
        assert len(xs) == 2, xs
        if y < 0:
            continue
        x1, x2 = (min(xs) + XY_ONE - 1) >> XY_SHIFT, max(xs) >> XY_SHIFT
        if x1 < W and x2 >= 0:
            mask[y, max(x1, 0):min(x2, W - 1) + 1] = 255


def hole_mask(img, uv):
    """texture_fitting.py:193-205: uint8 [H, W, 3] texture, uv float32 [NF, 3, 2] (load_obj_uv * H) -> (mask uint8 [H, W, 3] with 255 in
    every selected face's filled triangle, selected bool [NF])"""
    sel = select_faces(img, uv)
    mask = np.zeros_like(img)
    for face in np.asarray(uv)[sel]:
        fill_triangle(mask, np.array(face.astype(np.int32)))
    return mask, sel


# ---------------------------------------------------------------------------------------------------------------------------------
# cv2.erode / cv2.dilate with np.ones((k, k)) and the default border (pixels outside the image are ignored), and the post-processing
# ---------------------------------------------------------------------------------------------------------------------------------
def _morph(a, k, fn):
    a = np.asarray(a)
    r = k // 2
    H, W = a.shape[:2]
    out = a.copy()
    for dy in range(-r, k - r):
        for dx in range(-r, k - r):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] = fn(out[yd, xd], a[ys, xs])
    return out


def erode(a, k):
    """cv2.erode(a, np.ones((k, k), np.uint8)): the minimum over the k x k window around each pixel, per channel"""
    return _morph(a, k, np.minimum)


def dilate(a, k):
    """cv2.dilate(a, np.ones((k, k), np.uint8)): the maximum over the k x k window"""
    return _morph(a, k, np.maximum)


def quantize(network_out):
    """texture_fitting.py:207: (out * 255).astype(np.uint8), float32"""
    return (np.asarray(network_out, np.float32) * 255).astype(np.uint8)


def postprocess(img):
    """texture_fitting.py:209-214 on the quantized network output img (uint8 [H, W, 3])"""
    mask = (1 - (img == 255).astype(np.uint8))
    img2 = erode(img, 7)
    mask = erode(mask, 3)
    mask_d = dilate(mask, 7)
    mask2 = mask_d - mask
    return mask * img + mask2 * img2 + (1 - mask_d) * img


def morph_texture(tex_img, depth):
    """texture_fitting.py:154-161 (render_texture_map(morph=True)) on uint8 [H, W, 3] and float32 depth [H, W]"""
    valid = (depth[:, :, None] < 2).astype(np.uint8)
    valid2 = dilate(valid[:, :, 0], 3)[:, :, None]
    tex2 = erode(tex_img, 3)
    return (valid2 - valid) * tex2 + valid * tex_img + (1 - valid2) * tex2


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU
# ---------------------------------------------------------------------------------------------------------------------------------
MORPH_ERODE, MORPH_DILATE = 0, 1


def morph_u8(op, k, a, device=0):
    """bf_morph_u8 on uint8 [H, W] / [H, W, C] / [n, H, W, C]: cv2.erode (op 0) or cv2.dilate (op 1) with a k x k rectangle"""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError("morph_u8: uint8 images only")
    shp = a.shape
    b = a.reshape((1,) + shp + (1,)) if a.ndim == 2 else a.reshape((1,) + shp) if a.ndim == 3 else a
    b = np.ascontiguousarray(b)
    out = np.empty_like(b)
    lib = _lib.load()
    n, H, W, C = b.shape
    _lib.check(lib.bf_morph_u8(int(device), int(op), int(k), n, H, W, C, _u8p(b), _u8p(out)), "bf_morph_u8")
    return out.reshape(shp)


def _u8p(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


class Inpainter:
    """Inpainter(model_dir=None, device=0, max_batch=1): models/inpaint.py's Inpainter with LBAMModel(4, 3) resident on the GPU.
    `model_dir`: a path to the .pth, a state dict, or None for `assets.get_inpainter()`.  `inpainter(image, mask)` takes uint8
    [H, W, 3] image and mask (255 = hole), H and W multiples of 128, and returns float32 [H, W, 3] as the reference does; `batch`
    takes [n, H, W, 3] stacks.  Device buffers are sized to the largest image seen (at least 512 x 512) and max_batch."""

    def __init__(self, model_dir=None, device=0, max_batch=1):
        if model_dir is None:
            from . import assets
            packed = assets.get_inpainter()
        elif isinstance(model_dir, (str, bytes)) or hasattr(model_dir, "__fspath__"):
            packed = pack(load_weights(model_dir))
        else:
            packed = pack(match_state(model_dir))
        self._packed = packed
        self.device, self.max_batch = int(device), int(max_batch)
        self.max_h = self.max_w = 0
        self._h = None
        self._lib = None

    @classmethod
    def from_packed(cls, packed, device=0, max_batch=1):
        """an Inpainter on weights already packed (assets.get_inpainter())"""
        self = cls.__new__(cls)
        self._packed = np.ascontiguousarray(packed, np.float32)
        self.device, self.max_batch = int(device), int(max_batch)
        self.max_h = self.max_w = 0
        self._h = self._lib = None
        return self

    def _handle(self, H, W):
        import ctypes as C
        check_size(H, W)
        if self._h is not None and H <= self.max_h and W <= self.max_w:
            return self._h
        self.close()
        self._lib = _lib.load()
        n = int(self._lib.bf_inpaint_n_weights())
        if self._packed.size != n:
            raise ValueError(f"{self._packed.size} packed LBAM weights, the network has {n}")
        mh, mw = max(H, self.max_h, 512), max(W, self.max_w, 512)
        h = C.c_void_p()
        _lib.check(self._lib.bf_inpaint_create(self.device, _lib.fptr(self._packed), n, self.max_batch, mh, mw, C.byref(h)),
                   "bf_inpaint_create")
        self._h, self.max_h, self.max_w = h, mh, mw
        return h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.bf_inpaint_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch(self, images, masks):
        """uint8 [n, H, W, 3] images and masks -> float32 [n, H, W, 3], each image as __call__ gives it"""
        images, masks = _u8_images(images, "Inpainter.batch images"), _u8_images(masks, "Inpainter.batch masks")
        if images.shape != masks.shape:
            raise ValueError(f"Inpainter: image {images.shape} and mask {masks.shape} differ")
        n, H, W, _ = images.shape
        check_size(H, W)
        out = np.empty((n, H, W, 3), np.float32)
        for i in range(0, n, self.max_batch):
            k = min(self.max_batch, n - i)
            h = self._handle(H, W)
            _lib.check(self._lib.bf_inpaint_run(h, k, H, W, _u8p(images[i:i + k]), _u8p(masks[i:i + k]), _lib.fptr(out[i:i + k])),
                       "bf_inpaint_run")
        return out

    def __call__(self, image, mask):
        return self.batch(np.asarray(image)[None], np.asarray(mask)[None])[0]

    def hole_mask(self, img, uv):
        """the GPU face test and fill (bf_inpaint_hole_mask) -> uint8 [H, W, 3]"""
        img = _u8_images(np.asarray(img)[None], "Inpainter.hole_mask")[0]
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 3, 2)
        H, W = img.shape[:2]
        h = self._handle(H, W)
        mask = np.empty_like(img)
        _lib.check(self._lib.bf_inpaint_hole_mask(h, H, W, _u8p(img), len(uv), _lib.fptr(uv), _u8p(mask)), "bf_inpaint_hole_mask")
        return mask

    def select_faces(self, img, uv):
        """the GPU face test alone (bf_inpaint_select_faces) -> bool [NF]"""
        img = _u8_images(np.asarray(img)[None], "Inpainter.select_faces")[0]
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 3, 2)
        H, W = img.shape[:2]
        h = self._handle(H, W)
        sel = np.zeros(len(uv), np.uint8)
        _lib.check(self._lib.bf_inpaint_select_faces(h, H, W, _u8p(img), len(uv), _lib.fptr(uv), _u8p(sel)), "bf_inpaint_select_faces")
        return sel.astype(bool)

    def texture(self, img, uv, return_mask=False):
        """TextureFitting.inpaint on the GPU (bf_inpaint_texture): uint8 [H, W, 3] texture map, uv float32 [NF, 3, 2] in pixels
        (load_obj_uv * H) -> uint8 [H, W, 3] (and the hole mask)"""
        img = _u8_images(np.asarray(img)[None], "Inpainter.texture")[0]
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 3, 2)
        H, W = img.shape[:2]
        h = self._handle(H, W)
        out = np.empty_like(img)
        mask = np.empty_like(img) if return_mask else None
        _lib.check(self._lib.bf_inpaint_texture(h, H, W, _u8p(img), len(uv), _lib.fptr(uv), _u8p(out), _u8p(mask)), "bf_inpaint_texture")
        return (out, mask) if return_mask else out
