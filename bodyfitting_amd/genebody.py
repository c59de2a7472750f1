"""GeneBody captures end to end: the reference's `apps/genebody_fitting.py` on the GPU.

`python -m bodyfitting_amd.genebody --target_dir ... --subject ...` takes a GeneBody capture from its dataset folder to fitted SMPL /
SMPL-X parameters with the reference's options, tasks and files:

- `get_data`'s per-view work (genebody_fitting.py:119-140) runs for all views of a frame at once in `libbodyfit.so`
  (csrc/views_kernels.hip, views_api.hip) through `ViewPrep`: the mask bounding box on the device, image_cropping's scalar arithmetic
  on the host, then one fused crop, mask, resize and sum kernel.  Only each view's crop rectangle of the image goes up.
- the `openpose` task detects on the GPU (`openpose.OpenPose`, and `openpose_hand.OpenPoseHand` for SMPL-X as `--hand` asks) in place
  of openpose.bin, writes the JSON files openpose.bin writes, and `read_openpose` reads them back as the reference does.
- the `smplify` task is `body_fitting.BodyFitting`, the `output` task copies what it wrote.

`image_cropping` and `cv2_resize_linear` are numpy restatements of utils/io_utils.py:97-136 and of the cv2.resize calls the app makes;
they are the checker of the kernels (tests/), never a fallback: without a device `ViewPrep` fails as the rest of the library does.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import csv
import ctypes as C
import os
import shutil
import sys

import numpy as np

from . import _lib

MASK_FRAMES = [1, 7, 13, 19, 25, 31, 37, 43]        # genebody_fitting.py:88, the views with ground-truth masks


# ---------------------------------------------------------------------------------------------------------------------------------
# host restatements (the checker of the kernels)
# ---------------------------------------------------------------------------------------------------------------------------------
def crop_from_box(top, left, bottom, right, h, w):
    """utils/io_utils.py:103-136: image_cropping's arithmetic on the box (top, left, bottom, right) of mask != 0 (max inclusive) of an
    h x w mask, as the reference computes it: numpy int64 against Python float, int() truncation, `left` padded by bbox_h * 0.1 (sic),
    and the four clamp branches.  -> (top, left, bottom, right) as Python ints, unclipped (left can be negative, right beyond w)."""
    top, left, bottom, right = np.int64(top), np.int64(left), np.int64(bottom), np.int64(right)
    bbox_h, bbox_w = bottom - top, right - left

    bottom = min(int(bbox_h * 0.1 + bottom), h)
    top = max(int(top - bbox_h * 0.1), 0)
    right = min(int(bbox_w * 0.1 + right), w)
    left = max(int(left - bbox_h * 0.1), 0)
    bbox_h, bbox_w = bottom - top, right - left

    if bbox_h >= bbox_w:
        w_c = (left + right) / 2
        size = bbox_h
        if w_c - size / 2 < 0:
            left = 0
            right = size
        elif w_c + size / 2 >= w:
            left = w - size
            right = w
        else:
            left = int(w_c - size / 2)
            right = left + size
    else:
        h_c = (top + bottom) / 2
        size = bbox_w
        if h_c - size / 2 < 0:
            top = 0
            bottom = size
        elif h_c + size / 2 >= h:
            top = h - size
            bottom = h
        else:
            top = int(h_c - size / 2)
            bottom = top + size
    return top, left, bottom, right


def image_cropping(mask):
    """utils/io_utils.py:97-136 on a mask [H, W]: the square crop (top, left, bottom, right); an empty mask raises ValueError as np.min
    does"""
    m = np.asarray(mask)
    a = np.where(m != 0)
    h, w = list(m.shape[:2])
    return crop_from_box(np.min(a[0]), np.min(a[1]), np.max(a[0]), np.max(a[1]), h, w)


def slice_rect(crop, H, W, what="view"):
    """the rectangle `img[top:bottom, left:right]` actually reads: slice(...).indices() per axis (a negative start wraps as numpy
    wraps it, an overshooting stop is clipped); an empty one is an error (cv2.resize asserts on it)"""
    top, left, bottom, right = (int(x) for x in crop)
    r0, r1, _ = slice(top, bottom).indices(H)
    c0, c1, _ = slice(left, right).indices(W)
    if r1 <= r0 or c1 <= c0:
        raise ValueError(f"{what}: the crop {tuple(crop)} of a {H} x {W} image is empty")
    return r0, c0, r1, c1


def _axis(n_src, L, clamp_weight):
    """one axis of cv2.resize INTER_LINEAR on 8-bit data (hmr._axis for any n_src -> L): OpenCV's scale 1 / (L / n_src)"""
    scale = 1.0 / (L / n_src)
    f = ((np.arange(L) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_weight:
        lo, hi = s < 0, s >= n_src - 1
        f[lo], s[lo] = 0, 0
        f[hi], s[hi] = 0, n_src - 1
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1), a0, a1


def cv2_resize_linear(src, dsize):
    """cv2.resize(src, dsize) with the default INTER_LINEAR on uint8 [H, W] or [H, W, C], dsize = (width, height): OpenCV's 8-bit
    fixed-point arithmetic in integers (see csrc/views_kernels.hip)"""
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"cv2_resize_linear takes uint8 [H, W] or [H, W, C]; got {a.dtype} {a.shape}")
    flat = a.ndim == 2
    img = (a[:, :, None] if flat else a).astype(np.int64)
    H, W = img.shape[:2]
    dw, dh = int(dsize[0]), int(dsize[1])
    x0, x1, a0, a1 = _axis(W, dw, True)
    y0, y1, b0, b1 = _axis(H, dh, False)
    edge = x0 == W - 1
    h = img[:, x0] * a0[None, :, None] + img[:, x1] * a1[None, :, None]
    h[:, edge] = img[:, x0[edge]] * 2048
    v = ((((b0[:, None, None] * (h[y0] >> 4)) >> 16) + ((b1[:, None, None] * (h[y1] >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
    return v[:, :, 0] if flat else v


# ---------------------------------------------------------------------------------------------------------------------------------
# the device object
# ---------------------------------------------------------------------------------------------------------------------------------
def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


class ViewPrep:
    """ViewPrep(device=0, L=512, max_views=48, max_h=0, max_w=0): get_data's per-view work on the GPU for all views of a frame.
    `bbox(masks)` uploads the masks (uint8 [H, W], one size per call) and leaves them resident; `prepare(rects, images, mask_view)` then
    crops, masks, resizes and sums the same views.  Buffers start at the sizes given and grow with the frames."""

    def __init__(self, device=0, L=512, max_views=48, max_h=0, max_w=0):
        self._lib = _lib.load()
        self.device, self.L = int(device), int(L)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_views_create(self.device, int(max_views), int(max_h), int(max_w), self.L, C.byref(self._h)),
                   "bf_views_create")
        self._n = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bf_views_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bbox(self, masks, names=None):
        """-> int32 [n, 4] (top, left, bottom, right) of mask != 0 per view, max inclusive.  An empty mask raises ValueError naming
        the view (names[i], default its index), as np.min on the empty np.where does in the reference."""
        ms = [np.ascontiguousarray(m) for m in masks]
        if not ms:
            raise ValueError("ViewPrep.bbox: no masks")
        H, W = ms[0].shape[:2]
        for i, m in enumerate(ms):
            if m.dtype != np.uint8 or m.ndim != 2 or m.shape != (H, W):
                raise ValueError(f"view {names[i] if names else i}: masks must be single-channel uint8 [H, W] of one size; got "
                                 f"{m.dtype} {m.shape}")
        box = np.zeros((len(ms), 4), np.int32)
        rc = self._lib.bf_views_bbox(self._h, len(ms), H, W, _ptrs(ms), _lib.iptr(box))
        self._n = 0
        if rc != 0:
            msg = self._lib.bf_last_error().decode("utf-8", "replace")
            if "the mask is empty" in msg:
                i = int(np.nonzero(box[:, 2] < 0)[0][0])
                raise ValueError(f"view {names[i] if names else i}: the mask is empty (no pixel != 0)")
            _lib.check(rc, "bf_views_bbox")
        self._n, self._hw = len(ms), (H, W)
        return box

    def prepare(self, rects, images, mask_view=None):
        """rects [n, 4] (top, left, bottom, right) within the views of the last bbox call, images uint8 [H, W, 3] of those views ->
        (images uint8 [n, L, L, 3], masks uint8 [n, L, L] (zero where mask_view is off), sums int64 [n])"""
        n, L = self._n, self.L
        if n < 1:
            raise ValueError("ViewPrep.prepare: call bbox on the frame's masks first")
        r = np.ascontiguousarray(np.asarray(rects, np.int64).reshape(-1, 4).astype(np.int32))
        ims = [np.ascontiguousarray(im) for im in images]
        if len(ims) != n or len(r) != n:
            raise ValueError(f"ViewPrep.prepare: {len(ims)} images and {len(r)} rectangles for the {n} views of the last bbox call")
        for i, im in enumerate(ims):
            if im.dtype != np.uint8 or im.shape != self._hw + (3,):
                raise ValueError(f"view {i}: images must be uint8 [H, W, 3] of the masks' size {self._hw}; got {im.dtype} {im.shape}")
        mv = np.zeros(n, np.int32) if mask_view is None else np.ascontiguousarray(np.asarray(mask_view).astype(np.int32))
        out = np.empty((n, L, L, 3), np.uint8)
        msk = np.zeros((n, L, L), np.uint8)
        sums = np.zeros(n, np.int64)
        _lib.check(self._lib.bf_views_prepare(self._h, n, _lib.iptr(r), _ptrs(ims), _lib.iptr(mv), _u8(out), _u8(msk),
                                              sums.ctypes.data_as(C.POINTER(C.c_int64))), "bf_views_prepare")
        return out, msk, sums

    def last_timing(self):
        """device time (ms) of the last calls: bbox (upload, kernels, download), prepare (upload, kernel, download); bytes moved: masks
        up, crops up, results down"""
        ms, by = np.zeros(6, np.float32), np.zeros(3, np.int64)
        _lib.check(self._lib.bf_views_last_timing(self._h, _lib.fptr(ms), by.ctypes.data_as(C.POINTER(C.c_int64))), "bf_views_last_timing")
        return ms, by


def _cams(annots):
    return annots["cams"] if "cams" in annots else annots


def prepare_frame(images, masks, annots, views, mask_frames, use_mask, L, prep=None, device=0):
    """get_data (genebody_fitting.py:111-142) on decoded views: images[i] uint8 [H, W, 3] and masks[i] uint8 [H, W] of views[i] ->
    (images, masks, Ks, Rts, use_frames, mask_frames) exactly as the reference returns them.  Camera i is the enumerate index over
    `views` (:119, :134), not the kept index.  `annots`: the annots.npy dict or its 'cams' entry.  `prep`: a ViewPrep of load size L
    (one is made on `device` when None)."""
    cams = _cams(annots)
    views = list(views)
    if len(images) != len(views) or len(masks) != len(views):
        raise ValueError(f"prepare_frame: {len(images)} images and {len(masks)} masks for {len(views)} views")
    if prep is None:
        prep = ViewPrep(device=device, L=L, max_views=len(views))
    if prep.L != L:
        raise ValueError(f"prepare_frame: the ViewPrep resizes to {prep.L}, not {L}")
    imgs, msks = [np.asarray(im) for im in images], [np.asarray(m) for m in masks]
    for v, im, m in zip(views, imgs, msks):
        if m.ndim != 2 or m.dtype != np.uint8:
            raise ValueError(f"view {v}: masks must be single-channel uint8 [H, W] ((msk > 128)[..., None] masks the image); got "
                             f"{m.dtype} {m.shape}")
        if im.dtype != np.uint8 or im.shape != m.shape + (3,):
            raise ValueError(f"view {v}: the image must be uint8 [H, W, 3] of its mask's size {m.shape}; got {im.dtype} {im.shape}")
    groups = {}
    for i, m in enumerate(msks):
        groups.setdefault(m.shape, []).append(i)
    crops, out_img, out_msk, sums = [None] * len(views), [None] * len(views), [None] * len(views), np.zeros(len(views), np.int64)
    for (H, W), idx in groups.items():
        box = prep.bbox([msks[i] for i in idx], names=[views[i] for i in idx])
        rects = []
        for k, i in enumerate(idx):
            crops[i] = crop_from_box(*box[k], H, W)
            rects.append(slice_rect(crops[i], H, W, f"view {views[i]}"))
        mv = [bool(use_mask) and views[i] in mask_frames for i in idx]
        o, om, s = prep.prepare(rects, [imgs[i] for i in idx], mv)
        for k, i in enumerate(idx):
            out_img[i], out_msk[i], sums[i] = o[k], om[k], s[k]
    Ks, Rts, use_frames, mask_frames_out, images_out, masks_out = [], [], [], [], [], []
    for i, view in enumerate(views):
        if sums[i] > 10 * L * L * 3:                          # np.mean(img) > 10 (:126): not a black frame
            top, left, bottom, right = crops[i]
            use_frames.append(view)
            images_out.append(out_img[i])
            if view in mask_frames and use_mask:
                masks_out.append(out_msk[i])
                mask_frames_out.append(view)
            K, Rt = cams["K"][i].copy(), cams["RT"][i].copy()
            K[0, 2] -= left
            K[1, 2] -= top
            K[0, :] *= L / float(right - left)
            K[1, :] *= L / float(bottom - top)
            Ks.append(K.astype(np.float32))
            Rts.append(Rt.astype(np.float32))
    return images_out, masks_out, Ks, Rts, use_frames, mask_frames_out


# ---------------------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------------------
def config_parser():
    """genebody_fitting.py:17-58, the same options and defaults; --device added.  Options the runner does not use are accepted and
    ignored, as the reference ignores them."""
    parser = argparse.ArgumentParser(prog="python -m bodyfitting_amd.genebody")
    parser.add_argument("--target_dir", type=str, default="/data/genebody", help='target directory storing obj data')
    parser.add_argument("--annot_dir", type=str, help='annot file contains camera parameter')
    parser.add_argument("--output_dir", type=str, default="./logs", help='directory contains output smpl and parameter')
    parser.add_argument("--openpose_dir", type=str, default="../openpose", help='directory of built openpose binary file (unused)')
    parser.add_argument("--info_dir", type=str, help='csv file which contains gender information')
    parser.add_argument('--debug', default=True, action='store_true', help='is output debug, false will speed up')
    parser.add_argument('--subject', type=str, default='zhuna', help='target subject to fit smpl')
    parser.add_argument('--load_size', default=512, type=int, help='load size of image data')
    parser.add_argument('--tasks', nargs='+', type=str, default=['openpose', 'smplify', 'output'], help='tasks to perform')
    parser.add_argument('--use_mask', default=False, action='store_true', help='smplify with human mask or not')
    parser.add_argument('--smpl_type', default="smpl", type=str, help='use smpl or smplx')
    parser.add_argument('--age', default="adult", type=str, help='use smpl or smil')
    parser.add_argument('--smplx_with_smpl_init', default=True, action='store_true',
                        help='if use smpl fitting result to initialize smplx fitting')
    parser.add_argument('--use_bodyscan', default=False, action='store_true', help='use body scan as 3D supervision or not')
    parser.add_argument('--viewnum', type=int, default=8, help='use multiview data')
    parser.add_argument('--smpl_uv_dir', type=str, default="./data/smpl_uv", help='folder to smpl uv')
    parser.add_argument('--white_bkgd', default=True, action='store_true', help='white bkgd')
    parser.add_argument('--device', default=0, type=int, help='HIP device to run on')
    return parser


def io_threads():
    """the decode / encode pool: OMP_NUM_THREADS (default 8), at most 16"""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "8"))
    except ValueError:
        n = 8
    return max(1, min(n, 16))


def read_image(path):
    """imageio.imread for the dataset's formats (imageio reads them through PIL)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


def write_png(path, img):
    from PIL import Image
    Image.fromarray(np.asarray(img)).save(path)


class Detection:
    """the `openpose` task on the GPU, shared by the GeneBody and RenderPeople runners: the estimators (`_openpose`, and
    `_openpose_hand` when `use_hand_face`) are made on `device` at the first call and kept for the run"""
    _openpose = _openpose_hand = None

    def detect_and_write(self, images, use_frames, wrt_dir):
        """openpose.bin --image_dir --write_json [--hand] on the GPU: view use_frames[i]'s image (RGB) flipped to BGR, as openpose.bin
        reads the PNG, detected, and written to wrt_dir/<view %02d>_keypoints.json"""
        from . import openpose as O
        if not images:
            return
        bgr = np.ascontiguousarray(np.stack([np.asarray(im)[:, :, ::-1] for im in images]))     # what openpose.bin reads from the PNG
        H, W = bgr.shape[1:3]
        if self._openpose is None:
            self._openpose = O.OpenPose(device=self.device, max_batch=4, max_h=max(H, 1024), max_w=max(W, 1024))
        if self.use_hand_face:
            from . import openpose_hand as OH
            if self._openpose_hand is None:
                self._openpose_hand = OH.OpenPoseHand(device=self.device, max_hands=16, max_h=max(H, 1024), max_w=max(W, 1024))
            people, write = OH.detect_people(self._openpose, self._openpose_hand, bgr), OH.write_json
        else:
            people, write = self._openpose.pose25(bgr), O.write_json
        for view, p in zip(use_frames, people):
            write(os.path.join(wrt_dir, '%02d_keypoints.json' % view), p)


class runner(Detection):
    """genebody_fitting.py:61-215 with the GPU stages.  `prep`: the view-preparation object (default a ViewPrep on --device)."""

    def __init__(self, args, prep=None):
        from .body_fitting import BodyFitting
        self.options = args
        self.subject = args.subject
        self.target_dir = os.path.join(args.target_dir, self.subject)
        self.output_dir = os.path.join(args.output_dir, self.subject)
        self.openpose_dir = args.openpose_dir
        self.use_mask = args.use_mask
        self.white_bkgd = args.white_bkgd
        self.annot_dir = os.path.join(args.annot_dir, self.subject + '.npy') if args.annot_dir is not None \
            else os.path.join(args.target_dir, 'annots.npy')
        self.smpl_type = args.smpl_type
        self.debug = args.debug
        self.use_hand_face = (self.smpl_type == 'smplx')
        self.load_size = args.load_size
        self.annots = np.load(self.annot_dir, allow_pickle=True).item()['cams']
        self.views = self.get_views()
        self.tasks = args.tasks
        # :78-83 fills self.gender before it exists (AttributeError); what it means: a csv of (subject, 0 = female / 1 = male)
        if self.options.info_dir is not None and os.path.exists(self.options.info_dir):
            self.genders = {}
            with open(self.options.info_dir, 'r') as info:
                reader = csv.reader(info)
                for row in reader:
                    self.genders[row[0]] = 'female' if int(row[1]) == 0 else 'male'
        self.gender = 'neutral' if not hasattr(self, 'genders') else self.genders[self.subject]
        self.bodyfitter = BodyFitting(self.options)
        self.seqs = self.get_sequence()
        self.mask_frames = list(MASK_FRAMES)
        self.device = int(getattr(args, "device", 0))
        self.prep = prep
        self._openpose = self._openpose_hand = None
        self._pool = None

    def get_views(self):
        # In GeneBody data, there exist some view missing in several sequences
        all_cameras_raw = list(range(48))
        if self.subject == 'Tichinah_jervier' or self.subject == 'dannier':
            all_cameras = list(set(all_cameras_raw) - set([32]))
        elif self.subject == 'wuwenyan':
            all_cameras = list(set(all_cameras_raw) - set([34, 36]))
        elif self.subject == 'joseph_matanda':
            all_cameras = list(set(all_cameras_raw) - set([39, 40, 42, 43, 44, 45, 46, 47]))
        else:
            all_cameras = all_cameras_raw
        return all_cameras

    def get_sequence(self):
        sequence_list = os.listdir(os.path.join(self.target_dir, 'image', '00'))
        sequence_list = [int(os.path.splitext(dir_)[0]) for dir_ in sequence_list]
        return sorted(sequence_list)

    def _map(self, fn, items):
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=io_threads())
        return list(self._pool.map(fn, items))

    def get_data(self, frame):
        img_dir = os.path.join(self.output_dir, '%06d' % frame, 'images')
        os.makedirs(img_dir, exist_ok=True)
        imgnames = sorted(os.listdir(os.path.join(self.target_dir, 'image', '00')))
        msknames = sorted(os.listdir(os.path.join(self.target_dir, 'mask', '00')))
        paths = []
        for view in self.views:                      # the frame number is a list index (:115-121)
            paths.append(os.path.join(self.target_dir, 'image', '{:02d}'.format(view), imgnames[frame]))
            paths.append(os.path.join(self.target_dir, 'mask', '{:02d}'.format(view), msknames[frame]))
        decoded = self._map(read_image, paths)
        if self.prep is None:
            self.prep = ViewPrep(device=self.device, L=self.load_size, max_views=len(self.views))
        data = prepare_frame(decoded[0::2], decoded[1::2], self.annots, self.views, self.mask_frames, self.use_mask,
                             self.load_size, prep=self.prep)
        images, use_frames = data[0], data[4]
        self._map(lambda a: write_png(*a), [(os.path.join(img_dir, '%02d.png' % v), im) for v, im in zip(use_frames, images)])
        return data

    def run_openpose(self, frame, data):
        """openpose.bin --image_dir images --write_json openpose [--hand] (:144-155) on the GPU, with the reference's skip test"""
        wrt_dir = os.path.abspath(os.path.join(self.output_dir, '%06d' % frame, 'openpose'))
        os.makedirs(wrt_dir, exist_ok=True)
        if len([dir_ for dir_ in os.listdir(wrt_dir) if '.json' in dir_]) >= len(data[0]):
            return
        self.detect_and_write(data[0], data[4], wrt_dir)

    def read_openpose(self, frame):
        from .io import load_openpose
        openpose_dir = os.path.join(self.output_dir, '%06d' % frame, 'openpose')
        views = sorted([dir_ for dir_ in os.listdir(openpose_dir) if '.json' in dir_])
        return [load_openpose(os.path.join(openpose_dir, view)) for view in views]

    def keyframe(self, use_frames):
        """:167's keyframe (view 25 when kept, else the first kept view) as the index BodyFitting reads images[] and c2ws[] at: the
        reference passes the view number itself, which is the same index while views 0-25 are all kept"""
        keyframe = 25 if 25 in use_frames else use_frames[0]
        return list(use_frames).index(keyframe)

    def run_smplify(self, frame, data, keypoints):
        images, masks, Ks, Rts, use_frames, mask_frames = data
        output_dir = os.path.join(self.output_dir, '%06d' % frame, 'smplify')
        return self.bodyfitter(images, Rts, Ks, keypoints, gender=self.gender, keyframe=self.keyframe(use_frames), use_frames=use_frames,
                               use_mask=self.use_mask, masks=masks, mask_frames=mask_frames, output_folder=output_dir)

    def run_output(self, frame):
        """:172-181 copies debug/ files BodyFitting never writes; this copies what it did write"""
        frame_dir = os.path.join(self.output_dir, '%06d' % frame)
        smpl_folder = os.path.join(self.output_dir, 'smpl')
        param_folder = os.path.join(self.output_dir, 'param')
        os.makedirs(smpl_folder, exist_ok=True)
        os.makedirs(param_folder, exist_ok=True)
        for src, dst in ((os.path.join(frame_dir, 'smplify', f'{self.smpl_type}.obj'), os.path.join(smpl_folder, '%04d.obj' % frame)),
                         (os.path.join(frame_dir, 'smplify', f'{self.smpl_type}_parameter.npy'), os.path.join(param_folder, '%04d.npy' % frame))):
            if os.path.exists(src):
                shutil.copyfile(src, dst)
            else:                                    # (the reference's cp fails and the run goes on)
                print(f"bodyfitting_amd.genebody: {src} does not exist, not copied", file=sys.stderr)

    def run(self):
        if self.debug:
            print("bodyfitting_amd.genebody: --debug outputs (OpenPose skeleton images, BodyFitting's smpl_fitting/ overlays) are not "
                  "produced", file=sys.stderr)
        for frame in self.seqs:
            data = self.get_data(frame)
            if 'openpose' in self.tasks:
                self.run_openpose(frame, data)
            keypoints = self.read_openpose(frame)
            if 'smplify' in self.tasks:
                self.run_smplify(frame, data, keypoints)
            if 'output' in self.tasks:
                self.run_output(frame)

    def close(self):
        for obj in (self.prep, self._openpose, self._openpose_hand):
            if obj is not None and hasattr(obj, "close"):
                obj.close()
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None


def main(argv=None):
    args = config_parser().parse_args(argv)
    r = runner(args)
    try:
        r.run()
    finally:
        r.close()


if __name__ == "__main__":
    main()
