"""The reference's OpenPose hand estimator (openpose/hand.py `Hand`, openpose/model.py `handpose_model`, openpose/util.py
`handDetect` / `npmax`) on the GPU, and the hand arrays of an `openpose.bin --hand` JSON.

The crops, the network, the map resizes, the scale accumulation, the Gaussian filter and the per-part component pick run in
`libbodyfit.so` (csrc/openpose_hand_kernels.hip, openpose_hand_api.hip).  Every hand of every view runs as one batch per scale: a
square handDetect box of side w is resized to rint(w * (m * 368 / w)) = 184 * 2m whatever w is, so the boxes of a frame share the
network size at each scale; boxes that do not (the `Hand` drop-in on arbitrary crops) are grouped by their padded size.

This module also holds the numpy restatements the kernels are held to: the hand's map pipeline (`accumulate_hand`), skimage's
8-connected labelling (`label8`), numpy's pairwise summation (`pairwise_sum`), and the whole of Hand.__call__'s post-processing
(`hand_postprocess`).

Weights: `hand_pose_model.pth` (caffe layer names, e.g. `conv1_1.weight`, `Mconv7_stage6.bias`: the keys util.transfer looks up
after stripping `model1_0.` / `model1_1.` / `modelN.`), read without torch by hmr.load_checkpoint, or a state dict registered with
`assets.register_openpose_hand(...)`.  They stay resident on the device in fp32.
"""
from __future__ import annotations

import collections
import math

import numpy as np

from . import _lib
from . import openpose as O

SCALE_SEARCH = (0.5, 1.0, 1.5, 2.0)                     # hand.py:27-31
BOXSIZE, STRIDE, PAD_VALUE, THRE = 368, 8, 128, 0.05
N_MAP, N_PART = 22, 21                                  # the network's maps; part 21 (background) is averaged, never picked
RATIO_WRIST_ELBOW = 0.33                                # util.py:130

# the network (model.py:143-217)
HAND_VGG = (("conv1_1", 3, 64, 3), ("conv1_2", 64, 64, 3), "pool", ("conv2_1", 64, 128, 3), ("conv2_2", 128, 128, 3), "pool",
            ("conv3_1", 128, 256, 3), ("conv3_2", 256, 256, 3), ("conv3_3", 256, 256, 3), ("conv3_4", 256, 256, 3), "pool",
            ("conv4_1", 256, 512, 3), ("conv4_2", 512, 512, 3), ("conv4_3", 512, 512, 3), ("conv4_4", 512, 512, 3),
            ("conv5_1", 512, 512, 3), ("conv5_2", 512, 512, 3), ("conv5_3_CPM", 512, 128, 3))
HAND_STAGE1 = (("conv6_1_CPM", 128, 512, 1), ("conv6_2_CPM", 512, N_MAP, 1))
HAND_STAGE_T = (("Mconv1_stage%d", 150, 128, 7), ("Mconv2_stage%d", 128, 128, 7), ("Mconv3_stage%d", 128, 128, 7),
                ("Mconv4_stage%d", 128, 128, 7), ("Mconv5_stage%d", 128, 128, 7), ("Mconv6_stage%d", 128, 128, 1),
                ("Mconv7_stage%d", 128, N_MAP, 1))
NO_RELU = ("conv6_2_CPM", "Mconv7_stage2", "Mconv7_stage3", "Mconv7_stage4", "Mconv7_stage5", "Mconv7_stage6")
# the 150-channel stage input torch.cat([out_prev, out1_0]) is held as out_prev 0:22 | 0 0 | out1_0 24:152 (16-byte aligned groups);
# input channel c of Mconv1 (torch order) sits at HCAT_POS[c]
HCAT_C = 152
HCAT_POS = np.concatenate([np.arange(N_MAP), 24 + np.arange(128)])


def hand_conv_shapes():
    """every convolution of handpose_model: caffe name -> (cout, cin, k)"""
    out = collections.OrderedDict()
    for v in HAND_VGG + HAND_STAGE1:
        if v != "pool":
            out[v[0]] = (v[2], v[1], v[3])
    for s in range(2, 7):
        for name, cin, cout, k in HAND_STAGE_T:
            out[name % s] = (cout, cin, k)
    return out


def expected_hand_keys():
    """the state-dict keys util.transfer reads (caffe names without the model1_0. / model1_1. / modelN. prefix) -> shape"""
    keys = collections.OrderedDict()
    for name, (cout, cin, k) in hand_conv_shapes().items():
        keys[name + ".weight"] = (cout, cin, k, k)
        keys[name + ".bias"] = (cout,)
    return keys


def match_hand_state(state, filename="hand_pose_model.pth"):
    """the state dict util.transfer builds, as float32 arrays; a missing or misshapen key raises ValueError naming it"""
    out = {}
    for key, shape in expected_hand_keys().items():
        if key not in state:
            raise ValueError(f"{filename}: missing key {key!r} (handpose_model needs every caffe layer of the hand model)")
        a = np.asarray(state[key], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{filename}: {key!r} has shape {a.shape}, handpose_model expects {shape}")
        out[key] = a
    return out


def load_hand_weights(path):
    """hand_pose_model.pth -> matched float32 state dict, without torch"""
    from .hmr import load_checkpoint
    return match_hand_state(load_checkpoint(path), path)


def pack_hand(state):
    """the matched state dict -> one float32 array in the order openpose_hand_api.hip walks the layers: the VGG front to
    conv5_3_CPM, conv6_1_CPM, conv6_2_CPM, then per stage 2 .. 6 Mconv1 on the padded 152-channel concat (HCAT_POS), Mconv2 .. 7"""
    parts = []
    for v in HAND_VGG + HAND_STAGE1:
        if v != "pool":
            parts += O._pack(state[v[0] + ".weight"], state[v[0] + ".bias"])
    for s in range(2, 7):
        parts += O._pack(state[f"Mconv1_stage{s}.weight"], state[f"Mconv1_stage{s}.bias"], HCAT_POS, HCAT_C)
        for j in range(2, 8):
            parts += O._pack(state[f"Mconv{j}_stage{s}.weight"], state[f"Mconv{j}_stage{s}.bias"])
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# util.handDetect
# ---------------------------------------------------------------------------------------------------------------------------------
def hand_detect(candidate, subset, H, W):
    """util.py:128-190 for an image of H x W: [[x, y, w, is_left]] per person of subset, left box first, in Python doubles"""
    out = []
    candidate = np.asarray(candidate, np.float64).reshape(-1, 4) if len(candidate) else np.zeros((0, 4))
    for person in np.asarray(subset).astype(int).reshape(-1, 20):
        has_left = np.sum(person[[5, 6, 7]] == -1) == 0
        has_right = np.sum(person[[2, 3, 4]] == -1) == 0
        hands = []
        if has_left:
            hands.append([float(v) for i in person[[5, 6, 7]] for v in candidate[i][:2]] + [True])
        if has_right:
            hands.append([float(v) for i in person[[2, 3, 4]] for v in candidate[i][:2]] + [False])
        for x1, y1, x2, y2, x3, y3, is_left in hands:
            x = x3 + RATIO_WRIST_ELBOW * (x3 - x2)
            y = y3 + RATIO_WRIST_ELBOW * (y3 - y2)
            d_we = math.sqrt((x3 - x2) ** 2 + (y3 - y2) ** 2)
            d_es = math.sqrt((x2 - x1) ** 2 + (y2 - y1) ** 2)
            width = 1.5 * max(d_we, 0.9 * d_es)
            x -= width / 2
            y -= width / 2
            if x < 0:
                x = 0
            if y < 0:
                y = 0
            w1 = w2 = width
            if x + width > W:
                w1 = W - x
            if y + width > H:
                w2 = H - y
            width = min(w1, w2)
            if width >= 20:
                out.append([int(x), int(y), int(width), is_left])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Hand.__call__'s maps (hand.py:26-56)
# ---------------------------------------------------------------------------------------------------------------------------------
def hand_scales(bh):
    return [m * BOXSIZE / bh for m in SCALE_SEARCH]


def hand_scale_dims(bh, bw):
    """per scale for a crop of bh x bw: (resized h, w, padded h, w)"""
    out = []
    for s in hand_scales(bh):
        h, w = O.scaled_size(bh, s), O.scaled_size(bw, s)
        out.append((h, w, -(-h // STRIDE) * STRIDE, -(-w // STRIDE) * STRIDE))
    return out


def preprocess_crop(crop, scale):
    """hand.py:35-38 for one scale: the padded network input [Hp, Wp, 3] float32 of a uint8 BGR crop"""
    return O.preprocess(np.ascontiguousarray(crop), scale)


def output_to_heat(out, rh, rw, bh, bw):
    """one scale's network output [Hp/8, Wp/8, 22] -> the float32 heatmap [bh, bw, 22] (hand.py:48-52)"""
    out = np.asarray(out, np.float32)
    up = O.resize_cubic_f32(out, out.shape[0] * STRIDE, out.shape[1] * STRIDE, float(STRIDE), float(STRIDE))[:rh, :rw]
    return O.resize_cubic_f32(up, bh, bw, bh / rh, bw / rw)


def accumulate_hand(outputs, bh, bw):
    """per-scale outputs of one crop -> heatmap_avg float64 [bh, bw, 22] (heatmap_avg += heatmap / 4, the quotient in float32)"""
    avg = np.zeros((bh, bw, N_MAP))
    for out, (h, w, _, _) in zip(outputs, hand_scale_dims(bh, bw)):
        avg += output_to_heat(out, h, w, bh, bw) / len(SCALE_SEARCH)
    return avg


# ---------------------------------------------------------------------------------------------------------------------------------
# the component pick (hand.py:58-75)
# ---------------------------------------------------------------------------------------------------------------------------------
def label8(binary):
    """skimage.measure.label(binary, connectivity=2, return_num=True): 8-connected components numbered 1.. by the raster order of
    their first pixel.  Restated as the kernel labels: every pixel ends at its component's smallest raster index (its root), and a
    label is 1 + the rank of its root."""
    b = np.asarray(binary, bool)
    H, W = b.shape
    big = H * W
    lab = np.where(b, np.arange(big).reshape(H, W), big)
    pad = np.full((H + 2, W + 2), big)
    while True:
        pad[1:-1, 1:-1] = lab
        m = lab.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m = np.minimum(m, pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        m = np.where(b, m, big)
        flat = np.append(m.reshape(-1), big)
        while True:                                  # pointer jumping: a root's index is its own label
            j = flat[flat]
            if (j == flat).all():
                break
            flat = j
        m = flat[:-1].reshape(H, W)
        if (m == lab).all():
            break
        lab = m
    roots = np.unique(lab[b])
    out = np.zeros((H, W), np.int64)
    out[b] = np.searchsorted(roots, lab[b]) + 1
    return out, len(roots)


def _pairwise(a, lo, n):
    if n < 8:
        r = -0.0
        for i in range(n):
            r += float(a[lo + i])
        return r
    if n <= 128:
        r = a[lo:lo + 8].copy()
        i = 8
        while i < n - n % 8:
            r += a[lo + i:lo + i + 8]
            i += 8
        res = float(((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])))
        while i < n:
            res += float(a[lo + i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a, lo, n2) + _pairwise(a, lo + n2, n - n2)


def pairwise_sum(a):
    """np.sum of a contiguous float64 vector as numpy computes it: pairwise summation (8 partial sums up to 128 elements, halves
    rounded down to multiples of 8 above that) within 8,192-element buffers, the buffer sums added in sequence"""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    s = -0.0
    for b in range(0, len(a), 8192):
        s = s + _pairwise(a, b, min(8192, len(a) - b))
    return s


def npmax(array):
    """util.npmax: (row, column) of the first raster occurrence of the maximum"""
    idx = array.argmax(1)
    i = array.max(1).argmax()
    return int(i), int(idx[i])


def hand_postprocess(heat_avg):
    """hand.py:58-76 on one crop's heatmap_avg float64 [h, w, 22] -> (peaks int64 [21, 2] = (x, y), scores [21] = the zeroed map at
    the peak, found bool [21] = the thresholded map was not empty)"""
    peaks, scores, found = np.zeros((N_PART, 2), np.int64), np.zeros(N_PART), np.zeros(N_PART, bool)
    for part in range(N_PART):
        map_ori = np.array(heat_avg[:, :, part], np.float64)
        binary = O.gaussian_filter(map_ori) > THRE
        if not binary.any():
            continue
        lab, num = label8(binary)
        best = int(np.argmax([np.sum(map_ori[lab == i]) for i in range(1, num + 1)])) + 1
        map_ori[lab != best] = 0
        y, x = npmax(map_ori)
        peaks[part], scores[part], found[part] = (x, y), map_ori[y, x], True
    return peaks, scores, found


# ---------------------------------------------------------------------------------------------------------------------------------
# the JSON layout (openpose.bin --hand): hand_left / hand_right [21, 3] in image coordinates
# ---------------------------------------------------------------------------------------------------------------------------------
def hand_array(box, peaks, scores, found):
    """one hand's [21, 3] (x, y, confidence) in image coordinates: crop peak + box corner, the heatmap peak as confidence, and
    (0, 0, 0) for a part whose thresholded map was empty"""
    a = np.zeros((N_PART, 3))
    f = np.asarray(found, bool)
    a[f, 0] = peaks[f, 0] + box[0]
    a[f, 1] = peaks[f, 1] + box[1]
    a[f, 2] = scores[f]
    return a


def select_person_entry(people):
    """io.load_openpose(only_one=True) on a view's people given as dicts of [n, 3] arrays (pose / hand_left / hand_right): arrays
    whose confidences are all <= 0 are dropped as the reader drops them, and the person whose summed confidences over all its
    arrays are strictly largest is kept, starting from entry 0 at score 0; None without people or when the kept entry is empty.
    (A kept person whose pose was dropped gets a zero pose - confidence 0, as the fit treats a missing part.)"""
    if not people:
        return None
    kept = [{k: np.asarray(v, np.float64) for k, v in p.items() if np.abs(np.asarray(v)[:, -1]).max() > 0} for p in people]
    best, best_score = 0, 0
    for i, e in enumerate(kept):
        s = sum(a[:, -1].sum() for a in e.values())
        if s > best_score:
            best, best_score = i, s
    entry = kept[best]
    if not entry:
        return None
    entry.setdefault("pose", np.zeros((25, 3)))
    return entry


def write_json(path, people):
    """openpose.write_json with optional hands: each person a dict {'pose': [25, 3], 'hand_left': [21, 3], 'hand_right': [21, 3]}
    (missing hands omitted)"""
    import json
    keys = (("pose", "pose_keypoints_2d"), ("hand_left", "hand_left_keypoints_2d"), ("hand_right", "hand_right_keypoints_2d"))
    doc = {"version": 1.3, "people": []}
    for p in people:
        q = {"person_id": [-1]}
        for k, name in keys:
            if k in p:
                q[name] = np.asarray(p[k]).flatten().tolist()
        doc["people"].append(q)
    with open(path, "w") as f:
        f.write(json.dumps(doc))


# ---------------------------------------------------------------------------------------------------------------------------------
# the device estimator
# ---------------------------------------------------------------------------------------------------------------------------------
def _boxes(boxes):
    b = np.ascontiguousarray(np.asarray(boxes, np.int64).reshape(-1, 5).astype(np.int32))
    return b


class OpenPoseHand:
    """OpenPoseHand(weights=None, device=0, max_hands=16, max_h=1024, max_w=1024): the hand estimator with its weights resident.
    `weights`: a state dict in the caffe-key layout, a path to hand_pose_model.pth, or None for `assets.get_openpose_hand()`.
    Views are uint8 BGR [H, W, 3] of one size (at most max_h x max_w); a box is (view, x, y, w, h) inside its view, and the crop
    img[y:y+h, x:x+w] is the reference's oriImg.  Up to max_hands crops of one network size run as one batch."""

    def __init__(self, weights=None, device=0, max_hands=16, max_h=1024, max_w=1024):
        import ctypes as C
        if weights is None:
            from . import assets
            packed = assets.get_openpose_hand()
        elif isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            packed = pack_hand(load_hand_weights(weights))
        else:
            packed = pack_hand(match_hand_state(weights))
        self._lib = _lib.load()
        n = int(self._lib.bf_openpose_hand_n_weights())
        if packed.size != n:
            raise ValueError(f"{packed.size} packed OpenPose hand weights, the network has {n}")
        self.device, self.max_hands, self.max_h, self.max_w = int(device), int(max_hands), int(max_h), int(max_w)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_openpose_hand_create(self.device, _lib.fptr(packed), n, self.max_hands, self.max_h, self.max_w,
                                                     C.byref(self._h)), "bf_openpose_hand_create")
        self._resident = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bf_openpose_hand_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _views(views):
        if isinstance(views, np.ndarray) and views.ndim == 3:
            views = [views]
        imgs = [O.check_image(v) for v in views]
        if len({v.shape for v in imgs}) != 1:
            raise ValueError("OpenPoseHand: one call takes views of one size")
        return np.ascontiguousarray(np.stack(imgs))

    def maps(self, views, boxes):
        """-> per box heatmap_avg float64 [h, w, 22] (hand.py:56); the maps stay resident for peaks()"""
        a, b = self._views(views), _boxes(boxes)
        heat = np.zeros(int(sum(int(h) * int(w) for _, _, _, w, h in b)) * N_MAP)
        _lib.check(self._lib.bf_openpose_hand_maps(self._h, a.shape[0], a.shape[1], a.shape[2], O.OpenPose._u8(a), len(b),
                                                   _lib.iptr(b), O._dptr(heat)), "bf_openpose_hand_maps")
        self._resident = b
        return self._split(heat, b)

    @staticmethod
    def _split(flat, b, c=N_MAP):
        out, at = [], 0
        for _, _, _, w, h in b:
            k = int(h) * int(w) * c
            out.append(flat[at:at + k].reshape(int(h), int(w), c))
            at += k
        return out

    def network(self, views, boxes):
        """per scale a list (one per box) of the network outputs float32 [Hp/8, Wp/8, 22], and of the inputs float32 [Hp, Wp, 3]"""
        a, b = self._views(views), _boxes(boxes)
        dims = [hand_scale_dims(int(h), int(w)) for _, _, _, w, h in b]
        n_out = sum(d[2] // 8 * (d[3] // 8) * N_MAP for dd in dims for d in dd)
        n_in = sum(d[2] * d[3] * 4 for dd in dims for d in dd)
        o, i = np.zeros(n_out, np.float32), np.zeros(n_in, np.float32)
        _lib.check(self._lib.bf_openpose_hand_network(self._h, a.shape[0], a.shape[1], a.shape[2], O.OpenPose._u8(a), len(b),
                                                      _lib.iptr(b), _lib.fptr(i), _lib.fptr(o)), "bf_openpose_hand_network")
        self._resident = b
        outs, ins, ao, ai = [], [], 0, 0
        for m in range(len(SCALE_SEARCH)):
            so, si = [], []
            for d in dims:
                hq, wq = d[m][2] // 8, d[m][3] // 8
                so.append(o[ao:ao + hq * wq * N_MAP].reshape(hq, wq, N_MAP))
                ao += hq * wq * N_MAP
                si.append(i[ai:ai + d[m][2] * d[m][3] * 4].reshape(d[m][2], d[m][3], 4)[..., :3])
                ai += d[m][2] * d[m][3] * 4
            outs.append(so)
            ins.append(si)
        return outs, ins

    def inject(self, outputs, boxes):
        """the maps from injected network outputs (per scale a list, one per box, of float32 [Hp/8, Wp/8, 22]); only the boxes'
        sizes are used.  The maps stay resident for peaks(); -> per box heatmap_avg float64 [h, w, 22]"""
        b = _boxes(boxes)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).reshape(-1) for sc in outputs for o in sc]))
        heat = np.zeros(int(sum(int(h) * int(w) for _, _, _, w, h in b)) * N_MAP)
        _lib.check(self._lib.bf_openpose_hand_inject(self._h, len(b), _lib.iptr(b), _lib.fptr(flat), int(flat.size), O._dptr(heat)),
                   "bf_openpose_hand_inject")
        self._resident = b
        return self._split(heat, b)

    def peaks(self, blurred=False):
        """on the resident maps: per box (peaks int64 [21, 2] = (x, y) in crop coordinates, scores [21], found bool [21]) as
        hand_postprocess gives them; with blurred, also the filtered maps float64 [h, w, 21] per box"""
        b = self._resident
        if b is None:
            raise ValueError("OpenPoseHand.peaks: no resident maps (call maps() or inject() first)")
        n = len(b)
        pk = np.zeros((n, N_PART, 2), np.int32)
        sc = np.zeros((n, N_PART))
        fd = np.zeros((n, N_PART), np.int32)
        bl = np.zeros(int(sum(int(h) * int(w) for _, _, _, w, h in b)) * N_PART) if blurred else None
        if n:
            _lib.check(self._lib.bf_openpose_hand_peaks(self._h, n, O._dptr(bl), _lib.iptr(pk), O._dptr(sc), _lib.iptr(fd)),
                       "bf_openpose_hand_peaks")
        res = [(pk[i].astype(np.int64), sc[i], fd[i].astype(bool)) for i in range(n)]
        return (res, self._split(bl, b, N_PART)) if blurred else res

    def detect(self, bgr_views, boxes):
        """Hand.__call__ on every box: per box (peaks [21, 2] int64, scores [21], found [21])"""
        a, b = self._views(bgr_views), _boxes(boxes)
        if len(b) == 0:
            return []
        _lib.check(self._lib.bf_openpose_hand_maps(self._h, a.shape[0], a.shape[1], a.shape[2], O.OpenPose._u8(a), len(b),
                                                   _lib.iptr(b), None), "bf_openpose_hand_maps")
        self._resident = b
        return self.peaks()


def detect_people(body, hand, bgr_views):
    """per view the people of an `openpose.bin --hand` run: dicts {'pose': BODY_25 [25, 3], 'hand_left' / 'hand_right': [21, 3]}
    (a hand only where handDetect accepts its box).  body: openpose.OpenPose, hand: OpenPoseHand; one hand call for the frame."""
    a = np.ascontiguousarray(np.stack([O.check_image(v) for v in bgr_views]))
    H, W = a.shape[1:3]
    found = body.detect_many(a)
    boxes, owner = [], []
    people = []
    for v, (cand, subset) in enumerate(found):
        persons = [{"pose": p} for p in O.pose25(cand, subset)]
        people.append(persons)
        for pi, person in enumerate(np.asarray(subset).reshape(-1, 20)):
            for x, y, w, is_left in hand_detect(cand, person[None], H, W):
                boxes.append((v, x, y, w, w))
                owner.append((v, pi, "hand_left" if is_left else "hand_right"))
    if boxes:
        for (v, pi, key), box, (pk, sc, fd) in zip(owner, boxes, hand.detect(a, boxes)):
            people[v][pi][key] = hand_array(box[1:3], pk, sc, fd)
    return people
