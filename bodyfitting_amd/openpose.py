"""The reference's OpenPose body estimator (openpose/body.py `Body`, openpose/model.py `bodypose_model`: the CMU COCO-18 body CPM of
pytorch-openpose) on the GPU, and the BODY_25-layout JSON of openpose/infer_openpose.py.

The network, the map resizes, the scale accumulation, the Gaussian peak filter and the limb scoring run in `libbodyfit.so`
(csrc/openpose_kernels.hip, openpose_api.hip).  The greedy connection pick and the subset assembly (body.py:175-238) stay on the
host in numpy: they are branchy and touch a few dozen peaks.

This module also holds the numpy restatements the kernels are held to bit for bit - cv2.resize INTER_CUBIC on uint8 (OpenCV's
11-bit fixed-point path) and on float32 maps, scipy.ndimage.gaussian_filter(sigma=3) - and the whole of Body.__call__'s
post-processing (`postprocess`), which tools/gen_openpose_golden.py also installs as the `cv2.resize` the unmodified reference
calls.

Weights: `body_pose_model.pth` (caffe layer names, e.g. `conv1_1.weight`, `Mconv7_stage6_L2.bias`: the keys util.transfer looks
up after stripping `model0.` / `modelN_M.`), read without torch by hmr.load_checkpoint, or a state dict registered with
`assets.register_openpose(...)`.  They stay resident on the device in fp32.
"""
from __future__ import annotations

import collections
import json
import math
import sys

import numpy as np

from . import _lib

BOXSIZE, STRIDE, PAD_VALUE = 368, 8, 128                 # body.py:62-65
SCALE_SEARCH = (0.5, 1.0, 1.5, 2.0)
THRE1, THRE2, MID_NUM = 0.1, 0.05, 100
N_HEAT, N_PAF, N_OUT = 19, 38, 57                       # the network's per-pixel output: paf 0:38, heat 38:57
LIMB_SEQ = ((2, 3), (2, 6), (3, 4), (4, 5), (6, 7), (7, 8), (2, 9), (9, 10), (10, 11), (2, 12), (12, 13), (13, 14), (2, 1), (1, 15),
            (15, 17), (1, 16), (16, 18), (3, 17), (6, 18))
MAP_IDX = ((31, 32), (39, 40), (33, 34), (35, 36), (41, 42), (43, 44), (19, 20), (21, 22), (23, 24), (25, 26), (27, 28), (29, 30),
           (47, 48), (49, 50), (53, 54), (51, 52), (55, 56), (37, 38), (45, 46))
COCO17_FROM_18 = (0, 15, 14, 17, 16, 5, 2, 6, 3, 7, 4, 11, 8, 12, 9, 13, 10)        # infer_openpose.py:26
BODY25_FROM_17 = (0, 16, 15, 18, 17, 5, 2, 6, 3, 7, 4, 12, 9, 13, 10, 14, 11)       # infer_openpose.py:69
PEAK_CAP = 8192                                          # peaks per view the device list holds

# ---------------------------------------------------------------------------------------------------------------------------------
# the network (model.py:24-124)
# ---------------------------------------------------------------------------------------------------------------------------------
VGG = (("conv1_1", 3, 64, 3), ("conv1_2", 64, 64, 3), "pool", ("conv2_1", 64, 128, 3), ("conv2_2", 128, 128, 3), "pool",
       ("conv3_1", 128, 256, 3), ("conv3_2", 256, 256, 3), ("conv3_3", 256, 256, 3), ("conv3_4", 256, 256, 3), "pool",
       ("conv4_1", 256, 512, 3), ("conv4_2", 512, 512, 3), ("conv4_3_CPM", 512, 256, 3), ("conv4_4_CPM", 256, 128, 3))
STAGE1 = (("conv5_1_CPM", 128, 128, 3), ("conv5_2_CPM", 128, 128, 3), ("conv5_3_CPM", 128, 128, 3), ("conv5_4_CPM", 128, 512, 1))
STAGE_T = (("Mconv1_stage%d", 185, 128, 7), ("Mconv2_stage%d", 128, 128, 7), ("Mconv3_stage%d", 128, 128, 7),
           ("Mconv4_stage%d", 128, 128, 7), ("Mconv5_stage%d", 128, 128, 7), ("Mconv6_stage%d", 128, 128, 1))
BRANCH_OUT = {"L1": N_PAF, "L2": N_HEAT}
# the 192-channel stage input torch.cat([L1, L2, out1]) is held as out1 | L1 | 0 0 | L2 | 0 x 5 (16-byte aligned groups);
# input channel c of Mconv1 (185 of them, torch order) sits at CAT_POS[c]
CAT_C = 192
CAT_POS = np.concatenate([128 + np.arange(38), 168 + np.arange(19), np.arange(128)])


def conv_shapes():
    """every convolution of bodypose_model: caffe name -> (cout, cin, k)"""
    out = collections.OrderedDict()
    for v in VGG:
        if v != "pool":
            out[v[0]] = (v[2], v[1], v[3])
    for br in ("L1", "L2"):
        for name, cin, cout, k in STAGE1:
            out[f"{name}_{br}"] = (cout, cin, k)
        out[f"conv5_5_CPM_{br}"] = (BRANCH_OUT[br], 512, 1)
    for s in range(2, 7):
        for br in ("L1", "L2"):
            for name, cin, cout, k in STAGE_T:
                out[(name % s) + "_" + br] = (cout, cin, k)
            out[f"Mconv7_stage{s}_{br}"] = (BRANCH_OUT[br], 128, 1)
    return out


def expected_keys():
    """the state-dict keys util.transfer reads (caffe names without the model0. / modelN_M. prefix) -> shape"""
    keys = collections.OrderedDict()
    for name, (cout, cin, k) in conv_shapes().items():
        keys[name + ".weight"] = (cout, cin, k, k)
        keys[name + ".bias"] = (cout,)
    return keys


def match_state(state, filename="body_pose_model.pth"):
    """the state dict util.transfer builds, as float32 arrays; a missing or misshapen key raises ValueError naming it (the reference
    raises KeyError from util.transfer, or a size mismatch from load_state_dict)"""
    out = {}
    for key, shape in expected_keys().items():
        if key not in state:
            raise ValueError(f"{filename}: missing key {key!r} (bodypose_model needs every caffe layer of the COCO body model)")
        a = np.asarray(state[key], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{filename}: {key!r} has shape {a.shape}, bodypose_model expects {shape}")
        out[key] = a
    return out


def load_weights(path):
    """body_pose_model.pth -> matched float32 state dict, without torch"""
    from .hmr import load_checkpoint
    return match_state(load_checkpoint(path), path)


def _pack(w, b, perm=None, cin_pad=None):
    """torch [cout][cin][k][k] -> [k*k*cin_pad][cout_pad] in (ky, kx, ci) order, then the bias [cout_pad]; cin_pad / cout_pad are
    multiples of 4, the padding is zero.  perm: the padded channel position of each input channel."""
    cout, cin, k, _ = w.shape
    cp = cin_pad or -(-cin // 4) * 4
    co = -(-cout // 4) * 4
    wt = np.zeros((k, k, cp, co), np.float32)
    pos = np.arange(cin) if perm is None else perm
    wt[:, :, pos, :cout] = w.transpose(2, 3, 1, 0)
    bb = np.zeros(co, np.float32)
    bb[:cout] = b
    return [wt.reshape(-1), bb]


def pack(state):
    """the matched state dict -> one float32 array in the order openpose_api.hip walks the layers: the VGG front; stage 1's
    conv5_1 as one 128 -> 256 layer (L1 outputs 0:128, L2 128:256); conv5_2..5_5 L1 then L2; per later stage Mconv1 as one
    192 -> 256 layer on the padded concat (CAT_POS), then Mconv2..7 L1 then L2"""
    parts = []
    for v in VGG:
        if v != "pool":
            parts += _pack(state[v[0] + ".weight"], state[v[0] + ".bias"])

    def merged(a, b, perm=None, cin_pad=None):
        w = np.concatenate([state[a + ".weight"], state[b + ".weight"]])
        return _pack(w, np.concatenate([state[a + ".bias"], state[b + ".bias"]]), perm, cin_pad)

    parts += merged("conv5_1_CPM_L1", "conv5_1_CPM_L2")
    for name in ("conv5_2_CPM", "conv5_3_CPM", "conv5_4_CPM", "conv5_5_CPM"):
        for br in ("L1", "L2"):
            parts += _pack(state[f"{name}_{br}.weight"], state[f"{name}_{br}.bias"])
    for s in range(2, 7):
        parts += merged(f"Mconv1_stage{s}_L1", f"Mconv1_stage{s}_L2", CAT_POS, CAT_C)
        for j in range(2, 8):
            for br in ("L1", "L2"):
                parts += _pack(state[f"Mconv{j}_stage{s}_{br}.weight"], state[f"Mconv{j}_stage{s}_{br}.bias"])
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# cv2.resize(..., INTER_CUBIC) restatements (the kernel's: csrc/openpose_kernels.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def scaled_size(n, scale):
    """saturate_cast<int>(n * scale): round half to even"""
    return int(np.rint(np.float64(n) * np.float64(scale)))


def cubic_coeffs(f):
    """interpolateCubic(x, coeffs) with A = -0.75, in float32, for a float32 array of fractions"""
    A, one = np.float32(-0.75), np.float32(1)
    x = np.asarray(f, np.float32)
    x1 = x + one
    c0 = ((A * x1 - np.float32(5) * A) * x1 + np.float32(8) * A) * x1 - np.float32(4) * A
    c1 = ((A + np.float32(2)) * x - (A + np.float32(3))) * x * x + one
    y = one - x
    c2 = ((A + np.float32(2)) * y - (A + np.float32(3))) * y * y + one
    c3 = one - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], -1).astype(np.float32)


def cubic_axis(n_dst, scale, n_src):
    """per destination index: the four clamped source indices and the float32 coefficients.  fx = (float)((d + 0.5) * scale - 0.5)
    in double, floored; taps sx - 1 .. sx + 2 replicate the border (HResizeCubic / the row clamp)"""
    f = ((np.arange(n_dst) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    idx = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    return idx, cubic_coeffs(f)


def resize_cubic_u8(image, scale):
    """cv2.resize(image, (0, 0), fx=scale, fy=scale, interpolation=cv2.INTER_CUBIC) on uint8 [H, W, C]: OpenCV's fixed-point path -
    coefficients saturate_cast<short>(c * 2048), an int horizontal sum per row, then (sum_k S_k * b_k + 2^21) >> 22 saturated"""
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError("resize_cubic_u8 takes uint8 images")
    H, W = img.shape[:2]
    Ho, Wo = scaled_size(H, scale), scaled_size(W, scale)
    inv = 1.0 / float(scale)
    xi, xa = cubic_axis(Wo, inv, W)
    yi, ya = cubic_axis(Ho, inv, H)
    xa, ya = np.rint(xa * np.float32(2048)).astype(np.int64), np.rint(ya * np.float32(2048)).astype(np.int64)
    src = img.astype(np.int64)
    h = sum(src[:, xi[:, j]] * xa[None, :, j, None] for j in range(4))         # [H, Wo, C]
    v = sum(h[yi[:, j]] * ya[:, j, None, None] for j in range(4))              # [Ho, Wo, C]
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_cubic_f32(img, dst_h, dst_w, inv_scale_y, inv_scale_x):
    """cv2.resize INTER_CUBIC on float32 [H, W, C] to (dst_h, dst_w) with cv2's inverse scales (fx / fy, or dsize / ssize):
    horizontal D = ((S0 a0 + S1 a1) + S2 a2) + S3 a3 per row, then the same over four rows, every step rounded to float32"""
    img = np.asarray(img, np.float32)
    H, W = img.shape[:2]
    xi, xa = cubic_axis(dst_w, 1.0 / inv_scale_x, W)
    yi, ya = cubic_axis(dst_h, 1.0 / inv_scale_y, H)
    h = img[:, xi[:, 0]] * xa[None, :, 0, None]
    for j in range(1, 4):
        h = h + img[:, xi[:, j]] * xa[None, :, j, None]
    v = h[yi[:, 0]] * ya[:, 0, None, None]
    for j in range(1, 4):
        v = v + h[yi[:, j]] * ya[:, j, None, None]
    return v.astype(np.float32)


def cv2_resize(src, dsize, fx=None, fy=None, interpolation=None):
    """the cv2.resize calls of body.py (INTER_CUBIC, uint8 images and float32 maps) - the stub tools/gen_openpose_golden.py hands
    the reference"""
    src = np.asarray(src)
    H, W = src.shape[:2]
    if dsize is None or tuple(dsize) == (0, 0):
        Ho, Wo, iy, ix = scaled_size(H, fy), scaled_size(W, fx), float(fy), float(fx)
    else:
        Wo, Ho = int(dsize[0]), int(dsize[1])
        iy, ix = Ho / H, Wo / W
    if src.dtype == np.uint8:
        if (Ho, Wo) != (scaled_size(H, fy), scaled_size(W, fx)) or fx != fy:
            raise NotImplementedError("uint8 resize: body.py uses fx == fy only")
        return resize_cubic_u8(src, fx)
    return resize_cubic_f32(src, Ho, Wo, iy, ix)


def scales(H):
    """body.py:67 multipliers for an image of height H"""
    return [x * BOXSIZE / H for x in SCALE_SEARCH]


def scale_dims(H, W):
    """per scale: (resized h, w, padded h, w) (util.padRightDownCorner to a multiple of 8)"""
    out = []
    for s in scales(H):
        h, w = scaled_size(H, s), scaled_size(W, s)
        out.append((h, w, -(-h // STRIDE) * STRIDE, -(-w // STRIDE) * STRIDE))
    return out


def preprocess(bgr, scale):
    """body.py:73-75 for one scale: the padded network input [Hp, Wp, 3] float32 (/256 - 0.5)"""
    r = resize_cubic_u8(bgr, scale)
    h, w = r.shape[:2]
    Hp, Wp = -(-h // STRIDE) * STRIDE, -(-w // STRIDE) * STRIDE
    pad = np.full((Hp, Wp, 3), PAD_VALUE, np.uint8)
    pad[:h, :w] = r
    return pad.astype(np.float32) / np.float32(256) - np.float32(0.5)


def output_to_maps(out, h, w, H, W):
    """one scale's network output [Hp/8, Wp/8, 57] (paf 0:38, heat 38:57) -> (heat, paf) float32 [H, W, c] as body.py:90-99"""
    out = np.asarray(out, np.float32)
    up = resize_cubic_f32(out, out.shape[0] * STRIDE, out.shape[1] * STRIDE, float(STRIDE), float(STRIDE))[:h, :w]
    m = resize_cubic_f32(up, H, W, H / h, W / w)
    return m[..., N_PAF:], m[..., :N_PAF]


def accumulate(outputs, H, W):
    """per-scale outputs -> (heatmap_avg, paf_avg) float64 with body.py:101-102's operation order (heatmap_avg += heatmap_avg + heatmap / 4)"""
    heat_avg, paf_avg = np.zeros((H, W, N_HEAT)), np.zeros((H, W, N_PAF))
    n = len(SCALE_SEARCH)
    for out, (h, w, _, _) in zip(outputs, scale_dims(H, W)):
        heat, paf = output_to_maps(out, h, w, H, W)
        heat_avg += heat_avg + heat / n
        paf_avg += + paf / n
    return heat_avg, paf_avg


# ---------------------------------------------------------------------------------------------------------------------------------
# scipy.ndimage.gaussian_filter(sigma=3) and the peaks
# ---------------------------------------------------------------------------------------------------------------------------------
GAUSS_RADIUS = 12


def gaussian_weights(sigma=3.0):
    """scipy.ndimage._gaussian_kernel1d(sigma, 0, radius), radius = int(4 * sigma + 0.5); symmetric, so its reverse is itself"""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum()


def _reflect(i, n):
    i = np.asarray(i)
    period = 2 * n
    i = np.mod(i, period)
    return np.where(i >= n, period - 1 - i, i)


def _correlate_sym(a, w, axis):
    """NI_Correlate1D's symmetric branch: out = x[i] * w0, then out += (x[i - j] + x[i + j]) * w_j for j = r .. 1; mode 'reflect'"""
    r = (len(w) - 1) // 2
    n = a.shape[axis]
    idx = np.arange(n)
    take = lambda off: np.take(a, _reflect(idx + off, n), axis=axis)
    out = a * w[r]
    for j in range(-r, 0):
        out = out + (take(j) + take(-j)) * w[r + j]
    return out


def gaussian_filter(a, sigma=3.0):
    """scipy.ndimage.gaussian_filter(a, sigma) on a float64 2-D array (or [..., H, W] stacks along the last two axes), bit for bit"""
    w = gaussian_weights(sigma)
    a = np.asarray(a, np.float64)
    return _correlate_sym(_correlate_sym(a, w, a.ndim - 2), w, a.ndim - 1)


def find_peaks(heat_avg):
    """body.py:104-128 -> all_peaks: per part a list of (x, y, score, id)"""
    all_peaks, counter = [], 0
    blurred = gaussian_filter(np.moveaxis(heat_avg[:, :, :18], 2, 0))
    for part in range(18):
        one = blurred[part]
        left, right, up, down = (np.zeros(one.shape) for _ in range(4))
        left[1:, :], right[:-1, :], up[:, 1:], down[:, :-1] = one[:-1, :], one[1:, :], one[:, :-1], one[:, 1:]
        binary = np.logical_and.reduce((one >= left, one >= right, one >= up, one >= down, one > THRE1))
        ys, xs = np.nonzero(binary)
        peaks = [(int(x), int(y), float(heat_avg[y, x, part]), counter + i) for i, (x, y) in enumerate(zip(xs, ys))]
        all_peaks.append(peaks)
        counter += len(peaks)
    return all_peaks


def linspace100(a, b):
    """np.linspace(a, b, num=100) for integer endpoints: arange * (delta / 99) + a, the last sample set to b"""
    delta = np.float64(b - a)
    step = delta / 99
    y = np.arange(0, MID_NUM, dtype=np.float64)
    if step == 0:
        y = y / 99 * delta
    else:
        y = y * step
    y = y + a
    y[-1] = b
    return y


def score_pair(paf_avg, k, ax, ay, bx, by, H):
    """body.py:143-163 for one candidate pair -> (score_with_dist_prior, number of samples > thre2)"""
    vx, vy = bx - ax, by - ay
    norm = math.sqrt(vx * vx + vy * vy)
    if norm == 0:
        norm = 0.1
    ux, uy = vx / norm, vy / norm
    xs, ys = linspace100(ax, bx), linspace100(ay, by)
    xi = np.array([int(round(v)) for v in xs])
    yi = np.array([int(round(v)) for v in ys])
    cx, cy = MAP_IDX[k][0] - 19, MAP_IDX[k][1] - 19
    mid = np.multiply(paf_avg[yi, xi, cx], ux) + np.multiply(paf_avg[yi, xi, cy], uy)
    score = sum(mid.tolist()) / len(mid) + min(0.5 * H / norm - 1, 0)
    return score, int(np.count_nonzero(mid > THRE2))


def assemble(all_peaks, pair_scores, H):
    """body.py:136-238 given the peaks and a scorer pair_scores(list of (k, ax, ay, bx, by)) -> (scores, counts) -> (candidate, subset)"""
    jobs = []
    for k in range(len(MAP_IDX)):
        candA, candB = all_peaks[LIMB_SEQ[k][0] - 1], all_peaks[LIMB_SEQ[k][1] - 1]
        for i in range(len(candA)):
            for j in range(len(candB)):
                jobs.append((k, candA[i][0], candA[i][1], candB[j][0], candB[j][1]))
    scores, counts = pair_scores(jobs) if jobs else ([], [])
    at = 0
    connection_all, special_k = [], []
    for k in range(len(MAP_IDX)):
        candA, candB = all_peaks[LIMB_SEQ[k][0] - 1], all_peaks[LIMB_SEQ[k][1] - 1]
        nA, nB = len(candA), len(candB)
        if nA != 0 and nB != 0:
            cc = []
            for i in range(nA):
                for j in range(nB):
                    s, c = float(scores[at]), int(counts[at])
                    at += 1
                    if c > 0.8 * MID_NUM and s > 0:
                        cc.append([i, j, s, s + candA[i][2] + candB[j][2]])
            cc = sorted(cc, key=lambda x: x[2], reverse=True)
            connection = np.zeros((0, 5))
            for i, j, s, _ in cc:
                if i not in connection[:, 3] and j not in connection[:, 4]:
                    connection = np.vstack([connection, [candA[i][3], candB[j][3], s, i, j]])
                    if len(connection) >= min(nA, nB):
                        break
            connection_all.append(connection)
        else:
            special_k.append(k)
            connection_all.append([])
    subset = -1 * np.ones((0, 20))
    candidate = np.array([item for sublist in all_peaks for item in sublist])
    for k in range(len(MAP_IDX)):
        if k in special_k:
            continue
        partAs, partBs = connection_all[k][:, 0], connection_all[k][:, 1]
        indexA, indexB = np.array(LIMB_SEQ[k]) - 1
        for i in range(len(connection_all[k])):
            found, subset_idx = 0, [-1, -1]
            for j in range(len(subset)):
                if subset[j][indexA] == partAs[i] or subset[j][indexB] == partBs[i]:
                    subset_idx[found] = j
                    found += 1
            if found == 1:
                j = subset_idx[0]
                if subset[j][indexB] != partBs[i]:
                    subset[j][indexB] = partBs[i]
                    subset[j][-1] += 1
                    subset[j][-2] += candidate[partBs[i].astype(int), 2] + connection_all[k][i][2]
            elif found == 2:
                j1, j2 = subset_idx
                membership = ((subset[j1] >= 0).astype(int) + (subset[j2] >= 0).astype(int))[:-2]
                if len(np.nonzero(membership == 2)[0]) == 0:
                    subset[j1][:-2] += (subset[j2][:-2] + 1)
                    subset[j1][-2:] += subset[j2][-2:]
                    subset[j1][-2] += connection_all[k][i][2]
                    subset = np.delete(subset, j2, 0)
                else:
                    subset[j1][indexB] = partBs[i]
                    subset[j1][-1] += 1
                    subset[j1][-2] += candidate[partBs[i].astype(int), 2] + connection_all[k][i][2]
            elif not found and k < 17:
                row = -1 * np.ones(20)
                row[indexA], row[indexB] = partAs[i], partBs[i]
                row[-1] = 2
                row[-2] = sum(candidate[connection_all[k][i, :2].astype(int), 2]) + connection_all[k][i][2]
                subset = np.vstack([subset, row])
    delete = [i for i in range(len(subset)) if subset[i][-1] < 4 or subset[i][-2] / subset[i][-1] < 0.4]
    return candidate, np.delete(subset, delete, axis=0)


def postprocess(heat_avg, paf_avg):
    """body.py:103-238 in numpy: (candidate [N, 4], subset [P, 20]) from the accumulated float64 maps"""
    H = heat_avg.shape[0]
    peaks = find_peaks(heat_avg)

    def scorer(jobs):
        res = [score_pair(paf_avg, *j, H) for j in jobs]
        return [r[0] for r in res], [r[1] for r in res]
    return assemble(peaks, scorer, H)


# ---------------------------------------------------------------------------------------------------------------------------------
# infer_openpose.py's layout
# ---------------------------------------------------------------------------------------------------------------------------------
def get_pose(candidate, subset):
    """body.get_pose: per person [18, 3] (x, y, score), zeros for missing parts"""
    poses = []
    for item in subset:
        p = np.zeros((18, 3))
        for i in range(18):
            idx = int(item[i])
            if idx != -1:
                p[i] = candidate[idx][0:3]
        poses.append(p)
    return poses


def pose25(candidate, subset):
    """infer_openpose.py:19-27,57-70: per person BODY_25 [25, 3] float32 (neck, mid-hip and feet stay 0)"""
    out = []
    for p in get_pose(candidate, subset):
        coco = np.float32(p[list(COCO17_FROM_18)])
        b25 = np.zeros((25, 3))
        b25[list(BODY25_FROM_17)] = coco
        out.append(b25)
    return out


def write_json(path, people):
    """infer_openpose.py:60-82: {"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": [75 floats]}]}"""
    obj = {"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": np.asarray(p).flatten().tolist()} for p in people]}
    with open(path, "w") as f:
        f.write(json.dumps(obj))


def select_person(people):
    """io.load_openpose's choice among one view's people (only_one): {'pose': [25, 3]} of the person whose confidence sum is strictly
    largest, starting from entry 0 at score 0; None without people"""
    if not people:
        return None
    best, best_score = 0, 0
    for i, p in enumerate(people):
        conf = np.asarray(p)[:, -1]
        if np.abs(conf).max() <= 0:       # io._openpose_array drops an all-zero-confidence person's pose entry
            continue
        s = conf.sum()
        if s > best_score:
            best, best_score = i, s
    return {"pose": np.asarray(people[best], np.float64)}


def check_image(image):
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"OpenPose takes uint8 BGR images [H, W, 3]; got {a.dtype} {a.shape}")
    return a


class OpenPose:
    """OpenPose(weights=None, device=0, max_batch=8, max_h=1024, max_w=1024): the body estimator with its weights resident.
    `weights`: a state dict in the caffe-key layout, a path to body_pose_model.pth, or None for `assets.get_openpose()`.
    Images are uint8 BGR [H, W, 3] (what cv2.imread returns); one call takes images of one size."""

    def __init__(self, weights=None, device=0, max_batch=8, max_h=1024, max_w=1024):
        import ctypes as C
        if weights is None:
            from . import assets
            packed = assets.get_openpose()
        elif isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            packed = pack(load_weights(weights))
        else:
            packed = pack(match_state(weights))
        self._lib = _lib.load()
        n = int(self._lib.bf_openpose_n_weights())
        if packed.size != n:
            raise ValueError(f"{packed.size} packed OpenPose weights, the network has {n}")
        self.device, self.max_batch, self.max_h, self.max_w = int(device), int(max_batch), int(max_h), int(max_w)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_openpose_create(self.device, _lib.fptr(packed), n, self.max_batch, self.max_h, self.max_w,
                                                C.byref(self._h)), "bf_openpose_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bf_openpose_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _batch(self, images):
        if isinstance(images, np.ndarray) and images.ndim == 3:
            images = [images]
        imgs = [check_image(im) for im in images]
        if len({im.shape for im in imgs}) != 1:
            raise ValueError("OpenPose: one call takes images of one size")
        return np.ascontiguousarray(np.stack(imgs))

    @staticmethod
    def _u8(a):
        import ctypes as C
        return a.ctypes.data_as(C.POINTER(C.c_uint8))

    def _chunks(self, a):
        for s in range(0, len(a), self.max_batch):
            yield s, np.ascontiguousarray(a[s:s + self.max_batch])

    def maps(self, images):
        """-> (heatmap_avg float64 [n, H, W, 19], paf_avg float64 [n, H, W, 38]) as body.py:101-102 leaves them"""
        a = self._batch(images)
        n, H, W = a.shape[:3]
        heat, paf = np.zeros((n, H, W, N_HEAT)), np.zeros((n, H, W, N_PAF))
        for s, c in self._chunks(a):
            hh, pp = np.zeros((len(c), H, W, N_HEAT)), np.zeros((len(c), H, W, N_PAF))
            _lib.check(self._lib.bf_openpose_maps(self._h, len(c), H, W, self._u8(c), _dptr(hh), _dptr(pp)), "bf_openpose_maps")
            heat[s:s + len(c)], paf[s:s + len(c)] = hh, pp
        return heat, paf

    def network(self, images):
        """the per-scale stage-6 outputs: a list (one per scale) of float32 [n, Hp/8, Wp/8, 57] (paf 0:38, heat 38:57), and the
        per-scale network inputs float32 [n, Hp, Wp, 3]"""
        a = self._batch(images)
        n, H, W = a.shape[:3]
        dims = scale_dims(H, W)
        outs = [np.zeros((n, d[2] // 8, d[3] // 8, N_OUT), np.float32) for d in dims]
        ins = [np.zeros((n, d[2], d[3], 4), np.float32) for d in dims]
        for s, c in self._chunks(a):
            o = np.zeros(sum(len(c) * x[0].size for x in outs), np.float32)
            i = np.zeros(sum(len(c) * x[0].size for x in ins), np.float32)
            _lib.check(self._lib.bf_openpose_network(self._h, len(c), H, W, self._u8(c), _lib.fptr(i), _lib.fptr(o)), "bf_openpose_network")
            ao = ai = 0
            for m in range(len(dims)):
                k = len(c) * outs[m][0].size
                outs[m][s:s + len(c)] = o[ao:ao + k].reshape((len(c),) + outs[m].shape[1:])
                ao += k
                k = len(c) * ins[m][0].size
                ins[m][s:s + len(c)] = i[ai:ai + k].reshape((len(c),) + ins[m].shape[1:])
                ai += k
        return outs, [x[..., :3] for x in ins]

    def inject(self, outputs, H, W):
        """the maps from injected per-scale stage-6 outputs (float32 [n, Hp/8, Wp/8, 57] per scale): runs everything after the
        network and leaves the maps resident for peaks() / pairs(); -> (heat, paf) float64"""
        n = outputs[0].shape[0]
        flat = np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).reshape(-1) for o in outputs]))
        heat, paf = np.zeros((n, H, W, N_HEAT)), np.zeros((n, H, W, N_PAF))
        _lib.check(self._lib.bf_openpose_inject(self._h, n, H, W, _lib.fptr(flat), int(flat.size), _dptr(heat), _dptr(paf)),
                   "bf_openpose_inject")
        return heat, paf

    def peaks(self, n, blurred=False):
        """on the resident maps of the last maps() / inject(): per view all_peaks (body.py:104-128), and the filtered heatmaps
        float64 [n, H, W, 18] when blurred"""
        import ctypes as C
        counts = np.zeros(n, np.int32)
        pk = np.zeros((n, PEAK_CAP, 3), np.int32)
        sc = np.zeros((n, PEAK_CAP), np.float64)
        H, W = self._last_hw()
        bl = np.zeros((n, H, W, 18)) if blurred else None
        _lib.check(self._lib.bf_openpose_peaks(self._h, n, PEAK_CAP, _dptr(bl), _lib.iptr(counts), _lib.iptr(pk), _dptr(sc)),
                   "bf_openpose_peaks")
        out = []
        for b in range(n):
            c = int(counts[b])
            p, s = pk[b, :c], sc[b, :c]
            order = np.lexsort((p[:, 0], p[:, 1], p[:, 2]))               # part, then row-major: np.nonzero's order
            all_peaks, counter = [], 0
            for part in range(18):
                sel = [i for i in order if p[i, 2] == part]
                all_peaks.append([(int(p[i, 0]), int(p[i, 1]), float(s[i]), counter + t) for t, i in enumerate(sel)])
                counter += len(sel)
            out.append(all_peaks)
        return (out, bl) if blurred else out

    def _last_hw(self):
        import ctypes as C
        hw = np.zeros(2, np.int32)
        _lib.check(self._lib.bf_openpose_map_size(self._h, _lib.iptr(hw)), "bf_openpose_map_size")
        return int(hw[0]), int(hw[1])

    def pairs(self, view, jobs):
        """limb scores on the resident paf_avg of one view: jobs [(k, ax, ay, bx, by)] -> (score_with_dist_prior, count > thre2)"""
        J = np.ascontiguousarray(np.asarray(jobs, np.int32).reshape(-1, 5))
        score, cnt = np.zeros(len(J)), np.zeros(len(J), np.int32)
        if len(J):
            _lib.check(self._lib.bf_openpose_pairs(self._h, int(view), len(J), _lib.iptr(J), _dptr(score), _lib.iptr(cnt)), "bf_openpose_pairs")
        return score, cnt

    def _detect_resident(self, n):
        H, _ = self._last_hw()
        res = []
        for b, all_peaks in enumerate(self.peaks(n)):
            res.append(assemble(all_peaks, lambda jobs, b=b: self.pairs(b, jobs), H))
        return res

    def detect_many(self, images):
        """Body.__call__ per image -> list of (candidate, subset)"""
        a = self._batch(images)
        n, H, W = a.shape[:3]
        out = []
        for _, c in self._chunks(a):
            _lib.check(self._lib.bf_openpose_maps(self._h, len(c), H, W, self._u8(c), None, None), "bf_openpose_maps")
            out += self._detect_resident(len(c))
        return out

    def detect(self, image):
        """Body.__call__(oriImg) -> (candidate [N, 4], subset [P, 20])"""
        return self.detect_many([image])[0]

    def pose25(self, images):
        """per view the people as BODY_25 [25, 3] float32-valued arrays (infer_openpose.py's layout)"""
        return [pose25(c, s) for c, s in self.detect_many(images)]

    write_json = staticmethod(write_json)


def _dptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def warn_drawing(what):
    """the drop-ins compute what the reference computes and skip its drawing / image writes; said once per process"""
    if what not in _WARNED:
        _WARNED.add(what)
        print(f"bodyfitting_amd.openpose: {what} is not reproduced (drawing and cv2.imwrite are out of scope)", file=sys.stderr)


_WARNED = set()
