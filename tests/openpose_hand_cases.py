"""Shared by tools/gen_openpose_hand_golden.py and the OpenPose hand tests: a torch restatement of the reference's handpose_model
forward (openpose/model.py:204-217), pinned to the imported module by tests/test_openpose_hand_model.py, the planted network outputs
Hand.__call__'s post-processing is tested on, and the planted body detections handDetect is tested on.

The planted outputs are built from one patch per bump (computed once, pasted at whole cells), so every machine builds the same bits
and two pastes of one patch are exact translates of each other."""
import numpy as np

PLANT_SIDE = 184                  # a square crop: the network sizes are 184, 368, 552 and 736, a cell is 8, 4, 8/3 and 2 pixels
NET_HW = (128, 32)                # the crop the network golden runs on (not square: 184 x 46 at the first scale)


def _bump(radius, amp):
    r = int(radius)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    d2 = (xx * xx + yy * yy) / float(r * r)
    return np.where(d2 < 1.0, amp * (1.0 - d2) * (1.0 - d2), 0.0).astype(np.float32)


def _paste(o, part, patch, cy, cx):
    r = patch.shape[0] // 2
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, o.shape[0]), max(cx - r, 0), min(cx + r + 1, o.shape[1])
    sub = patch[y0 - (cy - r):y1 - (cy - r), x0 - (cx - r):x1 - (cx - r)]
    o[y0:y1, x0:x1, part] = np.maximum(o[y0:y1, x0:x1, part], sub)


# part -> bumps (x, y, radius in crop pixels, amplitude); positions are multiples of 8 pixels, so whole cells at every scale
BUMPS = {
    0: [(64, 72, 16, 1.0)],
    1: [(40, 40, 8, 1.5), (120, 128, 40, 0.35)],         # the spike holds the maximum, the wide blob the larger sum
    2: [(48, 48, 16, 0.75), (112, 104, 16, 0.75)],       # one patch pasted twice: equal sums, the first label wins
    5: [(16, 168, 16, 0.5)],
    6: [(168, 16, 16, 0.9), (96, 96, 8, 0.6)],
    7: [(0, 0, 16, 0.7)],
    8: [(176, 176, 24, 0.4)],
    9: [(88, 24, 16, 0.25), (24, 88, 16, 0.3)],
}
for _p in range(10, 22):
    BUMPS[_p] = [(8 * (3 + (5 * _p) % 17), 8 * (2 + (7 * _p) % 19), 8 * (1 + _p % 3), 0.2 + 0.05 * (_p % 7))]
NEGATIVE_PART = 4                 # part 3 stays empty; part 4 holds a component whose values are all negative
NEG_COL, NEG_WIDTH = 2, 8         # (cells of the last scale) -eps left of NEG_COL, +A at NEG_COL, -B over the next NEG_WIDTH
NEG_EPS, NEG_A, NEG_B = 2.0 ** -10, 4.0, 4.0


def planted_outputs(side=PLANT_SIDE):
    """per scale float32 [hq, hq, 22] for a square crop of `side` pixels"""
    from bodyfitting_amd import openpose_hand as OH
    outs = []
    for m, (h, w, Hp, Wp) in enumerate(OH.hand_scale_dims(side, side)):
        hq, wq = Hp // 8, Wp // 8
        o = np.zeros((hq, wq, OH.N_MAP), np.float32)
        cell = side / hq                                   # crop pixels per cell
        for part, bumps in BUMPS.items():
            for x, y, r, a in bumps:
                _paste(o, part, _bump(max(1, round(r / cell)), a), int(round(y / cell)), int(round(x / cell)))
        if m == len(OH.SCALE_SEARCH) - 1:
            o[:, :NEG_COL, NEGATIVE_PART] = -NEG_EPS
            o[:, NEG_COL, NEGATIVE_PART] = NEG_A
            o[:, NEG_COL + 1:NEG_COL + 1 + NEG_WIDTH, NEGATIVE_PART] = -NEG_B
        outs.append(o)
    return outs


# handDetect on an image of DETECT_HW: COCO-18 joints (x, y) per person
DETECT_HW = (200, 300)
DETECT_PEOPLE = (
    {2: (100.0, 60.0), 3: (90.0, 90.5), 4: (85.25, 120.0), 5: (140.0, 60.0), 6: (150.0, 90.0), 7: (158.5, 118.75)},   # both hands
    {2: (220.0, 50.0), 3: (215.0, 75.0), 5: (250.0, 50.0), 6: (260.0, 80.0), 7: (268.0, 110.0)},                      # left only
    {2: (30.0, 40.0), 3: (18.0, 22.0), 4: (6.5, 5.0), 5: (280.0, 160.0), 6: (290.0, 178.0), 7: (297.0, 195.0)},       # clamped
    {2: (200.0, 150.0), 3: (203.0, 155.0), 4: (205.0, 158.0)},                                                        # < 20: dropped
    {0: (10.0, 190.0), 1: (12.0, 180.0)},                                                                             # no arms
)


def detect_inputs():
    """(candidate [N, 4], subset [P, 20]) as Body.__call__ lays them out for DETECT_PEOPLE"""
    cand, subset = [], []
    for person in DETECT_PEOPLE:
        row = -np.ones(20)
        for j, (x, y) in sorted(person.items()):
            row[j] = len(cand)
            cand.append([x, y, 0.9, len(cand)])
        row[-2], row[-1] = 1.0, len(person)
        subset.append(row)
    return np.array(cand), np.array(subset)


def handpose_forward(state, x, dtype):
    """handpose_model.forward on x [1, 3, H, W] (numpy, NCHW) with the caffe-keyed state dict, in `dtype` (torch.float32 / float64)
    -> [H/8, W/8, 22] numpy (Mconv7_stage6, no ReLU)"""
    import torch
    import torch.nn.functional as F
    from bodyfitting_amd import openpose_hand as OH
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}

    def conv(t, name):
        w = P[name + ".weight"]
        t = F.conv2d(t, w, P[name + ".bias"], padding=w.shape[-1] // 2)
        return t if name in OH.NO_RELU else torch.relu(t)

    with torch.no_grad():
        t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
        for v in OH.HAND_VGG:
            t = F.max_pool2d(t, 2, 2) if v == "pool" else conv(t, v[0])
        out1_0 = t
        out = conv(conv(out1_0, "conv6_1_CPM"), "conv6_2_CPM")
        for s in range(2, 7):
            u = torch.cat([out, out1_0], 1)
            for j in range(1, 8):
                u = conv(u, f"Mconv{j}_stage{s}")
            out = u
        return out[0].permute(1, 2, 0).numpy()
